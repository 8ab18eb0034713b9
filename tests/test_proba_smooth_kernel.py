"""Per-flow smoothing kernel (csrc/ensemble_kernels.hip proba_smooth_kernel)
and its CPU oracle ops.cpu.proba_smooth.

Exact cases: alpha in {1/2, 1/4} and probabilities in eighths, five calls on
the same state.  The first call copies eighths and every later one adds at
most two binary places (a * p and b * s with a, b in quarters), so every
product and every sum is a multiple of 2^-15 below 2: exact in f32 whether
or not the multiply-add is fused.  state, held, labels and conf must then
equal the oracle's bit for bit after each call; the margins 0 and 1/16 and
the leads compared with them are exact too.

Inexact cases: alpha = 0.3 and Dirichlet rows over T = 8 calls against an
f64 recurrence that uses the same f32 a and b, atol = T * 2^-23.  Per call
the product b * s < 1 rounds by at most 2^-25 and the fused add of a value
<= 1 by at most 2^-24, under 2^-23 together, and the error inherited from
the call before shrinks by b < 1.  labels, held and conf are functions of
the returned state and the previous held, and are checked exactly.
"""

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd.ops import cpu as oc

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

ROWS = (1, 255, 256, 257, 1500)  # 256 rows per block: partial, full, second block
CLASSES = (2, 3, 4, 6, 8)  # scalar, float2 and float4 row paths


def _og():
    from traffic_classifier_sdn_amd.ops import gpu as og

    return og


def _caps(monkeypatch):
    for cap in (None, 2):
        if cap is None:
            monkeypatch.delenv("TCSDN_PROBA_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("TCSDN_PROBA_BLOCKS", str(cap))
        yield cap


def _eighths(rng, n, C):
    """Rows of C multiples of 1/8 that sum to 1."""
    cuts = np.sort(rng.integers(0, 9, size=(n, C - 1)), axis=1)
    parts = np.diff(np.concatenate([np.zeros((n, 1), int), cuts, np.full((n, 1), 8)], axis=1), axis=1)
    return torch.from_numpy((parts / 8.0).astype(np.float32))


def _fresh(cap, C, device="cpu"):
    return (torch.zeros(cap, C, dtype=torch.float32, device=device),
            torch.full((cap,), -1, dtype=torch.int32, device=device))


def _live(v, device="cpu"):
    return torch.tensor([v], dtype=torch.int32, device=device)


# ----------------------------------------------------------------------
# CPU oracle: one hand-written case per rule
# ----------------------------------------------------------------------


def test_oracle_first_sighting_copies_the_row():
    p = torch.tensor([[0.1, 0.7, 0.2], [0.3, 0.3, 0.4]])
    state, held = _fresh(3, 3)
    label, conf = oc.proba_smooth(p, state, held, 0.3, 0.1)
    assert label.dtype == torch.int32 and label.tolist() == [1, 2]
    assert conf.dtype == torch.float32 and torch.equal(conf, p.max(dim=1).values)
    assert torch.equal(state[:2], p)  # bit for bit, whatever alpha is
    assert held.tolist() == [1, 2, -1] and torch.equal(state[2], torch.zeros(3))


def test_oracle_one_ema_step():
    state = torch.tensor([[0.5, 0.25, 0.25]])
    held = torch.tensor([0], dtype=torch.int32)
    p = torch.tensor([[0.25, 0.5, 0.25]])
    label, conf = oc.proba_smooth(p, state, held, 0.25)
    # 0.25 * p + 0.75 * state
    assert torch.equal(state, torch.tensor([[0.4375, 0.3125, 0.25]]))
    assert label.tolist() == [0] and conf.tolist() == [0.4375] and held.tolist() == [0]
    # a and b are f32: 0.3 is rounded, and b = 1 - a in f32
    a = np.float32(0.3)
    b = np.float32(1.0) - a
    state = torch.tensor([[0.6, 0.4]])
    want = [float(np.float32(float(a) * float(np.float32(pv)) + float(b * np.float32(sv))))
            for pv, sv in ((0.2, 0.6), (0.8, 0.4))]
    oc.proba_smooth(torch.tensor([[0.2, 0.8]]), state, torch.tensor([0], dtype=torch.int32), 0.3)
    assert state[0].tolist() == want


def test_oracle_margin_holds_below_and_switches_above():
    p = torch.tensor([[0.25, 0.75]] * 2)
    # alpha = 1/2 on state (0.5, 0.25): s = (0.375, 0.5), a lead of 0.125,
    # which has to EXCEED the margin
    for margin, want_label, want_conf in (
        (0.0, 1, 0.5), (0.0625, 1, 0.5), (0.125, 0, 0.375), (0.25, 0, 0.375)
    ):
        state = torch.tensor([[0.5, 0.25]] * 2)
        held = torch.tensor([0, 0], dtype=torch.int32)
        label, conf = oc.proba_smooth(p, state, held, 0.5, margin)
        assert label.tolist() == [want_label] * 2, margin
        assert conf.tolist() == [want_conf] * 2, margin
        assert held.tolist() == [want_label] * 2, margin
        assert torch.equal(state, torch.tensor([[0.375, 0.5]] * 2)), margin


def test_oracle_exact_tie_keeps_the_held_label_against_a_lower_index():
    # s = (0.375, 0.375, 0.25): class 0 is the first maximum, class 1 is held
    state = torch.tensor([[0.25, 0.5, 0.25]])
    held = torch.tensor([1], dtype=torch.int32)
    label, conf = oc.proba_smooth(torch.tensor([[0.5, 0.25, 0.25]]), state, held, 0.5, 0.0)
    assert state[0].tolist() == [0.375, 0.375, 0.25]
    assert label.tolist() == [1] and held.tolist() == [1] and conf.tolist() == [0.375]
    # never seen: nothing is held, so the first maximum it is
    state, held = _fresh(1, 3)
    label, _ = oc.proba_smooth(torch.tensor([[0.375, 0.375, 0.25]]), state, held, 0.5, 0.0)
    assert label.tolist() == [0]


def test_oracle_conf_is_the_held_class_not_the_maximum():
    state = torch.tensor([[0.75, 0.25]])
    held = torch.tensor([0], dtype=torch.int32)
    label, conf = oc.proba_smooth(torch.tensor([[0.0, 1.0]]), state, held, 0.5, 0.5)
    # s = (0.375, 0.625): a lead of 0.25 does not exceed 0.5
    assert label.tolist() == [0] and conf.tolist() == [0.375]
    assert float(state.max()) == 0.625


def test_oracle_not_live_rows_are_reset():
    state = torch.tensor([[0.5, 0.5], [0.75, 0.25], [0.75, 0.25], [0.25, 0.75]])
    held = torch.tensor([0, 0, 0, 1], dtype=torch.int32)
    p = torch.tensor([[0.25, 0.75], [0.25, 0.75], [0.5, 0.5]])
    label, conf = oc.proba_smooth(p, state, held, 0.5, 0.25, _live(1))
    # row 0 live: s = (0.375, 0.625), lead 0.25 does not exceed the margin
    # rows 1, 2 not live: own first-maximum argmax and maximum, state gone
    # row 3 is past n: untouched
    assert label.tolist() == [0, 1, 0] and conf.tolist() == [0.375, 0.75, 0.5]
    assert state.tolist() == [[0.375, 0.625], [0.0, 0.0], [0.0, 0.0], [0.25, 0.75]]
    assert held.tolist() == [0, -1, -1, 1]
    # a count past n means all n rows: row 0 moves on to (0.3125, 0.6875),
    # a lead of 0.375 that switches it; rows 1, 2 are first sightings
    label, _ = oc.proba_smooth(p, state, held, 0.5, 0.25, _live(100))
    assert held.tolist() == [1, 1, 0, 1] and label.tolist() == [1, 1, 0]
    assert torch.equal(state[1:3], p[1:3])


def test_oracle_alpha_one_is_the_rows_own_argmax():
    rng = np.random.default_rng(5)
    n, C = 500, 5
    state, held = _fresh(n, C)
    for call in range(3):
        p = torch.from_numpy(rng.dirichlet(np.ones(C), size=n).astype(np.float32))
        p[:8] = p[:8, [0]]  # ties: the first maximum
        label, conf = oc.proba_smooth(p, state, held, 1.0, 0.0)
        best = p.max(dim=1).values
        first = torch.argmax((p == best.unsqueeze(1)).to(torch.uint8), dim=1)
        if call == 0:
            assert torch.equal(label, first.to(torch.int32))
        else:  # an exact tie with the held class keeps it: the value is the same
            moved = label.long() != first
            assert bool((p.gather(1, label.long().unsqueeze(1)).squeeze(1)[moved] == best[moved]).all())
        assert torch.equal(conf, best)  # bit for bit
        assert torch.equal(state, p)


def _bad_cases(device="cpu"):
    """(name, kwargs) of every refusal; fresh tensors per call."""
    def base(n=3, C=3, cap=4):
        state, held = _fresh(cap, C, device)
        state += 0.125
        held += 1
        return dict(proba=torch.full((n, C), 1.0 / C, device=device), state=state, held=held,
                    alpha=0.5, margin=0.0, n_live=None)

    def alias():
        kw = base()
        kw["proba"] = kw["state"][:3]
        return kw

    cases = [
        ("one class", lambda: base(C=1)),
        ("nine classes", lambda: base(C=9)),
        ("cap < n", lambda: base(n=5)),
        ("held shorter than n", lambda: {**base(), "held": torch.zeros(2, dtype=torch.int32, device=device)}),
        ("state columns", lambda: {**base(), "state": torch.zeros(4, 4, device=device)}),
        ("f64 proba", lambda: {**base(), "proba": torch.full((3, 3), 1 / 3, dtype=torch.float64, device=device)}),
        ("f64 state", lambda: {**base(), "state": torch.zeros(4, 3, dtype=torch.float64, device=device)}),
        ("int64 held", lambda: {**base(), "held": torch.zeros(4, dtype=torch.int64, device=device)}),
        ("strided proba", lambda: {**base(), "proba": torch.full((3, 6), 1 / 3, device=device)[:, ::2]}),
        ("strided state", lambda: {**base(), "state": torch.zeros(4, 6, device=device)[:, ::2]}),
        ("strided held", lambda: {**base(), "held": torch.zeros(8, dtype=torch.int32, device=device)[::2]}),
        ("proba is state", alias),
        ("int64 n_live", lambda: {**base(), "n_live": torch.tensor([2], device=device)}),
        ("n_live of two", lambda: {**base(), "n_live": torch.tensor([2, 2], dtype=torch.int32, device=device)}),
        ("n_live an int", lambda: {**base(), "n_live": 2}),
        ("alpha 0", lambda: {**base(), "alpha": 0.0}),
        ("alpha negative", lambda: {**base(), "alpha": -0.5}),
        ("alpha above 1", lambda: {**base(), "alpha": 1.0000001}),
        ("alpha nan", lambda: {**base(), "alpha": float("nan")}),
        ("alpha vanishing in f32", lambda: {**base(), "alpha": 1e-60}),
        ("margin negative", lambda: {**base(), "margin": -0.125}),
        ("margin nan", lambda: {**base(), "margin": float("nan")}),
        ("margin inf", lambda: {**base(), "margin": float("inf")}),
    ]
    if device != "cpu":
        cases.append(("state on the host", lambda: {**base(), "state": torch.zeros(4, 3)}))
        cases.append(("n_live on the host", lambda: {**base(), "n_live": _live(2)}))
    return cases


def _assert_refused(fn, make):
    kw = make()
    state0, held0 = kw["state"].clone(), kw["held"].clone()
    with pytest.raises(ValueError):
        fn(kw["proba"], kw["state"], kw["held"], kw["alpha"], kw["margin"], kw["n_live"])
    assert torch.equal(kw["state"], state0) and torch.equal(kw["held"], held0)


@pytest.mark.parametrize("case", _bad_cases(), ids=[c[0] for c in _bad_cases()])
def test_oracle_refusals_leave_state_untouched(case):
    _assert_refused(oc.proba_smooth, case[1])


def test_oracle_no_rows():
    state, held = _fresh(2, 3)
    label, conf = oc.proba_smooth(torch.zeros(0, 3), state, held, 0.5)
    assert label.shape == (0,) and label.dtype == torch.int32
    assert conf.shape == (0,) and conf.dtype == torch.float32


# ----------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
def test_gpu_refusals_leave_state_untouched():
    """The binding applies the oracle's rules, and the extension entry point
    has its own checks behind them."""
    og = _og()
    for name, make in _bad_cases("cuda"):
        _assert_refused(og.proba_smooth, make)
    state, held = _fresh(4, 3, "cuda")
    p = torch.full((3, 3), 1 / 3, device="cuda")
    ext = og._ext.proba_smooth
    for args in (
        (torch.full((3, 9), 1 / 9, device="cuda"), torch.zeros(4, 9, device="cuda"), held, None, 0.5, 0.0),
        (torch.full((5, 3), 1 / 3, device="cuda"), state, held, None, 0.5, 0.0),
        (p.double(), state, held, None, 0.5, 0.0),
        (state[:3], state, held, None, 0.5, 0.0),
        (p, state, held, torch.tensor([2], device="cuda"), 0.5, 0.0),
        (p, state, held, None, 0.0, 0.0),
        (p, state, held, None, 1.5, 0.0),
        (p, state, held, None, 0.5, -1.0),
        (p, state, held, None, 0.5, float("nan")),
    ):
        with pytest.raises(RuntimeError):
            ext(*args)
    assert not bool(state.any()) and bool((held == -1).all())
    label, conf = og.proba_smooth(torch.zeros(0, 3, device="cuda"), state, held, 0.5)
    assert label.shape == (0,) and conf.shape == (0,)


def _compare(tag, got, want):
    for name, g, w in zip(("labels", "conf"), got, want):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), f"{tag} {name}"


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
def test_exact_against_oracle(monkeypatch, C):
    og = _og()
    rng = np.random.default_rng(400 + C)
    calls = [_eighths(rng, max(ROWS), C) for _ in range(5)]
    # exact ties at the second call between the held last class and class 0,
    # which is the first maximum: rows 0..3 under alpha 1/2 (0.5 each), rows
    # 4..7 under alpha 1/4 (7/32 + 9/32 against 1/32 + 15/32)
    calls[0][:8] = 0.0
    calls[1][:8] = 0.0
    calls[0][:4, C - 1] = 1.0
    calls[1][:4, 0] = 1.0
    calls[0][4:8, 0], calls[0][4:8, C - 1] = 0.375, 0.625
    calls[1][4:8, 0], calls[1][4:8, C - 1] = 0.875, 0.125
    ties = {0.5: slice(0, 4), 0.25: slice(4, 8)}
    dev_calls = [p.cuda() for p in calls]
    for cap in _caps(monkeypatch):
        for n in ROWS:
            for alpha, margin in ((0.5, 0.0), (0.5, 0.0625), (0.25, 0.0), (0.25, 0.0625)):
                rows = n + 3  # rows past n stay as they are
                ref_s, ref_h = _fresh(rows, C)
                ref_s[n:], ref_h[n:] = 0.375, 1
                state, held = ref_s.cuda(), ref_h.cuda()
                for k, (p, dp) in enumerate(zip(calls, dev_calls)):
                    tag = f"C {C} cap {cap} n {n} alpha {alpha} call {k}"
                    want = oc.proba_smooth(p[:n], ref_s, ref_h, alpha, margin)
                    got = og.proba_smooth(dp[:n], state, held, alpha, margin)
                    _compare(tag, got, want)
                    assert torch.equal(state.cpu(), ref_s), tag
                    assert torch.equal(held.cpu(), ref_h), tag
                    if k == 1:  # the oracle's ties are real, and the held label stood
                        t = ref_s[:n][ties[alpha]]
                        assert torch.equal(t[:, 0], t[:, C - 1]), tag
                        assert bool((t[:, 0] == t.max(dim=1).values).all()), tag
                        assert bool((ref_h[:n][ties[alpha]] == C - 1).all()), tag
                assert bool((ref_s[n:] == 0.375).all()) and bool((ref_h[n:] == 1).all())


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
def test_exact_with_a_growing_live_count(monkeypatch, C):
    """Rows go from reset to first sighting to averaged as n_live grows."""
    og = _og()
    rng = np.random.default_rng(500 + C)
    n = max(ROWS)
    lives = (100, 257, 257, 1500, 1500)
    calls = [_eighths(rng, n, C) for _ in lives]
    for cap in _caps(monkeypatch):
        ref_s, ref_h = _fresh(n, C)
        ref_s += 0.25  # stale contents: a reset must clear them
        ref_h += 1
        state, held = ref_s.cuda(), ref_h.cuda()
        d_live = _live(0, "cuda")
        for k, (p, live) in enumerate(zip(calls, lives)):
            tag = f"C {C} cap {cap} call {k} live {live}"
            d_live.fill_(live)
            want = oc.proba_smooth(p, ref_s, ref_h, 0.25, 0.0625, _live(live))
            got = og.proba_smooth(p.cuda(), state, held, 0.25, 0.0625, d_live)
            _compare(tag, got, want)
            assert torch.equal(state.cpu(), ref_s), tag
            assert torch.equal(held.cpu(), ref_h), tag
            assert bool((ref_h[live:] == -1).all()) and not bool(ref_s[live:].any()), tag
            assert bool((ref_h[:live] >= 0).all()), tag


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 6, 8])
def test_inexact_against_f64(monkeypatch, C):
    og = _og()
    rng = np.random.default_rng(600 + C)
    n, T = max(ROWS), 8
    alpha, margin = 0.3, 0.1
    a = float(np.float32(alpha))
    b = float(np.float32(1.0) - np.float32(alpha))
    m32 = np.float32(margin)
    calls = [torch.from_numpy(rng.dirichlet(np.ones(C), size=n).astype(np.float32)) for _ in range(T)]
    atol = T * 2.0 ** -23
    for cap in _caps(monkeypatch):
        for rows in ROWS:
            state, held = _fresh(rows, C, "cuda")
            ref = None
            for k, p in enumerate(calls):
                tag = f"C {C} cap {cap} n {rows} call {k}"
                prev_h = held.cpu().long()
                label, conf = og.proba_smooth(p[:rows].cuda(), state, held, alpha, margin)
                ref = p[:rows].double() if ref is None else a * p[:rows].double() + b * ref
                s = state.cpu()
                err = float((s.double() - ref).abs().max())
                if k == T - 1:
                    print(f"{tag}: max err {err:.3e} (atol {atol:.3e})")
                assert err <= atol, tag
                # the verdict, exactly, from the returned state and the held before
                best = s.max(dim=1).values
                top = torch.argmax((s == best.unsqueeze(1)).to(torch.uint8), dim=1)
                sh = s.gather(1, prev_h.clamp(min=0).unsqueeze(1)).squeeze(1)
                lead = (best.numpy() - sh.numpy()).astype(np.float32)
                keep = (prev_h >= 0) & ~torch.from_numpy(lead > m32)
                want = torch.where(keep, prev_h, top)
                assert torch.equal(label.cpu().long(), want), tag
                assert torch.equal(held.cpu().long(), want), tag
                assert torch.equal(conf.cpu(), s.gather(1, want.unsqueeze(1)).squeeze(1)), tag


@needs_gpu
@pytest.mark.gpu
def test_smooth_captures():
    """No sync and no allocation beyond the outputs: one capture, replayed
    with changing proba and n_live contents, equals the eager calls."""
    og = _og()
    rng = np.random.default_rng(700)
    n, C = 2048, 6
    lives = (700, 2048, 1500, 2048)
    calls = [_eighths(rng, n, C).cuda() for _ in lives]
    state, held = _fresh(n, C, "cuda")
    static_p = calls[0].clone()
    d_live = _live(n, "cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            og.proba_smooth(static_p, state, held, 0.25, 0.0625, d_live)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = og.proba_smooth(static_p, state, held, 0.25, 0.0625, d_live)
    state.zero_()
    held.fill_(-1)
    ref_s, ref_h = _fresh(n, C, "cuda")
    for k, (p, live) in enumerate(zip(calls, lives)):
        static_p.copy_(p)
        d_live.fill_(live)
        g.replay()
        torch.cuda.synchronize()
        want = og.proba_smooth(p, ref_s, ref_h, 0.25, 0.0625, _live(live, "cuda"))
        for got, w in zip(out, want):
            assert torch.equal(got, w), k
        assert torch.equal(state, ref_s) and torch.equal(held, ref_h), k
