"""Per-class traffic accounting (csrc/traffic_kernels.hip) and its CPU oracle
ops.cpu.class_traffic.

Exact cases: integer-valued f32 features below 2^20.  With at most 1500 rows
every partial sum stays below 2^31, far under 2^53, so every summation order
is exact in f64 and the kernel's totals must equal the oracle's bit for bit.

Inexact cases: features exp(N(8, 4)) as f32.  The kernel and the oracle each
add the m_g rows of a group in some order, and any order of a k-term f64 sum
is within (k - 1) u sum|x| of the true sum, u = 2^-53.  With m live rows,
m_g <= m, so per cell
    |gpu - oracle| <= m * 2^-52 * sum over the group's rows of |X[r, j]|
the right-hand sum formed in f64 here.  Column 0 counts rows and is exact.
"""

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import ops
from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.utils.schema import FEATURE_NAMES

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# a wave takes 64 rows and a block 256: partial, full and second tiles of both
ROWS = (1, 63, 64, 65, 255, 256, 257, 1500)
CLASSES = (2, 6, 8)


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


def _live(v, device="cpu"):
    return torch.tensor([v], dtype=torch.int32, device=device)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _rows(values):
    """[n, 12] f32 with row r = values[r] + column index."""
    v = torch.tensor(values, dtype=torch.float32).unsqueeze(1)
    return (v + torch.arange(12, dtype=torch.float32)).contiguous()


# ----------------------------------------------------------------------
# CPU oracle: one hand-written case per rule
# ----------------------------------------------------------------------


def test_columns_are_the_count_and_the_schema():
    assert oc.TRAFFIC_COLUMNS == ("flows",) + FEATURE_NAMES
    assert ops.TRAFFIC_COLUMNS is oc.TRAFFIC_COLUMNS
    assert len(oc.TRAFFIC_COLUMNS) == 13


def test_oracle_counts_and_sums_five_rows():
    X = _rows([10.0, 20.0, 30.0, 40.0, 50.0])
    t = oc.class_traffic(X, _i32([0, 2, 0, 1, 2]), 3)
    assert t.dtype == torch.float64 and tuple(t.shape) == (4, 13)
    assert t[:, 0].tolist() == [2.0, 1.0, 2.0, 0.0]
    j = torch.arange(12, dtype=torch.float64)
    assert torch.equal(t[0, 1:], 40.0 + 2 * j)  # rows 0 and 2
    assert torch.equal(t[1, 1:], 40.0 + j)  # row 3
    assert torch.equal(t[2, 1:], 70.0 + 2 * j)  # rows 1 and 4
    assert not bool(t[3].any())


def test_oracle_out_of_range_labels_are_unknown():
    X = _rows([1.0, 2.0, 4.0, 8.0])
    t = oc.class_traffic(X, _i32([-1, 3, 2**31 - 1, 1]), 3)
    assert t[:, 0].tolist() == [0.0, 1.0, 0.0, 3.0]
    assert float(t[3, 1]) == 7.0 and float(t[1, 1]) == 8.0


def test_oracle_low_confidence_is_unknown_and_nan_is_not():
    X = _rows([1.0, 2.0, 4.0, 8.0])
    conf = torch.tensor([0.5, 0.25, float("nan"), 0.75])
    t = oc.class_traffic(X, _i32([0, 0, 0, 1]), 2, conf, 0.5)
    # 0.5 < 0.5 is false, 0.25 < 0.5 true, NaN < 0.5 false
    assert t[:, 0].tolist() == [2.0, 1.0, 1.0]
    assert float(t[0, 1]) == 5.0 and float(t[2, 1]) == 2.0
    # the comparison is made with f32(min_conf): 0.1f is above 0.1
    conf = torch.full((4,), 0.1)
    assert float(oc.class_traffic(X, _i32([0, 0, 0, 1]), 2, conf, 0.1)[2, 0]) == 0.0


@pytest.mark.parametrize("live, counted", [(0, 0), (1, 1), (4, 4), (9, 4)])
def test_oracle_n_live(live, counted):
    X = _rows([1.0, 2.0, 4.0, 8.0])
    X[live:] = float("nan")  # a dead row's values reach no sum
    lab = _i32([0, 1, 1, 0])
    t = oc.class_traffic(X, lab, 2, n_live=_live(live))
    assert float(t[:, 0].sum()) == counted
    assert bool(torch.isfinite(t).all())
    if live == 1:
        assert float(t[0, 1]) == 1.0 and not bool(t[1:].any())
    if live >= 4:
        assert torch.equal(t, oc.class_traffic(X, lab, 2))


def test_oracle_no_rows():
    t = oc.class_traffic(torch.zeros(0, 12), _i32([]), 6)
    assert t.dtype == torch.float64 and tuple(t.shape) == (7, 13) and not bool(t.any())


def test_oracle_a_nan_lands_in_one_cell():
    X = _rows([1.0, 2.0, 4.0, 8.0, 16.0])
    X[1, 4] = float("nan")
    X[3, 7] = float("inf")
    t = oc.class_traffic(X, _i32([0, 1, 2, 0, 9]), 3)
    bad = ~torch.isfinite(t)
    assert bad.nonzero().tolist() == [[0, 8], [1, 5]]
    assert torch.isnan(t[1, 5]) and float(t[0, 8]) == float("inf")
    clean = oc.class_traffic(_rows([1.0, 2.0, 4.0, 8.0, 16.0]), _i32([0, 1, 2, 0, 9]), 3)
    assert torch.equal(t[~bad], clean[~bad])


def _bad_cases(device):
    X = torch.zeros(4, 12, device=device)
    lab = torch.zeros(4, dtype=torch.int32, device=device)
    conf = torch.zeros(4, device=device)
    other = "cpu" if device != "cpu" else "meta"
    return [
        ("one class", lambda: (X, lab, 1)),
        ("nine classes", lambda: (X, lab, 9)),
        ("float class count", lambda: (X, lab, 3.0)),
        ("11 features", lambda: (X[:, :11].contiguous(), lab, 3)),
        ("flat X", lambda: (X.reshape(-1), lab, 3)),
        ("f64 X", lambda: (X.double(), lab, 3)),
        ("int64 labels", lambda: (X, lab.long(), 3)),
        ("short labels", lambda: (X, lab[:3], 3)),
        ("strided X", lambda: (torch.zeros(4, 24, device=device)[:, ::2], lab, 3)),
        ("strided labels", lambda: (X, torch.zeros(8, dtype=torch.int32, device=device)[::2], 3)),
        ("labels elsewhere", lambda: (X, lab.to(other), 3)),
        ("f64 conf", lambda: (X, lab, 3, conf.double(), 0.5)),
        ("short conf", lambda: (X, lab, 3, conf[:3], 0.5)),
        ("conf elsewhere", lambda: (X, lab, 3, conf.to(other), 0.5)),
        ("nan min_conf", lambda: (X, lab, 3, conf, float("nan"))),
        ("inf min_conf", lambda: (X, lab, 3, conf, float("inf"))),
        ("min_conf past f32", lambda: (X, lab, 3, conf, 1e39)),
        ("int n_live", lambda: (X, lab, 3, None, 0.0, 2)),
        ("int64 n_live", lambda: (X, lab, 3, None, 0.0, torch.tensor([2], device=device))),
        ("scalar n_live", lambda: (X, lab, 3, None, 0.0, torch.tensor(2, dtype=torch.int32, device=device))),
        ("n_live elsewhere", lambda: (X, lab, 3, None, 0.0, _live(2, other))),
    ]


@pytest.mark.parametrize("case", _bad_cases("cpu"), ids=lambda c: c[0])
def test_oracle_refusals(case):
    with pytest.raises(ValueError):
        oc.class_traffic(*case[1]())


# ----------------------------------------------------------------------
# GPU against the oracle
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
def test_gpu_refusals():
    og = _og()
    for name, make in _bad_cases("cuda"):
        with pytest.raises(ValueError):
            og.class_traffic(*make())
    # the extension entry point has its own checks behind the shared ones
    X = torch.zeros(4, 12, device="cuda")
    lab = torch.zeros(4, dtype=torch.int32, device="cuda")
    ext = og._ext.class_traffic
    with pytest.raises(RuntimeError, match="no kernel for"):
        ext(X, lab, 9, None, 0.0, None)
    with pytest.raises(RuntimeError, match="no kernel for"):
        ext(X, lab, 1, None, 0.0, None)
    for args in (
        (X.double(), lab, 3, None, 0.0, None),
        (X, lab[:3], 3, None, 0.0, None),
        (X, lab, 3, torch.zeros(3, device="cuda"), 0.0, None),
        (X, lab, 3, None, float("nan"), None),
        (X, lab, 3, None, 0.0, torch.tensor([2], device="cuda")),
    ):
        with pytest.raises(RuntimeError):
            ext(*args)


def _labels(rng, n, C):
    """Mostly classes, with out-of-range values of every kind mixed in."""
    lab = rng.integers(0, C, size=n).astype(np.int64)
    odd = rng.random(n) < 0.15
    lab[odd] = rng.choice([-1, -(2**31), C, C + 1, 2**31 - 1], size=int(odd.sum()))
    return torch.from_numpy(lab.astype(np.int32))


def _conf(rng, n):
    conf = rng.random(n).astype(np.float32)
    conf[rng.random(n) < 0.05] = np.nan
    conf[rng.random(n) < 0.05] = 0.5  # equal to min_conf: not below it
    return torch.from_numpy(conf)


def _lives(n):
    return (None, 0, 1, n - 1, n)


def _cases(rng, C, make_X):
    n = max(ROWS)
    return make_X(rng, n), _labels(rng, n, C), _conf(rng, n)


def _integers(rng, n):
    return torch.from_numpy(rng.integers(0, 2**20, size=(n, 12)).astype(np.float32))


def _lognormal(rng, n):
    return torch.from_numpy(np.exp(rng.normal(8.0, 4.0, size=(n, 12))).astype(np.float32))


def _sweep(monkeypatch, C, X, lab, conf):
    """Yields (tag, n, live rows m, conf given, gpu totals, oracle totals) over
    the row counts, the block caps, conf given or not and the live counts."""
    og = _og()
    dX, dlab, dconf = X.cuda(), lab.cuda(), conf.cuda()
    want = {}
    for cap in _caps(monkeypatch):
        for n in ROWS:
            for use_conf in (False, True):
                for live in _lives(n):
                    key = (n, use_conf, live)
                    if key not in want:  # the oracle does not depend on the cap
                        want[key] = oc.class_traffic(
                            X[:n], lab[:n], C, conf[:n] if use_conf else None, 0.5,
                            None if live is None else _live(live),
                        )
                    got = og.class_traffic(
                        dX[:n], dlab[:n], C, dconf[:n] if use_conf else None, 0.5,
                        None if live is None else _live(live, "cuda"),
                    )
                    assert got.dtype == torch.float64 and tuple(got.shape) == (C + 1, 13)
                    tag = f"C {C} cap {cap} n {n} conf {use_conf} live {live}"
                    m = n if live is None else min(n, live)
                    yield tag, n, m, use_conf, got.cpu(), want[key]


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
def test_exact_against_oracle(monkeypatch, C):
    rng = np.random.default_rng(800 + C)
    X, lab, conf = _cases(rng, C, _integers)
    for tag, _, m, _, got, want in _sweep(monkeypatch, C, X, lab, conf):
        assert float(want[:, 0].sum()) == m, tag
        assert torch.equal(got, want), tag


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
def test_inexact_against_oracle(monkeypatch, C):
    rng = np.random.default_rng(900 + C)
    X, lab, conf = _cases(rng, C, _lognormal)
    worst = 0.0
    for tag, n, m, use_conf, got, want in _sweep(monkeypatch, C, X, lab, conf):
        assert torch.equal(got[:, 0], want[:, 0]), tag
        # sum |x| per cell: the oracle on |X| over the same rows and groups
        mag = oc.class_traffic(
            X[:n].abs(), lab[:n], C, conf[:n] if use_conf else None, 0.5, _live(m)
        )
        bound = m * 2.0 ** -52 * mag[:, 1:]
        err = (got[:, 1:] - want[:, 1:]).abs()
        ratio = float((err / bound.clamp(min=1e-300)).max()) if m else 0.0
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), f"{tag}: {ratio:.3e} of the bound"
    print(f"C {C}: largest |gpu - oracle| is {worst:.3e} of its bound")


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
def test_one_class_and_all_unknown(monkeypatch, C):
    og = _og()
    rng = np.random.default_rng(1000 + C)
    n = max(ROWS)
    X = _integers(rng, n)
    dX = X.cuda()
    sums = X.double().sum(dim=0)
    for cap in _caps(monkeypatch):
        for g, lab in ((C - 1, torch.full((n,), C - 1, dtype=torch.int32)),
                       (C, torch.full((n,), -7, dtype=torch.int32))):
            got = og.class_traffic(dX, lab.cuda(), C).cpu()
            want = torch.zeros(C + 1, 13, dtype=torch.float64)
            want[g, 0], want[g, 1:] = n, sums
            assert torch.equal(got, want), f"C {C} cap {cap} group {g}"
        # every confidence below the threshold: all unknown (the `want` just
        # above), whatever the label
        lab = _labels(rng, n, C)
        got = og.class_traffic(dX, lab.cuda(), C, torch.zeros(n, device="cuda"), 0.25).cpu()
        assert torch.equal(got, want), f"C {C} cap {cap} low confidence"


@needs_gpu
@pytest.mark.gpu
def test_gpu_a_nan_lands_in_one_cell(monkeypatch):
    og = _og()
    rng = np.random.default_rng(1100)
    n, C = 700, 6
    X, lab = _integers(rng, n), _labels(rng, n, C)
    X[333, 4] = float("nan")
    X[64, 11] = float("-inf")
    lab[333], lab[64] = 2, -1
    clean = oc.class_traffic(torch.nan_to_num(X, nan=0.0, neginf=0.0), lab, C)
    for cap in _caps(monkeypatch):
        got = og.class_traffic(X.cuda(), lab.cuda(), C).cpu()
        bad = ~torch.isfinite(got)
        assert bad.nonzero().tolist() == [[2, 5], [C, 12]], cap
        assert torch.isnan(got[2, 5]) and float(got[C, 12]) == float("-inf")
        assert torch.equal(got[~bad], clean[~bad]), cap


@needs_gpu
@pytest.mark.gpu
def test_no_rows_writes_zeros():
    og = _og()
    got = og.class_traffic(
        torch.zeros(0, 12, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), 6
    )
    assert got.dtype == torch.float64 and tuple(got.shape) == (7, 13) and not bool(got.any())


@needs_gpu
@pytest.mark.gpu
def test_two_calls_are_bit_identical(monkeypatch):
    og = _og()
    rng = np.random.default_rng(1200)
    n, C = 1500, 6
    X, lab, conf = _lognormal(rng, n).cuda(), _labels(rng, n, C).cuda(), _conf(rng, n).cuda()
    for cap in _caps(monkeypatch):
        a = og.class_traffic(X, lab, C, conf, 0.5)
        b = og.class_traffic(X, lab, C, conf, 0.5)
        assert torch.equal(a, b), cap


@needs_gpu
@pytest.mark.gpu
def test_traffic_captures():
    """One capture, replayed after X, labels, conf and n_live were overwritten
    in place, follows the new contents bit for bit; a live count of 0 leaves
    zeros, not the totals of the replay before."""
    og = _og()
    rng = np.random.default_rng(1300)
    n, C = 1500, 6
    polls = [
        (_lognormal(rng, n).cuda(), _labels(rng, n, C).cuda(), _conf(rng, n).cuda(), live)
        for live in (n, 5, 0, 1000)
    ]
    sX, slab, sconf = (t.clone() for t in polls[0][:3])
    d_live = _live(n, "cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            og.class_traffic(sX, slab, C, sconf, 0.5, d_live)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = og.class_traffic(sX, slab, C, sconf, 0.5, d_live)
    for k, (X, lab, conf, live) in enumerate(polls):
        sX.copy_(X)
        slab.copy_(lab)
        sconf.copy_(conf)
        d_live.fill_(live)
        g.replay()
        torch.cuda.synchronize()
        want = og.class_traffic(X, lab, C, conf, 0.5, _live(live, "cuda"))
        assert torch.equal(out, want), k
        assert float(out[:, 0].sum()) == live, k
        if live == 0:
            assert not bool(out.any())
