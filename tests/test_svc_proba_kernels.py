"""SVC decision and coupling kernels (csrc/svc_kernels.hip) against the CPU
oracles in ops/cpu.py, then a calibrated SVC on the GPU and in a captured
serve graph.

Tolerance of a decision value, per pair: atol = Sd * 2^-16, where Sd is the
sum of |dual| over that pair's support vectors.

The oracle is the f64 decision function of the same f32 rows, support
vectors and duals and the f32-rounded gamma.  The kernels differ from it in
three places, each bounded relative to Sd because a kernel value is <= 1:

  * the kernel value.  Its argument a = -gamma * d2 carries 15 f32 roundings
    (12 fused steps of the distance, the subtraction feeding each, the
    product with gamma), a relative 15 * 2^-24, and exp turns an absolute
    error e of its argument into a relative e of its value: |a| * e^-|a| *
    15 * 2^-24 <= (1/e) * 15 * 2^-24 < 2^-21.  A hardware exp good to one
    ulp adds 2^-24.  Allowing a value 2^-18 absolute, eight times that,
    makes the bound independent of the exact accuracy of __expf; that is
    2^-18 * Sd on the decision.
  * the tiled kernel's per-tile f32 chain: up to 128 fused multiply-adds,
    each rounding a partial sum that is at most the tile's share of Sd:
    128 * 2^-24 * Sd = 2^-17 * Sd over all tiles together.  (The wave kernel
    rounds each product once instead, 2^-24 * Sd.)
  * the f64 folds, the wave reduction and the intercept: a few 2^-53 * Sd.

2^-17 + 2^-18 < 2^-16.  Sd is computed from the inputs of every case.

The coupling kernel works in f64 from the same f64 decisions as its oracle,
in the same order; device exp() may differ from the host's in its last bit,
which moves a probability by about 1e-16.  Both sides are then compared
after the kernel's f32 store, half an ulp of a value <= 1 each: atol 2^-22
covers both, and C such roundings keep a row sum within 2^-21 of 1.  The
iteration stops on a threshold, and one sweep more or less moves a
probability by up to 1e-3; every case checks, on the oracle, that no row
comes within 1e-9 of that threshold at any sweep, so kernel and oracle make
the same number of sweeps on every row.
"""

import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd.ops import cpu as oc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

ROWS = (1, 255, 256, 257, 1500)  # 256 rows per block: partial, full, second block
CLASSES = (2, 3, 4, 5, 6)
# support vectors in all: below one wave, around the tile of 128, two tiles
# and a partial one; 2 is one per class and only exists for two classes
TOTALS = (2, 40, 127, 128, 129, 300)
GAMMA = float(np.float32(0.05))
WAVE, TILED = "1", "2"  # TCSDN_SVC_DEC_MODE


def _og():
    from traffic_classifier_sdn_amd.ops import gpu as og

    return og


def _n_support(C, total):
    """Class 0 holds a single SV; the others share the rest, the remainder
    going to the last."""
    if total == C:
        return [1] * C
    rest = total - 1
    ns = [1] + [rest // (C - 1)] * (C - 1)
    ns[-1] += rest - sum(ns[1:])
    assert sum(ns) == total and min(ns) >= 1
    return ns


def _svc_params(C, total, seed):
    rng = np.random.default_rng(seed)
    SV = torch.from_numpy(rng.normal(size=(total, 12)).astype(np.float32))
    dual = torch.from_numpy(rng.uniform(-1, 1, size=(C - 1, total)).astype(np.float32))
    b = torch.from_numpy(rng.normal(size=C * (C - 1) // 2).astype(np.float32))
    return SV, dual, b, torch.tensor(_n_support(C, total), dtype=torch.int64)


def _rows(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).normal(size=(n, 12)).astype(np.float32))


def _pair_sd(dual, n_support):
    """Sd per pair: sum |dual| over the pair's SVs, in f64."""
    C = n_support.numel()
    start = [0] + torch.cumsum(n_support, 0).tolist()
    d = dual.double().abs()
    out = []
    for i in range(C):
        for j in range(i + 1, C):
            out.append(float(d[j - 1, start[i]:start[i + 1]].sum() + d[i, start[j]:start[j + 1]].sum()))
    return torch.tensor(out, dtype=torch.float64)


def _oracle_dec(X, SV, dual, b, n_support):
    K = oc.rbf_kernel(X.double(), SV.double(), GAMMA)
    return oc.svc_ovo_decision(K, dual.double(), b.double(), n_support)


# ----------------------------------------------------------------------
# decision kernels
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [WAVE, TILED])
@pytest.mark.parametrize("C", CLASSES)
def test_svc_decision_kernels(monkeypatch, C, mode):
    og = _og()
    monkeypatch.setenv("TCSDN_SVC_DEC_MODE", mode)
    npair = C * (C - 1) // 2
    for total in TOTALS:
        if total < C or (total == 2 and C != 2):
            continue
        SV, dual, b, ns = _svc_params(C, total, seed=100 * C + total)
        sd = _pair_sd(dual, ns)
        m = torch.tensor([int(ns[i] + ns[j]) for i in range(C) for j in range(i + 1, C)])
        assert sd.shape == (npair,) and bool((sd > 0).all()) and bool((sd <= m).all())
        atol = sd * 2.0 ** -16
        dev = [t.cuda() for t in (SV, dual, b, ns)]
        for n in ROWS:
            X = _rows(n, seed=n + total)
            ref = _oracle_dec(X, SV, dual, b, ns)
            got = og.svc_decision(X.cuda(), *dev, GAMMA)
            assert got.dtype == torch.float64 and got.shape == (n, npair)
            err = (got.cpu() - ref).abs().max(dim=0).values
            tag = f"C={C} mode={mode} nsv={total} n={n}"
            print(f"{tag}: max err / Sd {float((err / sd).max()):.3e} (bound {2.0 ** -16:.3e})")
            assert bool((err <= atol).all()), tag
            # the label kernel follows the forced mode too and accumulates
            # as the decision kernel does: the same votes, row for row
            labels = og.svc_predict(X.cuda(), *dev, GAMMA)
            assert torch.equal(oc.svc_vote(got, C), labels), tag


@needs_gpu
@pytest.mark.gpu
def test_svc_tiled_row_loop(monkeypatch):
    """TCSDN_PROBA_BLOCKS=2 leaves the tiled kernels two blocks for the six
    row tiles of 1500 rows: each block loops three times and the second ends
    on the partial tile.  Same decisions as the uncapped launch, bit for
    bit, within the oracle's bound, and the labels are their votes."""
    og = _og()
    monkeypatch.setenv("TCSDN_SVC_DEC_MODE", TILED)
    monkeypatch.delenv("TCSDN_PROBA_BLOCKS", raising=False)
    C, total, n = 6, 129, 1500
    SV, dual, b, ns = _svc_params(C, total, seed=77)
    dev = [t.cuda() for t in (SV, dual, b, ns)]
    X = _rows(n, seed=78)
    ref = _oracle_dec(X, SV, dual, b, ns)
    uncapped = og.svc_decision(X.cuda(), *dev, GAMMA)
    monkeypatch.setenv("TCSDN_PROBA_BLOCKS", "2")
    got = og.svc_decision(X.cuda(), *dev, GAMMA)
    labels = og.svc_predict(X.cuda(), *dev, GAMMA)
    sd = _pair_sd(dual, ns)
    err = (got.cpu() - ref).abs().max(dim=0).values
    print(f"max err / Sd {float((err / sd).max()):.3e} (bound {2.0 ** -16:.3e})")
    assert bool((err <= sd * 2.0 ** -16).all())
    assert torch.equal(got, uncapped)
    assert torch.equal(oc.svc_vote(got, C), labels)


@needs_gpu
@pytest.mark.gpu
def test_svc_decision_votes_across_the_cutover(monkeypatch):
    """131072 rows run the wave kernels and 131073 the tiled ones, in
    launch_svc_decision as in launch_svc_predict: on either side the vote
    of the decisions is the label kernel's, exactly, and a forced variant
    gives the rows it shares bit for bit."""
    og = _og()
    monkeypatch.delenv("TCSDN_SVC_DEC_MODE", raising=False)
    C, total, n = 6, 300, 131073
    SV, dual, b, ns = _svc_params(C, total, seed=9)
    dev = [t.cuda() for t in (SV, dual, b, ns)]
    X = _rows(n, seed=10).cuda()
    for rows, mode in ((n - 1, WAVE), (n, TILED)):
        dec = og.svc_decision(X[:rows], *dev, GAMMA)
        labels = og.svc_predict(X[:rows], *dev, GAMMA)
        assert torch.equal(oc.svc_vote(dec, C), labels), rows
        monkeypatch.setenv("TCSDN_SVC_DEC_MODE", mode)
        assert torch.equal(og.svc_decision(X[:1500], *dev, GAMMA), dec[:1500]), rows
        monkeypatch.delenv("TCSDN_SVC_DEC_MODE")
    ref = _oracle_dec(X[-257:].cpu(), SV, dual, b, ns)  # the last, partial tile
    err = (dec[-257:].cpu() - ref).abs().max(dim=0).values
    assert bool((err <= _pair_sd(dual, ns) * 2.0 ** -16).all())


@needs_gpu
@pytest.mark.gpu
def test_svc_decision_rejects_bad_extents():
    """The kernels index by nsv and C alone; the binding checks the rest."""
    from traffic_classifier_sdn_amd.ops import _tcsdn_hip as ext

    SV, dual, b, ns = _svc_params(3, 40, seed=1)
    cls = torch.repeat_interleave(torch.arange(3), ns).to(torch.uint8).cuda()
    X = _rows(4, 0).cuda()
    with pytest.raises(RuntimeError, match="dual"):
        ext.svc_decision(X, SV.cuda(), dual[:, :39].contiguous().cuda(), cls, b.cuda(), GAMMA)
    with pytest.raises(RuntimeError, match="svclass"):
        ext.svc_decision(X, SV.cuda(), dual.cuda(), cls[:39].contiguous(), b.cuda(), GAMMA)
    with pytest.raises(RuntimeError, match="intercept"):
        ext.svc_decision(X, SV.cuda(), dual.cuda(), cls, b[:2].contiguous().cuda(), GAMMA)
    with pytest.raises(RuntimeError, match="2..6 classes"):
        ext.svc_couple(torch.zeros(4, 21, dtype=torch.float64).cuda(),
                       torch.zeros(21, dtype=torch.float64).cuda(),
                       torch.zeros(21, dtype=torch.float64).cuda(), 7)


# ----------------------------------------------------------------------
# coupling kernel
# ----------------------------------------------------------------------


def _couple_inputs(C, n, seed):
    rng = np.random.default_rng(seed)
    npair = C * (C - 1) // 2
    dec = rng.normal(size=(n, npair)) * 2
    k = min(n, 8)  # a few saturated rows: the clamp at 1e-7, on either side
    dec[:k] = np.where(rng.random(size=(k, npair)) < 0.5, -50.0, 50.0)
    A = rng.uniform(-12, -3, size=npair)
    B = rng.uniform(-2, 2, size=npair)
    return torch.from_numpy(dec), torch.from_numpy(A), torch.from_numpy(B)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
def test_svc_couple_kernel(monkeypatch, C):
    og = _og()
    for n in ROWS:
        dec, A, B = _couple_inputs(C, n, seed=1000 * C + n)
        ref, ref_idx, _, margin = oc.svc_couple(dec, A, B, C, with_margin=True)
        # every row keeps clear of the stopping threshold at every sweep, so
        # both sides stop at the same sweep (no row is left out)
        assert float(margin.min()) >= 1e-9, (C, n)
        for cap in (None, 2):
            if cap is None:
                monkeypatch.delenv("TCSDN_PROBA_BLOCKS", raising=False)
            else:
                monkeypatch.setenv("TCSDN_PROBA_BLOCKS", str(cap))
            proba, idx, conf = og.svc_couple(dec.cuda(), A.cuda(), B.cuda(), C)
            tag = f"C={C} n={n} cap={cap}"
            assert proba.dtype == torch.float32 and proba.shape == (n, C), tag
            assert idx.dtype == torch.int32 and conf.dtype == torch.float32, tag
            proba, idx, conf = proba.cpu(), idx.cpu(), conf.cpu()
            err = float((proba.double() - ref).abs().max())
            row_err = float((proba.double().sum(dim=1) - 1.0).abs().max())
            print(f"{tag}: max err {err:.3e} (atol {2.0 ** -22:.3e}), row-sum err {row_err:.3e}")
            assert err <= 2.0 ** -22, tag
            assert row_err <= 2.0 ** -21, tag
            assert torch.equal(idx, ref_idx), tag
            assert torch.equal(conf, proba[torch.arange(n), idx.long()]), tag
    # the clamp was reached: a saturated pair gives exactly 1e-7 or 1 - 1e-7
    s = torch.sigmoid(-(dec[:1] * A + B))
    assert bool(((s < 1e-7) | (s > 1 - 1e-7)).all())


# ----------------------------------------------------------------------
# model and serve engine
# ----------------------------------------------------------------------


@pytest.fixture(scope="module")
def gpu_models():
    from traffic_classifier_sdn_amd.models import load_model
    from traffic_classifier_sdn_amd.utils.datasets import load_six_class_dataset

    X, y = load_six_class_dataset()
    perm = np.random.RandomState(0).permutation(len(X))
    rows = perm[2100:5100]
    svc = load_model(os.path.join(MODELS, "SVC.npz"), device="cuda")
    rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device="cuda")
    return rf, svc, svc.calibrate(X[rows], y[rows]), X[perm[5100:5900]]


@needs_gpu
@pytest.mark.gpu
def test_calibrated_svc_on_gpu(gpu_models):
    from traffic_classifier_sdn_amd.models import CalibratedSVC

    og = _og()
    _, svc, cal, Xe = gpu_models
    assert isinstance(cal, CalibratedSVC) and cal.probA_.is_cuda
    X = torch.from_numpy(Xe.astype(np.float32)).cuda()
    proba, idx, conf = cal.predict_scores(X)
    dec = og.svc_decision(X, cal.support_vectors_, cal.dual_coef_, cal.intercept_,
                          cal.n_support_, cal.gamma_)
    assert torch.equal(dec, cal.decision_function(X))
    p2, i2, c2 = og.svc_couple(dec, cal.probA_, cal.probB_, 6)
    assert torch.equal(proba, p2) and torch.equal(idx, i2) and torch.equal(conf, c2)
    assert torch.equal(idx, cal.predict_index(X)) and torch.equal(idx, svc.predict_index(X))
    assert torch.equal(cal.predict_proba_device(X), proba)
    labels, c = cal.predict_with_confidence(X)
    assert np.array_equal(labels, svc.predict(X)) and np.array_equal(c, conf.cpu().numpy())


def _table64(seed):
    """A flow table of 64 flows with rates spread over the classes' ranges."""
    from traffic_classifier_sdn_amd.flow.parser import replay
    from traffic_classifier_sdn_amd.flow.replay import SynthFlowSpec, TelemetryReplaySource

    rng = np.random.default_rng(seed)
    specs = [
        SynthFlowSpec(f"02:00:00:00:00:{i:02x}", f"06:00:00:00:00:{i:02x}",
                      float(rng.uniform(1, 80)), float(rng.uniform(60, 1000)),
                      float(rng.uniform(1, 80)), float(rng.uniform(60, 1000)))
        for i in range(64)
    ]
    return replay(TelemetryReplaySource(specs=specs, seed=seed).stream(6))


@needs_gpu
@pytest.mark.gpu
def test_engine_graph_with_calibrated_svc(gpu_models):
    from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine

    rf, svc, cal, _ = gpu_models
    models = {"rf": rf, "svc": cal}
    kw = dict(capacity=64, confidence=True, ensemble=["rf", "svc"])
    graph = GpuServeEngine(models, use_graph=True, **kw)
    eager = GpuServeEngine(models, use_graph=False, **kw)
    plain = GpuServeEngine({"rf": rf, "svc": svc}, capacity=64, use_graph=True)
    for seed in (7, 11):  # the second call replays the captured graph
        table = _table64(seed)
        assert len(table) == 64
        out, ref, lab = graph.classify(table), eager.classify(table), plain.classify(table)
        assert list(graph.confidence) == ["rf", "svc", "ensemble"]
        for name in ("rf", "svc", "ensemble"):
            np.testing.assert_array_equal(out[name], ref[name])
            np.testing.assert_array_equal(graph.confidence[name], eager.confidence[name])
        # asking for confidence changed no label
        np.testing.assert_array_equal(out["svc"], lab["svc"])
        np.testing.assert_array_equal(out["rf"], lab["rf"])
        conf = graph.confidence["svc"]
        assert conf.dtype == np.float32 and float(conf.min()) > 0.0 and float(conf.max()) <= 1.0
    assert graph._graph is not None
