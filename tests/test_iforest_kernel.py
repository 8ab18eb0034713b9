"""Isolation forest score kernels (csrc/iforest_kernels.hip) against the CPU
oracle ops.cpu.iforest_score, in both TCSDN_IFOREST_MODE settings.

Every leaf value is 0 or an f32 in [1, 64), a multiple of 2^-23, and at most
4096 of them sum below 2^18: the f64 path-length sum is exact in any order,
so ``psum`` must equal the oracle's bit for bit, and with it the flags and
the masked labels.  The score is the f32 rounding of exp2 of one f64 product
of equal operands; the two exp2 implementations may round differently, which
moves the f32 result by at most one ulp.
"""

import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import ops
from traffic_classifier_sdn_amd.flow.parser import PollStreamParser
from traffic_classifier_sdn_amd.flow.replay import (
    SynthFlowSpec, TelemetryReplaySource, default_specs,
)
from traffic_classifier_sdn_amd.models import IsolationForest, load_model
from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
MODES = ("wave", "lane")
ROWS = (1, 63, 64, 65, 257, 4099)
TREES = (1, 3, 64, 65, 100, 129)


def _og():
    from traffic_classifier_sdn_amd.ops import gpu as og

    return og


def _train_rows():
    """300 heavy-tailed rows with ties, like rate features."""
    rng = np.random.default_rng(7)
    X = np.exp(rng.normal(3.0, 2.0, size=(300, 12)))
    X[:, 3] = np.round(X[:, 3])  # repeated values
    X[:100, 5] = 0.0
    return X.astype(np.float32)


def _queries(n, seed=0):
    rng = np.random.default_rng(100 + seed)
    Q = np.exp(rng.normal(3.0, 2.5, size=(n, 12))).astype(np.float32)
    k = min(n, 300)
    Q[:k:2] = _train_rows()[:k:2]  # training rows among them
    return torch.from_numpy(Q)


_fits = {}


def _fit(T):
    """The flattened forest of T trees fitted on the 300 rows (trees t of any
    T are the same trees), fresh per call: the packed cache lives in it."""
    if 129 not in _fits:
        _fits[129] = IsolationForest(n_estimators=129, max_samples=256, device="cpu").fit(_train_rows())
    m = _fits[129]
    return oc.iforest_flatten(m.trees_[:T], m.max_samples_)


def _chain(depth, feature, thr0):
    """A chain of ``depth`` inner nodes going left, node i testing
    x[feature] <= thr0 - i; every leaf holds one row, so a leaf's h is its
    depth."""
    n = 2 * depth + 1
    left, right, feat = np.full(n, -1), np.full(n, -1), np.full(n, -1)
    thr = np.zeros(n)
    for i in range(depth):
        left[i], right[i], feat[i], thr[i] = i + 1, n - 1 - i, feature, thr0 - i
    return {"left": left, "right": right, "feature": feat, "threshold": thr,
            "n_node_samples": np.ones(n, dtype=np.int64)}


def _hand_forest():
    """A root-only tree of two rows (h = 1) and a depth-8 chain on feature 0
    with thresholds 8, 7, ..., 1; psi = 2, so c(psi) = 1 and T c(psi) = 2."""
    root = {"left": np.array([-1]), "right": np.array([-1]), "feature": np.array([-1]),
            "threshold": np.array([0.0]), "n_node_samples": np.array([2])}
    return oc.iforest_flatten([root, _chain(8, 0, 8.0)], 2)


def _ulp_close(got, want):
    """Within one f32 ulp, sign and zero aside: both are positive scores."""
    g = got.cpu().view(torch.int32).long()
    w = want.cpu().view(torch.int32).long()
    return bool(((g - w).abs() <= 1).all())


def _check(monkeypatch, X, forest, threshold=None, labels=None):
    """Both kernels against the oracle on X; returns the oracle's tuple."""
    og = _og()
    want = oc.iforest_score(X, forest, threshold, labels, want_sum=True)
    Xd = X.cuda()
    lab = None if labels is None else labels.cuda()
    for mode in MODES:
        monkeypatch.setenv("TCSDN_IFOREST_MODE", mode)
        for want_sum in (True, False):
            score, flags, masked, psum = og.iforest_score(Xd, forest, threshold, lab, want_sum)
            assert score.dtype == torch.float32 and flags.dtype == torch.uint8
            assert _ulp_close(score, want[0]), mode
            assert torch.equal(flags.cpu(), want[1]), mode
            if labels is None:
                assert masked is None
            else:
                assert masked.dtype == torch.int32 and torch.equal(masked.cpu(), want[2]), mode
            if want_sum:
                assert psum.dtype == torch.float64 and torch.equal(psum.cpu(), want[3]), mode
            else:
                assert psum is None
    return want


# ----------------------------------------------------------------------
# shapes
# ----------------------------------------------------------------------


@pytest.mark.parametrize("T", TREES)
def test_fitted_forest_shapes(monkeypatch, T):
    forest = _fit(T)
    for n in ROWS:
        X = _queries(n, seed=T)
        labels = (torch.arange(n, dtype=torch.int32) % 6)
        thr = 0.55  # flags some rows of every shape but the smallest
        want = _check(monkeypatch, X, forest, thr, labels)
        if n >= 257:
            assert 0 < int(want[1].sum()) < n


def test_hand_made_forest(monkeypatch):
    forest = _hand_forest()
    # x0 = 10 leaves the chain at depth 1, 7.5 at depth 2, ..., 0.5 at depth 8
    x0 = [10.0, 7.5, 6.5, 5.5, 4.5, 3.5, 2.5, 1.5, 0.5, 8.0, 1.0]
    depth = [1, 2, 3, 4, 5, 6, 7, 8, 8, 2, 8]  # 8 <= 8 goes left, 8 <= 7 does not
    X = torch.zeros(len(x0), 12)
    X[:, 0] = torch.tensor(x0)
    want = _check(monkeypatch, X, forest)
    assert want[3].tolist() == [1.0 + d for d in depth]
    # the same rows many times over: more than one block, partial last one
    for n in ROWS:
        idx = torch.arange(n) % len(x0)
        w = _check(monkeypatch, X[idx].contiguous(), forest)
        assert torch.equal(w[3], want[3][idx])


def test_lane_kernel_loops_over_several_tiles(monkeypatch):
    """A grid capped at 2 blocks of 512 rows walks 4099 rows in 5 rounds, the
    last one partial."""
    monkeypatch.setenv("TCSDN_IFOREST_BLOCKS", "2")
    forest = _fit(65)
    X = _queries(4099, seed=3)
    _check(monkeypatch, X, forest, 0.55, torch.zeros(4099, dtype=torch.int32))


# ----------------------------------------------------------------------
# flags and masked labels
# ----------------------------------------------------------------------


def test_the_cut_is_strict(monkeypatch):
    """psi = 2 and T = 2 make T c(psi) = 2, and threshold 2^-2 gives
    depth_cut = 4 exactly: the psum of a row that leaves the chain at depth
    3.  psum < depth_cut is strict, so that row is not novel; the rows that
    leave earlier are."""
    forest = _hand_forest()
    T, c_psi, _ = oc.iforest_consts(forest)
    assert (T, c_psi) == (2, 1.0) and oc.iforest_depth_cut(0.25, T, c_psi) == 4.0
    X = torch.zeros(5, 12)
    X[:, 0] = torch.tensor([10.0, 7.5, 6.5, 5.5, float("nan")])  # depths 1, 2, 3, 4, 1
    labels = torch.tensor([5, 4, 3, 2, 1], dtype=torch.int32)
    want = _check(monkeypatch, X, forest, 0.25, labels)
    assert want[3].tolist() == [2.0, 3.0, 4.0, 5.0, 2.0]
    assert want[1].tolist() == [1, 1, 0, 0, 1]
    assert want[2].tolist() == [-1, -1, 3, 2, -1]
    exact = torch.tensor([-1.0, -1.5, -2.0, -2.5, -1.0], dtype=torch.float64)
    assert torch.equal(want[0], torch.exp2(exact).float())
    # a threshold just under and just over 2^-2
    under = _check(monkeypatch, X, forest, 0.25 * (1 - 1e-9), labels)
    assert under[1].tolist() == [1, 1, 1, 0, 1]
    over = _check(monkeypatch, X, forest, 0.25 * (1 + 1e-9), labels)
    assert over[1].tolist() == [1, 1, 0, 0, 1]


def test_fitted_forest_cut_at_a_rows_own_sum(monkeypatch):
    """depth_cut is what the host computes; whatever it is, the kernel's flag
    is psum < depth_cut on the exact sums, rows at the cut included."""
    forest = _fit(100)
    X = _queries(257, seed=9)
    psum = oc.iforest_score(X, forest, want_sum=True)[3]
    T, c_psi, inv = oc.iforest_consts(forest)
    for r in (0, 100, 256):
        thr = float(np.exp2(-float(psum[r]) * inv))
        want = _check(monkeypatch, X, forest, thr, torch.full((257,), 2, dtype=torch.int32))
        cut = oc.iforest_depth_cut(thr, T, c_psi)
        assert torch.equal(want[1].bool(), psum < cut)


# ----------------------------------------------------------------------
# edge rows
# ----------------------------------------------------------------------


def test_rows_on_a_threshold_and_non_finite_features(monkeypatch):
    forest = _fit(100)
    thr = forest["threshold"][forest["feature"] >= 0]
    feat = forest["feature"][forest["feature"] >= 0].long()
    base = _queries(64, seed=5)
    rows = [base]
    for k in range(0, 600, 7):  # rows that sit exactly on a node's threshold
        r = base[k % 64].clone()
        r[feat[k]] = thr[k]
        rows.append(r.unsqueeze(0))
    for val in (float("nan"), float("inf"), float("-inf")):
        for j in range(12):
            r = base[j].clone()
            r[j] = val
            rows.append(r.unsqueeze(0))
        rows.append(torch.full((1, 12), val))
    X = torch.cat(rows).contiguous()
    want = _check(monkeypatch, X, forest, 0.55, torch.ones(X.shape[0], dtype=torch.int32))
    assert bool(torch.isfinite(want[0]).all())
    # NaN goes right: the hand-made chain leaves a NaN at depth 1, like +inf
    hand = _hand_forest()
    Y = torch.zeros(3, 12)
    Y[:, 0] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    assert _check(monkeypatch, Y, hand)[3].tolist() == [2.0, 2.0, 9.0]


# ----------------------------------------------------------------------
# graph capture
# ----------------------------------------------------------------------


@pytest.mark.parametrize("mode", MODES)
def test_graph_capture_replays_on_new_inputs(monkeypatch, mode):
    monkeypatch.setenv("TCSDN_IFOREST_MODE", mode)
    og = _og()
    forest = _fit(100)
    n = 257
    X = _queries(n, seed=1).cuda()
    labels = (torch.arange(n, dtype=torch.int32) % 6).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        og.iforest_score(X, forest, 0.55, labels, True)  # packs outside the graph
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = og.iforest_score(X, forest, 0.55, labels, True)
    for seed in (2, 3):
        X.copy_(_queries(n, seed=seed))
        labels.copy_((torch.arange(n, dtype=torch.int32) + seed) % 6)
        g.replay()
        torch.cuda.synchronize()
        eager = og.iforest_score(X, forest, 0.55, labels, True)
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
        want = oc.iforest_score(X.cpu(), forest, 0.55, labels.cpu(), True)
        assert torch.equal(out[3].cpu(), want[3]) and torch.equal(out[2].cpu(), want[2])


# ----------------------------------------------------------------------
# engine
# ----------------------------------------------------------------------

BULK = SynthFlowSpec("00:00:00:00:01:01", "00:00:00:00:01:02", 8000.0, 1400.0, 4000.0, 64.0)


def test_engine_graph_matches_the_cpu_engine():
    det = IsolationForest(n_estimators=100, device="cpu").fit(_train_rows())
    params = det.to_params()
    engines = {}
    for dev in ("cuda", "cpu"):
        rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device=dev)
        kw = dict(capacity=256, use_graph=dev == "cuda", device=dev)
        engines[dev] = (
            GpuServeEngine({"Randomforest": rf}, traffic="Randomforest",
                           novelty=IsolationForest.from_params(params, device=dev), **kw),
            GpuServeEngine({"Randomforest": rf}, **kw),
        )
    src = TelemetryReplaySource(specs=default_specs() + [BULK], seed=0)
    parser = PollStreamParser()
    flagged = 0
    for _ in range(3):
        for line in src.poll():
            parser.feed(line)
        table = parser.table
        assert len(table) == 5
        (gpu, gpu_plain), (cpu, _) = engines["cuda"], engines["cpu"]
        out, ref, out_cpu = gpu.classify(table), gpu_plain.classify(table), cpu.classify(table)
        assert list(out) == list(ref)
        np.testing.assert_array_equal(out["Randomforest"], ref["Randomforest"])
        np.testing.assert_array_equal(gpu.novel, cpu.novel)
        assert _ulp_close(torch.from_numpy(gpu.novelty_score), torch.from_numpy(cpu.novelty_score))
        if np.array_equal(out["Randomforest"], out_cpu["Randomforest"]):
            np.testing.assert_array_equal(gpu.traffic, cpu.traffic)
        masked = np.where(gpu.novel, -1, out["Randomforest"]).astype(np.int32)
        X = torch.from_numpy(np.ascontiguousarray(table.feature_matrix(dtype=np.float32)))
        np.testing.assert_array_equal(
            gpu.traffic, oc.class_traffic(X, torch.from_numpy(masked), 6).numpy())
        flagged += int(gpu.novel.sum())
    assert gpu._graph is not None
    assert flagged > 0  # the flows are nothing like the 300 fitted rows


# ----------------------------------------------------------------------
# binding refusals
# ----------------------------------------------------------------------


def test_binding_refusals():
    og = _og()
    forest = _fit(3)
    X = _queries(8).cuda()
    lab = torch.zeros(8, dtype=torch.int32, device="cuda")
    og.iforest_score(X, forest, 0.5, lab)
    bad_inputs = {
        "dtype": X.double(),
        "width": torch.zeros(8, 11, device="cuda"),
        "non-contiguous": torch.zeros(12, 8, device="cuda").t(),
        "cpu tensor": X.cpu(),
    }
    for what, bad in bad_inputs.items():
        with pytest.raises(ValueError):
            og.iforest_score(bad, forest, 0.5)
        if bad.is_cuda:  # the dispatching op takes the same path
            with pytest.raises(ValueError):
                ops.iforest_score(bad, forest, 0.5)
    for bad in (lab[:7], lab.long(), lab.cpu()):
        with pytest.raises(ValueError, match="labels"):
            og.iforest_score(X, forest, 0.5, bad)
    for bad in (0.0, 1.0, 0, 1):
        with pytest.raises(ValueError, match="threshold"):
            og.iforest_score(X, forest, bad)
    torch.cuda.synchronize()
