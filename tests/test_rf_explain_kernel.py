"""Forest explanation kernels (csrc/rf_explain_kernels.hip) against the CPU
oracle ops.cpu.rf_explain, in both TCSDN_RF_EXPLAIN_MODE settings.

Every term of a contribution sum is an int32 and at most T * max_depth < 2^22
of them are added, so the int64 sums are exact in any order: ``sums`` must
equal the oracle's bit for bit.  ``contrib`` is one f64 division of such a
sum by 2^30 T rounded once to f32, ``why`` an argmax over the sums and
``why_value`` one of the contributions, so they are compared bit for bit too
(the floats through their int32 views, which tells -0 from +0).
"""

import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd.flow.parser import PollStreamParser
from traffic_classifier_sdn_amd.flow.replay import (
    SynthFlowSpec, TelemetryReplaySource, default_specs,
)
from traffic_classifier_sdn_amd.models import RandomForestClassifier, load_model
from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine
from traffic_classifier_sdn_amd.utils.datasets import load_six_class_dataset

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
MODES = ("wave", "lane")
ROWS = (1, 3, 4, 5, 63, 64, 65, 511, 513, 4099)
TREES = (1, 3, 64, 65, 100, 129)
CLASSES = (2, 6, 8)


def _og():
    from traffic_classifier_sdn_amd.ops import gpu as og

    return og


def _train_rows():
    """120 heavy-tailed rows with ties, like rate features."""
    rng = np.random.default_rng(7)
    X = np.exp(rng.normal(3.0, 2.0, size=(120, 12)))
    X[:, 3] = np.round(X[:, 3])  # repeated values
    X[:40, 5] = 0.0
    return X.astype(np.float32)


def _queries(n, seed=0):
    rng = np.random.default_rng(100 + seed)
    Q = np.exp(rng.normal(3.0, 2.5, size=(n, 12))).astype(np.float32)
    k = min(n, 120)
    Q[:k:2] = _train_rows()[:k:2]  # training rows among them
    if n > 2:
        Q[n // 2, (seed + n) % 12] = np.nan  # a NaN feature goes right
    return torch.from_numpy(Q)


def _labels(n, C, seed=0):
    """Every class, and the two labels just outside: -1 and C."""
    return ((torch.arange(n, dtype=torch.int64) * 7 + seed) % (C + 2) - 1).to(torch.int32)


_fits = {}


def _fit(T, C):
    """(forest, tables) of the first T of 129 trees fitted on the 120 rows
    with C noisy classes, fresh per call: the packed caches live in them."""
    if C not in _fits:
        X = _train_rows()
        rng = np.random.default_rng(C)
        y = (np.log(X[:, 0] + X[:, 7]) * 1.5 + rng.normal(0, 1.0, len(X))).astype(np.int64) % C
        y[:C] = np.arange(C)  # every class is there
        _fits[C] = RandomForestClassifier(n_estimators=129, device="cpu", builder="exact").fit(X, y)
    trees = _fits[C].trees_[:T]
    return oc.rf_flatten(trees, C), oc.rf_explain_flatten(trees, C)


def _bits(t):
    return t.cpu().view(torch.int32)


def _check(monkeypatch, X, forest, tables, labels, combos=((True, True), (False, False))):
    """Both kernels against the oracle on X; returns the oracle's tuple."""
    og = _og()
    want = oc.rf_explain(X, forest, tables, labels, True, True)
    Xd, lab = X.cuda(), labels.cuda()
    for mode in MODES:
        monkeypatch.setenv("TCSDN_RF_EXPLAIN_MODE", mode)
        for want_matrix, want_sums in combos:
            contrib, why, why_value, sums = og.rf_explain(
                Xd, forest, tables, lab, want_matrix, want_sums)
            assert why.dtype == torch.int32 and why_value.dtype == torch.float32
            assert torch.equal(why.cpu(), want[1]), mode
            assert torch.equal(_bits(why_value), _bits(want[2])), mode
            if want_matrix:
                assert contrib.dtype == torch.float32 and tuple(contrib.shape) == (X.shape[0], 12)
                assert torch.equal(_bits(contrib), _bits(want[0])), mode
            else:
                assert contrib is None
            if want_sums:
                assert sums.dtype == torch.int64 and torch.equal(sums.cpu(), want[3]), mode
            else:
                assert sums is None
    return want


# ----------------------------------------------------------------------
# shapes
# ----------------------------------------------------------------------


@pytest.mark.parametrize("T", TREES)
def test_fitted_forest_shapes(monkeypatch, T):
    for C in CLASSES:
        forest, tables = _fit(T, C)
        for n in ROWS:
            combos = ((True, True), (False, False))
            if n == 65:
                combos += ((True, False), (False, True))
            want = _check(monkeypatch, _queries(n, seed=T), forest, tables, _labels(n, C, T), combos)
            outside = (_labels(n, C, T) < 0) | (_labels(n, C, T) >= C)
            assert not bool(want[3][outside].any()) and bool((want[1][outside] == -1).all())
            if n >= 511 and T >= 3:
                assert bool((want[1] >= 0).any()) and bool((want[3] < 0).any())


def test_shipped_forest_on_dataset_rows(monkeypatch):
    rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device="cpu")
    X, _ = load_six_class_dataset()
    X = torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float32)[::9]))
    forest, tables = oc.rf_flatten(rf.trees_, 6), rf.explain_tables
    own = oc.rf_argmax(X, forest).to(torch.int32)
    want = _check(monkeypatch, X, forest, tables, own)
    assert bool((want[1] >= 0).all())  # something speaks for every verdict of the forest
    _check(monkeypatch, X, forest, tables, _labels(X.shape[0], 6))


def test_lane_kernel_loops_over_several_tiles(monkeypatch):
    """A grid capped at 2 blocks of 256 rows walks 4099 rows in 9 rounds, the
    last one partial."""
    monkeypatch.setenv("TCSDN_RF_EXPLAIN_BLOCKS", "2")
    forest, tables = _fit(65, 6)
    _check(monkeypatch, _queries(4099, seed=3), forest, tables, _labels(4099, 6))


def test_hand_made_forest(monkeypatch):
    tree_a = {"left": [1, -1, -1], "right": [2, -1, -1], "feature": [3, -2, -2],
              "threshold": [1.5, 0.0, 0.0], "values": [[2, 2], [2, 0], [0, 2]]}
    tree_b = {"left": [-1], "right": [-1], "feature": [-2], "threshold": [0.0], "values": [[1, 3]]}
    forest, tables = oc.rf_flatten([tree_a, tree_b], 2), oc.rf_explain_flatten([tree_a, tree_b], 2)
    X = torch.zeros(6, 12)
    X[:, 3] = torch.tensor([1.0, 2.0, float("nan"), 1.0, 1.0, 1.5])
    labels = torch.tensor([0, 0, 0, -1, 2, 1], dtype=torch.int32)
    want = _check(monkeypatch, X, forest, tables, labels)
    assert want[3][:, 3].tolist() == [1 << 29, -(1 << 29), -(1 << 29), 0, 0, -(1 << 29)]
    assert want[1].tolist() == [3, -1, -1, -1, -1, -1]
    assert want[2].tolist() == [0.25, 0.0, 0.0, 0.0, 0.0, 0.0]


# ----------------------------------------------------------------------
# graph capture
# ----------------------------------------------------------------------


@pytest.mark.parametrize("mode", MODES)
def test_graph_capture_replays_on_new_inputs(monkeypatch, mode):
    monkeypatch.setenv("TCSDN_RF_EXPLAIN_MODE", mode)
    og = _og()
    forest, tables = _fit(100, 6)
    n = 257
    X = _queries(n, seed=1).cuda()
    labels = _labels(n, 6).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        og.rf_explain(X, forest, tables, labels, True, True)  # packs outside the graph
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = og.rf_explain(X, forest, tables, labels, True, True)
    for seed in (2, 3):
        X.copy_(_queries(n, seed=seed))
        labels.copy_(_labels(n, 6, seed))
        g.replay()
        torch.cuda.synchronize()
        want = oc.rf_explain(X.cpu(), forest, tables, labels.cpu(), True, True)
        assert torch.equal(out[3].cpu(), want[3]) and torch.equal(out[1].cpu(), want[1])
        assert torch.equal(_bits(out[0]), _bits(want[0])) and torch.equal(_bits(out[2]), _bits(want[2]))


# ----------------------------------------------------------------------
# engine
# ----------------------------------------------------------------------

BULK = SynthFlowSpec("00:00:00:00:01:01", "00:00:00:00:01:02", 8000.0, 1400.0, 4000.0, 64.0)


@pytest.mark.parametrize("capacity", (256, 3))  # 3: five flows take the unbounded path
def test_engine_graph_eager_and_cpu_agree(capacity):
    engines = {}
    for key, dev, graph in (("graph", "cuda", True), ("eager", "cuda", False), ("cpu", "cpu", False)):
        rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device=dev)
        engines[key] = GpuServeEngine({"Randomforest": rf}, capacity=capacity, use_graph=graph,
                                      device=dev, explain="Randomforest", explain_matrix=True)
    rf_cpu = engines["cpu"].models["Randomforest"]
    src = TelemetryReplaySource(specs=default_specs() + [BULK], seed=0)
    parser = PollStreamParser()
    for _ in range(2):
        for line in src.poll():
            parser.feed(line)
        table = parser.table
        assert len(table) == 5
        out = {key: eng.classify(table) for key, eng in engines.items()}
        for key in ("eager", "cpu"):
            np.testing.assert_array_equal(out["graph"]["Randomforest"], out[key]["Randomforest"])
            for attr in ("why", "why_value", "contributions"):
                got, ref = getattr(engines["graph"], attr), getattr(engines[key], attr)
                assert got.dtype == ref.dtype and got.shape == ref.shape
                np.testing.assert_array_equal(got.view(np.int32), ref.view(np.int32), err_msg=f"{key} {attr}")
        X = torch.from_numpy(np.ascontiguousarray(table.feature_matrix(dtype=np.float32)))
        labels = torch.from_numpy(out["graph"]["Randomforest"].astype(np.int32))
        want = oc.rf_explain(X, rf_cpu.forest, rf_cpu.explain_tables, labels)
        np.testing.assert_array_equal(engines["graph"].why, want[1].numpy())
        np.testing.assert_array_equal(engines["graph"].contributions.view(np.int32),
                                      want[0].numpy().view(np.int32))
        assert engines["graph"].contributions.shape == (5, 12)
    assert (engines["graph"]._graph is not None) == (capacity >= 5)


# ----------------------------------------------------------------------
# launcher and binding refusals
# ----------------------------------------------------------------------


def _binding_args():
    forest, tables = _fit(3, 6)
    packed = _og().rf_pack(forest, "cuda")
    return dict(X=_queries(8).cuda(), nodes=packed["nodes"], roots=packed["roots"],
                delta=tables["delta"].cuda(), labels=_labels(8, 6).cuda(),
                want_matrix=True, want_sums=True)


def test_launcher_refuses_what_it_has_no_kernel_for():
    ext = _og()._ext.explain
    a = _binding_args()
    ext.rf_explain(*a.values())
    n_nodes = a["nodes"].shape[0]
    nine = dict(a, delta=torch.zeros(n_nodes, 9, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="rf_explain: no kernel for 9 classes"):
        ext.rf_explain(*nine.values())
    one = dict(a, delta=torch.zeros(n_nodes, 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="rf_explain: no kernel for 1 classes"):
        ext.rf_explain(*one.values())
    many = dict(a, roots=torch.zeros(4097, dtype=torch.int32, device="cuda"))  # 4097 times tree 0
    with pytest.raises(RuntimeError, match="4097 trees"):
        ext.rf_explain(*many.values())
    none = dict(a, roots=torch.zeros(0, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="0 trees"):
        ext.rf_explain(*none.values())
    ext.rf_explain(*dict(a, roots=torch.zeros(4096, dtype=torch.int32, device="cuda")).values())
    torch.cuda.synchronize()


def test_binding_refusals():
    ext = _og()._ext.explain
    a = _binding_args()
    other = {torch.float32: torch.float64, torch.int32: torch.int64}
    for name in ("X", "nodes", "roots", "delta", "labels"):
        t = a[name]
        bad = {
            "dtype": t.to(other[t.dtype]),
            "cpu": t.cpu(),
            "strided": torch.stack([t, t], dim=-1)[..., 0],
        }
        for what, v in bad.items():
            with pytest.raises(RuntimeError, match=rf"\b{name}\b"):
                ext.rf_explain(*dict(a, **{name: v}).values())
    shapes = {
        "X": a["X"][:, :11].contiguous(),
        "nodes": a["nodes"].reshape(-1),
        "roots": a["roots"].unsqueeze(0),
        "delta": a["delta"][:-1].contiguous(),  # one row short of the node table
        "labels": a["labels"][:-1].contiguous(),
    }
    for name, v in shapes.items():
        with pytest.raises(RuntimeError, match=rf"\b{name}\b"):
            ext.rf_explain(*dict(a, **{name: v}).values())
    with pytest.raises(RuntimeError, match=r"\bdelta\b"):
        ext.rf_explain(*dict(a, delta=a["delta"].reshape(-1)).values())
    with pytest.raises(RuntimeError, match=r"\blabels\b"):
        ext.rf_explain(*dict(a, labels=a["labels"].unsqueeze(0)).values())
    torch.cuda.synchronize()


def test_op_refusals():
    og = _og()
    forest, tables = _fit(3, 6)
    X, lab = _queries(8).cuda(), _labels(8, 6).cuda()
    og.rf_explain(X, forest, tables, lab)
    for bad in (X.double(), torch.zeros(12, 8, device="cuda").t()):
        with pytest.raises(ValueError, match="f32"):
            og.rf_explain(bad, forest, tables, lab)
    for bad in (lab[:7], lab.long(), lab.cpu()):
        with pytest.raises(ValueError, match="labels"):
            og.rf_explain(X, forest, tables, bad)
    with pytest.raises(ValueError, match="delta"):
        og.rf_explain(X, forest, dict(tables, delta=tables["delta"][:-1]), lab)
    torch.cuda.synchronize()
