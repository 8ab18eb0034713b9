"""Forest explanations on the CPU: the definition on hand-made forests, the
additivity of the contributions on the shipped forest, an independent
computation from sklearn's decision paths, and the model, engine and CLI
layers on top of ops.rf_explain.
"""

import io
import json
import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import ops
from traffic_classifier_sdn_amd.cli import main as cli_main
from traffic_classifier_sdn_amd.flow.parser import PollStreamParser
from traffic_classifier_sdn_amd.flow.replay import TelemetryReplaySource
from traffic_classifier_sdn_amd.models import RandomForestClassifier, load_model
from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.serve import RealtimeClassifier, render_flow_table
from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine
from traffic_classifier_sdn_amd.utils.checkpoint import save_params_npz
from traffic_classifier_sdn_amd.utils.datasets import load_six_class_dataset
from traffic_classifier_sdn_amd.utils.schema import FEATURE_NAMES, FEATURE_SHORT_NAMES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
HALF = 1 << 29  # a step of 0.5 in units of 2^-30


def _leaf(values):
    return {"left": [-1], "right": [-1], "feature": [-2], "threshold": [0.0], "values": [values]}


TREE_A = {"left": [1, -1, -1], "right": [2, -1, -1], "feature": [3, -2, -2],
          "threshold": [1.5, 0.0, 0.0], "values": [[2, 2], [2, 0], [0, 2]]}
TREE_B = _leaf([1, 3])


def _explain(trees, C, x, labels):
    """(contrib, why, why_value, sums) of rows given as {feature: value}."""
    X = torch.zeros(len(x), 12)
    for r, row in enumerate(x):
        for f, v in row.items():
            X[r, f] = v
    return ops.rf_explain(X, oc.rf_flatten(trees, C), oc.rf_explain_flatten(trees, C),
                          torch.tensor(labels, dtype=torch.int32), True, True)


def _shipped():
    return load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device="cpu")


# ----------------------------------------------------------------------
# the definition
# ----------------------------------------------------------------------


def test_hand_forest():
    tables = oc.rf_explain_flatten([TREE_A, TREE_B], 2)
    assert tables["bias"].dtype == torch.float64 and tables["bias"].tolist() == [0.375, 0.625]
    assert tables["delta"].dtype == torch.int32 and tables["max_depth"] == 1
    assert tables["delta"].tolist() == [[0, 0], [HALF, -HALF], [-HALF, HALF], [0, 0]]
    nan = float("nan")
    contrib, why, why_value, sums = _explain(
        [TREE_A, TREE_B], 2, [{3: 1.0}, {3: 2.0}, {3: nan}, {3: nan}, {3: 1.0}, {3: 1.0}],
        [0, 0, 0, 1, -1, 2])
    want = torch.zeros(6, 12, dtype=torch.int64)
    want[:, 3] = torch.tensor([HALF, -HALF, -HALF, HALF, 0, 0])  # a NaN goes right
    assert sums.dtype == torch.int64 and torch.equal(sums, want)
    assert contrib.dtype == torch.float32 and contrib[:, 3].tolist() == [0.25, -0.25, -0.25, 0.25, 0.0, 0.0]
    assert why.dtype == torch.int32 and why.tolist() == [3, -1, -1, 3, -1, -1]
    assert why_value.dtype == torch.float32 and why_value.tolist() == [0.25, 0.0, 0.0, 0.25, 0.0, 0.0]
    assert 0.375 + 0.25 == 0.625  # bias + contributions: the forest's (1 + 0.25) / 2
    # the two optional outputs
    X = torch.zeros(1, 12)
    got = ops.rf_explain(X, oc.rf_flatten([TREE_A], 2), oc.rf_explain_flatten([TREE_A], 2),
                         torch.zeros(1, dtype=torch.int32), want_matrix=False)
    assert got[0] is None and got[3] is None and got[1].tolist() == [3]


def test_chain_and_tie():
    # feature 2 twice, then feature 5: class 0 goes 1/2 -> 3/4 -> 1/2 -> 1
    chain = {"left": [1, 2, 3, -1, -1, -1, -1], "right": [6, 5, 4, -1, -1, -1, -1],
             "feature": [2, 2, 5, -2, -2, -2, -2],
             "threshold": [10.0, 5.0, 1.0, 0.0, 0.0, 0.0, 0.0],
             "values": [[4, 4], [3, 1], [1, 1], [1, 0], [0, 1], [2, 0], [1, 3]]}
    tables = oc.rf_explain_flatten([chain], 2)
    assert tables["max_depth"] == 3 and tables["bias"].tolist() == [0.5, 0.5]
    contrib, why, why_value, sums = _explain([chain], 2, [{2: 4.0, 5: 0.0}, {2: 4.0, 5: 2.0}, {2: 11.0}], [0, 0, 1])
    quarter = HALF // 2
    assert sums[0].tolist()[2] == quarter - quarter and sums[0].tolist()[5] == HALF
    assert sums[1].tolist()[2] == 0 and sums[1].tolist()[5] == -HALF
    assert sums[2].tolist()[2] == quarter  # class 1: 1/2 -> 3/4 at the root's right leaf
    assert why.tolist() == [5, -1, 2] and why_value.tolist() == [0.5, 0.0, 0.25]
    assert contrib[0].sum().item() + 0.5 == 1.0
    # a tie: features 7 and 4 each add 1/4 to class 0; the lower index wins
    def split(f):
        return {"left": [1, -1, -1], "right": [2, -1, -1], "feature": [f, -2, -2],
                "threshold": [0.0, 0.0, 0.0], "values": [[2, 2], [3, 1], [1, 3]]}
    contrib, why, why_value, sums = _explain([split(7), split(4)], 2, [{}, {4: 1.0, 7: 1.0}], [0, 1])
    assert sums[0, 4] == sums[0, 7] == quarter and why.tolist() == [4, 4]
    assert why_value.tolist() == [0.125, 0.125]


def test_flatten_refuses_too_many_path_edges():
    depth = 1 << 10
    n = 2 * depth + 1  # a chain going left
    chain = {"left": np.full(n, -1), "right": np.full(n, -1), "feature": np.full(n, -2),
             "threshold": np.zeros(n), "values": np.ones((n, 2))}
    for i in range(depth):
        chain["left"][i], chain["right"][i], chain["feature"][i] = i + 1, n - 1 - i, 0
    assert oc.rf_explain_flatten([chain] * 4095, 2)["max_depth"] == depth
    with pytest.raises(ValueError, match="2\\^22"):
        oc.rf_explain_flatten([chain] * 4096, 2)
    assert ops.rf_explain_flatten([TREE_A], 2)["max_depth"] == 1  # reachable through ops too


def test_op_checks_its_arguments():
    forest, tables = oc.rf_flatten([TREE_A, TREE_B], 2), oc.rf_explain_flatten([TREE_A, TREE_B], 2)
    X, lab = torch.zeros(3, 12), torch.zeros(3, dtype=torch.int32)
    for bad in (X.double(), torch.zeros(12, 3).t(), torch.zeros(3, 3), X.numpy()):
        with pytest.raises(ValueError):  # dtype, layout, too few columns for feature 3, no tensor
            ops.rf_explain(bad, forest, tables, lab)
    for bad in (lab.long(), lab[:2], None):
        with pytest.raises(ValueError, match="labels"):
            oc.rf_explain(X, forest, tables, bad)
    with pytest.raises(ValueError, match="delta"):
        oc.rf_explain(X, forest, dict(tables, delta=tables["delta"][:-1]), lab)
    with pytest.raises(ValueError, match="2\\^22"):
        oc.rf_explain(X, forest, dict(tables, max_depth=1 << 21), lab)


# ----------------------------------------------------------------------
# additivity on the shipped forest
# ----------------------------------------------------------------------


def _paths_proba(trees, X32, C):
    """f64 [n, C] forest probabilities straight from the trees' values."""
    p = np.zeros((len(X32), C))
    for t in trees:
        thr = np.asarray(t["threshold"], dtype=np.float64).astype(np.float32)
        values = np.asarray(t["values"], dtype=np.float64)
        for r, x in enumerate(X32):
            v = 0
            while t["left"][v] != -1:
                v = t["left"][v] if x[t["feature"][v]] <= thr[v] else t["right"][v]
            p[r] += values[v] / values[v].sum()
    return p / len(trees)


def test_additivity_on_the_shipped_forest():
    rf = _shipped()
    X, _ = load_six_class_dataset()
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32)[::37])
    tables = rf.explain_tables
    T, D, C = len(rf.trees_), tables["max_depth"], len(rf.classes_)
    assert (T, D, C) == (100, 14, 6)
    exact = _paths_proba(rf.trees_, X, C)
    bias = tables["bias"].numpy()
    worst = 0.0
    for c in range(C):
        labels = torch.full((len(X),), c, dtype=torch.int32)
        contrib, _, _, sums = ops.rf_explain(torch.from_numpy(X), rf.forest, tables, labels, True, True)
        total = bias[c] + sums.numpy().astype(np.float64).sum(axis=1) / (2.0 ** 30 * T)
        err = np.abs(total - exact[:, c])
        worst = max(worst, float(err.max()))
        assert bool((err <= D * 2.0 ** -31 + 1e-12).all()), (c, float(err.max()))
        want = (sums.double() / (2.0 ** 30 * T)).float()
        assert torch.equal(contrib.view(torch.int32), want.view(torch.int32))
    print(f"largest |bias + sum S / (2^30 T) - p| = {worst:.3g}, bound {D * 2.0 ** -31 + 1e-12:.3g}")


# ----------------------------------------------------------------------
# an independent oracle: sklearn's decision paths
# ----------------------------------------------------------------------


def test_sums_equal_sklearn_decision_paths():
    sk = pytest.importorskip("sklearn.ensemble")
    rng = np.random.default_rng(0)
    X = rng.integers(0, 50, size=(300, 12)).astype(np.float64)
    y = (X[:, 0] + X[:, 5] > X[:, 9] + 20).astype(int) + (X[:, 3] > 30)
    model = sk.RandomForestClassifier(n_estimators=7, random_state=0).fit(X, y)
    C, T = 3, 7
    assert list(model.classes_) == [0, 1, 2]
    trees = []
    for est in model.estimators_:
        t = est.tree_
        trees.append({"left": t.children_left, "right": t.children_right, "feature": t.feature,
                      "threshold": t.threshold, "values": t.value.reshape(t.node_count, C)})
    tables = oc.rf_explain_flatten(trees, C)
    forest = oc.rf_flatten(trees, C)
    X32 = torch.from_numpy(X.astype(np.float32))
    labels = torch.from_numpy(model.predict(X).astype(np.int32))
    _, _, _, sums = ops.rf_explain(X32, forest, tables, labels, False, True)
    want = np.zeros((len(X), 12), dtype=np.int64)
    proba = np.zeros(len(X))
    for est in model.estimators_:
        t = est.tree_
        p = t.value.reshape(t.node_count, C)
        p = p / p.sum(axis=1, keepdims=True)
        path = est.decision_path(X).tocsr()
        for r in range(len(X)):  # every row
            nodes = path.indices[path.indptr[r]:path.indptr[r + 1]]  # ascending = root to leaf
            c = labels[r].item()
            for v, w in zip(nodes[:-1], nodes[1:]):
                want[r, t.feature[v]] += int(np.rint((p[w, c] - p[v, c]) * 2.0 ** 30))
            proba[r] += p[nodes[-1], c]
    assert np.array_equal(sums.numpy(), want)
    total = tables["bias"].numpy()[labels.numpy()] + want.sum(axis=1) / (2.0 ** 30 * T)
    assert float(np.abs(total - proba / T).max()) <= tables["max_depth"] * 2.0 ** -31 + 1e-12


# ----------------------------------------------------------------------
# model, engine, CLI
# ----------------------------------------------------------------------


def test_model_explain_round_trips_through_a_checkpoint(tmp_path):
    rng = np.random.default_rng(1)
    X = rng.normal(size=(120, 12)).astype(np.float32)
    y = np.where(X[:, 2] + X[:, 8] > 0, "a", "b")
    rf = RandomForestClassifier(n_estimators=5, device="cpu", builder="exact").fit(X, y)
    first = rf.explain_tables
    assert rf.explain_tables is first  # cached
    names, contrib, bias = rf.explain(X)
    assert list(names) == list(rf.predict(X)) and contrib.shape == (120, 12) and bias.dtype == np.float64
    proba = rf.predict_proba(X).numpy().max(axis=1)
    assert float(np.abs(bias + contrib.astype(np.float64).sum(axis=1) - proba).max()) < 1e-6
    path = str(tmp_path / "rf.npz")
    save_params_npz(rf.to_params(), path)
    again = load_model(path, device="cpu")
    for a, b in zip(rf.explain(X), again.explain(X)):
        assert np.array_equal(a, b)
    contrib_dev, why, why_value, sums = again.explain_device(X, want_sums=True)
    assert np.array_equal(contrib_dev.numpy(), contrib) and sums.dtype == torch.int64
    other = again.explain_device(X, np.zeros(120, dtype=np.int64), want_matrix=False)
    assert other[0] is None and other[1].shape == (120,)
    rf.fit(X, np.where(X[:, 0] > 0, "a", "b"))
    assert rf.explain_tables is not first  # dropped on fit


def _replay_table(polls=3):
    src = TelemetryReplaySource(seed=0)
    parser = PollStreamParser()
    for _ in range(polls):
        for line in src.poll():
            parser.feed(line)
    return parser.table


def test_cpu_engine_equals_the_op():
    rf = _shipped()
    table = _replay_table()
    plain = GpuServeEngine({"Randomforest": rf}, capacity=64, device="cpu")
    eng = GpuServeEngine({"Randomforest": rf}, capacity=64, device="cpu", explain="Randomforest")
    full = GpuServeEngine({"Randomforest": rf}, capacity=2, device="cpu", explain="Randomforest",
                          explain_matrix=True)  # past capacity: the unbounded path
    ref, out, out_full = plain.classify(table), eng.classify(table), full.classify(table)
    assert list(out) == list(ref) == list(out_full) == ["Randomforest"]
    assert np.array_equal(out["Randomforest"], ref["Randomforest"])
    for attr in ("why", "why_value", "contributions", "explain_bias", "explain_features"):
        assert getattr(plain, attr) is None, attr
    assert vars(plain).keys() == vars(GpuServeEngine({"Randomforest": rf}, capacity=64, device="cpu")).keys()
    assert not any("exp" in k for k in vars(plain))
    X = torch.from_numpy(np.ascontiguousarray(table.feature_matrix(dtype=np.float32)))
    labels = torch.from_numpy(out["Randomforest"].astype(np.int32))
    contrib, why, why_value, _ = ops.rf_explain(X, rf.forest, rf.explain_tables, labels)
    for e in (eng, full):
        assert e.why.dtype == np.int32 and np.array_equal(e.why, why.numpy())
        assert e.why_value.dtype == np.float32 and np.array_equal(e.why_value, why_value.numpy())
        assert e.explain_features == FEATURE_SHORT_NAMES
        assert e.explain_bias.dtype == np.float64
        assert np.array_equal(e.explain_bias, rf.explain_tables["bias"].numpy())
    assert eng.contributions is None and np.array_equal(full.contributions, contrib.numpy())
    assert bool((eng.why >= 0).all())


def test_engine_refuses_what_it_cannot_explain():
    rf = _shipped()
    nb = load_model(os.path.join(MODELS, "GaussianNB.npz"), device="cpu")
    models = {"Randomforest": rf, "gaussiannb": nb}
    with pytest.raises(ValueError, match="not a key of models"):
        GpuServeEngine(models, device="cpu", explain="forest")
    with pytest.raises(ValueError, match="not a random forest"):
        GpuServeEngine(models, device="cpu", explain="gaussiannb")
    with pytest.raises(ValueError, match="explain_matrix needs explain="):
        GpuServeEngine(models, device="cpu", explain_matrix=True)


def test_render_flow_table_default_is_unchanged():
    table = _replay_table()
    labels = ["dns"] * len(table)
    conf = np.linspace(0.1, 0.9, len(table))
    assert render_flow_table(table, labels) == render_flow_table(table, labels, None, None)
    assert "Why" not in render_flow_table(table, labels, conf)
    cells = ["Rev avg B/s +0.21"] + [""] * (len(table) - 1)
    text = render_flow_table(table, labels, conf, cells)
    assert text.splitlines()[1].split("|")[-2].strip() == "Why" and "Rev avg B/s +0.21" in text
    assert len(FEATURE_SHORT_NAMES) == len(FEATURE_NAMES) == len(set(FEATURE_SHORT_NAMES)) == 12


def test_realtime_classifier_explains_the_class_shown():
    rf = _shipped()
    out, stats = io.StringIO(), io.StringIO()
    # min_confidence 0.7 shows some of the replay flows as unknown
    rc = RealtimeClassifier(rf, out=out, stats=True, stats_out=stats, min_confidence=0.7,
                            smooth=0.5, explain=True)
    rc.run(TelemetryReplaySource(seed=0).stream(30))
    shown = rc.classify_now()
    assert "unknown" in set(shown) and set(shown) - {"unknown"}
    index = {str(c): i for i, c in enumerate(rf.classes_)}
    labels = torch.tensor([index.get(str(s), -1) for s in shown], dtype=torch.int32)
    X = torch.from_numpy(np.ascontiguousarray(rc.parser.table.feature_matrix(dtype=np.float32)))
    _, why, why_value, _ = ops.rf_explain(X, rf.forest, rf.explain_tables, labels)
    assert np.array_equal(rc.last_why, why.numpy()) and np.array_equal(rc.last_why_value, why_value.numpy())
    assert bool((rc.last_why[np.asarray(shown) == "unknown"] == -1).all())
    last_table = out.getvalue().strip().split("\n+")[-6:]
    rows = [l for l in out.getvalue().splitlines() if l.startswith("|") and "unknown" in l]
    assert rows and all(r.split("|")[-2].strip() == "" for r in rows), last_table
    line = json.loads(stats.getvalue().splitlines()[-1])
    assert set(line["why"]) <= set(FEATURE_SHORT_NAMES) and sum(line["why"].values()) <= line["flows"]
    with pytest.raises(ValueError, match="not a random forest"):
        RealtimeClassifier(load_model(os.path.join(MODELS, "GaussianNB.npz"), device="cpu"), explain=True)


def test_cli_explain(capsys):
    argv = ["--source", "replay", "--replay-polls", "8", "--device", "cpu"]
    assert cli_main(["Randomforest", "--explain", "--stats"] + argv) == 0
    got = capsys.readouterr()
    header = [l for l in got.out.splitlines() if "Flow ID" in l]
    assert header and all(h.split("|")[-2].strip() == "Why" for h in header)
    assert any(name in got.out for name in FEATURE_SHORT_NAMES)
    lines = [json.loads(l) for l in got.err.splitlines() if l.startswith("{")]
    assert lines and all("why" in l for l in lines)
    assert sum(lines[-1]["why"].values()) == lines[-1]["flows"]
    # without the flag: the table and the stats line of before
    assert cli_main(["Randomforest", "--stats"] + argv) == 0
    plain = capsys.readouterr()
    assert "Why" not in plain.out and all("why" not in json.loads(l) for l in plain.err.splitlines() if l.startswith("{"))
    assert cli_main(["gaussiannb", "--explain"] + argv) == 2
    refused = capsys.readouterr()
    assert "--explain" in refused.err and "not a random forest" in refused.err and refused.out == ""
