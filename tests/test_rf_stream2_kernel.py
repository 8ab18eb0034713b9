"""Streaming forest-predict kernel with two rows per lane (TCSDN_RF_MODE=6)
against the CPU oracle ops.cpu.rf_argmax, label for label: the row counts
around one lane set, both lane sets of a wave and one block's 2048 slots,
the pass thresholds, the synthetic forests of test_rf_stream_kernel.py, and
the fall-back to modes 5 and 4 for tables too big for two sets of feature
rows.  (The row-per-lane kernel, mode 2, kept its LDS layout, so it has no
case here.)

Synthetic forests use leaf distributions in eighths, so every score the
oracle and the kernel form is an exact f32 value whatever the summation
order, and ties fall to the first maximum on both sides: equality is exact,
not approximate.
"""

import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd.ops import cpu as oc

og = pytest.importorskip("traffic_classifier_sdn_amd.ops.gpu")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RF_CKPT = os.path.join(REPO, "data", "ref_models", "RandomForestClassifier.npz")

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# nodes (without the two sentinels) up to which the table and two, or one,
# sets of 1024 13-slot feature rows fit in 160 KiB of LDS
TWO_ROWS_MAX_NODES = (160 * 1024 - 2 * 13 * 1024 * 4) // 8 - 2
ONE_ROW_MAX_NODES = (160 * 1024 - 13 * 1024 * 4) // 8 - 2


# ----------------------------------------------------------------------
# forest builders (trees_-style dicts, depth-first layout)
# ----------------------------------------------------------------------


def _pure(rng, C):
    v = np.zeros(C)
    v[rng.integers(C)] = 5.0
    return v


def _mixed(rng, C):
    """Counts summing to 8 over at least two classes: probabilities k/8."""
    v = np.zeros(C)
    a, b = rng.choice(C, size=2, replace=False)
    k = int(rng.integers(1, 8))
    v[a] += k
    v[b] += 8 - k
    return v


def _tree(rng, C, max_depth, leaf, p_split=0.8, min_depth=0):
    left, right, feature, threshold, values = [], [], [], [], []

    def grow(d):
        i = len(left)
        for a in (left, right, feature, threshold):
            a.append(-1)
        values.append(np.ones(C))
        if d < max_depth and (d < min_depth or rng.random() < p_split):
            feature[i] = int(rng.integers(12))
            threshold[i] = float(np.float32(rng.normal()))
            left[i] = len(left)
            grow(d + 1)
            right[i] = len(left)
            grow(d + 1)
        else:
            feature[i] = -2
            threshold[i] = -2.0
            values[i] = leaf(rng, C)

    grow(0)
    return {
        "left": np.asarray(left),
        "right": np.asarray(right),
        "feature": np.asarray(feature),
        "threshold": np.asarray(threshold),
        "values": np.stack(values),
    }


def _leaf_tree(rng, C, leaf):
    return _tree(rng, C, 0, leaf)


def _chain(rng, C, depth, leaf):
    """Every inner node's left child is a leaf and its right child the next
    inner node: rows that keep going right walk `depth` nodes, rows that go
    left at the root walk one."""
    n = 2 * depth + 1
    left = np.full(n, -1)
    right = np.full(n, -1)
    feature = np.full(n, -2)
    threshold = np.full(n, -2.0)
    values = np.ones((n, C))
    for d in range(depth):
        i = 2 * d
        feature[i] = int(rng.integers(12))
        threshold[i] = float(np.float32(rng.normal(-0.5, 0.5)))
        left[i] = i + 1
        right[i] = i + 2
        values[i + 1] = leaf(rng, C)
    values[n - 1] = leaf(rng, C)
    return {"left": left, "right": right, "feature": feature,
            "threshold": threshold, "values": values}


def _rows(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).normal(size=(n, 12)).astype(np.float32))


def _check(monkeypatch, forest, X, ref=None, mode="6", **env):
    """Labels of the kernel that TCSDN_RF_MODE=`mode` runs equal the
    oracle's, row for row."""
    for k in ("TCSDN_RF_STREAM_RANGE", "TCSDN_RF_STREAM_REFILL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    monkeypatch.setenv("TCSDN_RF_MODE", mode)
    if ref is None:
        ref = oc.rf_argmax(X, forest)
    got = og.rf_argmax(X.cuda(), dict(forest)).cpu()
    assert got.dtype == torch.int32 and got.shape == ref.shape
    assert torch.equal(got, ref), f"mode {mode}"


# ----------------------------------------------------------------------
# shipped forest: refill machinery over both slots of a lane
# ----------------------------------------------------------------------


@pytest.fixture(scope="module")
def shipped():
    """(forest, 20 000 benchmark-style rows, their oracle labels)."""
    from traffic_classifier_sdn_amd.models import load_model
    from traffic_classifier_sdn_amd.utils.datasets import load_reference_dataset, synthetic_flow_rows

    forest = load_model(RF_CKPT, device="cpu").forest
    X_real, _ = load_reference_dataset()
    X = torch.from_numpy(synthetic_flow_rows(20_000, seed=1, reference_X=X_real))
    return forest, X, oc.rf_argmax(X, forest)


def test_shipped_forest_fits_two_row_sets(shipped):
    """Else the cases below would run as mode 5."""
    assert shipped[0]["feature"].numel() <= TWO_ROWS_MAX_NODES


# rows per wave: the launcher's own choice (128 at these sizes: one refill of
# both slots, a cursor that runs dry inside slot 0 or slot 1), 129 (one row
# left for a second refill) and one range for everything (a single wave
# refills until one slot is left)
@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("rows_per_wave", [None, 129, 1 << 20])
@pytest.mark.parametrize(
    "n", [1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 2 * 2048 + 7, 20_000])
def test_row_counts(monkeypatch, shipped, n, rows_per_wave):
    forest, X, ref = shipped
    env = {} if rows_per_wave is None else {"TCSDN_RF_STREAM_RANGE": rows_per_wave}
    _check(monkeypatch, forest, X[:n], ref[:n], **env)


# a pass as soon as one slot waits, when half do, and only when all do
@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("refill", [1, 64, 128])
def test_pass_thresholds(monkeypatch, shipped, refill):
    forest, X, ref = shipped
    _check(monkeypatch, forest, X[:5000], ref[:5000],
           TCSDN_RF_STREAM_RANGE=700, TCSDN_RF_STREAM_REFILL=refill)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("copies", [37, 38, 74, 75])
def test_default_thresholds(monkeypatch, shipped, copies):
    """Nothing forced, through the public predict_index, either side of the
    row counts at which the launcher moves from the row-per-lane kernel to
    the streaming one (750 000) and on to two rows per lane (1 500 000).
    Rows are independent, so copies of the 20 000 rows have copies of their
    labels."""
    from traffic_classifier_sdn_amd.models import load_model

    for k in ("TCSDN_RF_MODE", "TCSDN_RF_STREAM_RANGE", "TCSDN_RF_STREAM_REFILL"):
        monkeypatch.delenv(k, raising=False)
    _, X, ref = shipped
    model = load_model(RF_CKPT, device="cuda")
    got = model.predict_index(X.cuda().repeat(copies, 1)).cpu()
    assert torch.equal(got, ref.repeat(copies))


# ----------------------------------------------------------------------
# synthetic forests
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 13, 24])
def test_no_early_exit(monkeypatch, T):
    """Uniformly random pure leaf classes: no row is decided early, every
    slot runs to the last tree (T = 13 is no multiple of the 8-tree test
    interval)."""
    rng = np.random.default_rng(100 + T)
    forest = oc.rf_flatten([_tree(rng, 6, 6, _pure, min_depth=2) for _ in range(T)], 6)
    _check(monkeypatch, forest, _rows(3000, 7), TCSDN_RF_STREAM_RANGE=500)


@needs_gpu
@pytest.mark.gpu
def test_single_node_trees(monkeypatch):
    """Trees whose root is a leaf, at the first, a middle and the last
    position."""
    rng = np.random.default_rng(11)
    trees = [_tree(rng, 6, 5, _pure, min_depth=1) for _ in range(9)]
    for pos, leaf in ((0, _pure), (4, _mixed), (8, _pure)):
        trees[pos] = _leaf_tree(rng, 6, leaf)
    _check(monkeypatch, oc.rf_flatten(trees, 6), _rows(2000, 8), TCSDN_RF_STREAM_RANGE=300)


@needs_gpu
@pytest.mark.gpu
def test_all_mixed_leaves(monkeypatch):
    rng = np.random.default_rng(12)
    forest = oc.rf_flatten([_tree(rng, 6, 6, _mixed, min_depth=1) for _ in range(20)], 6)
    assert float(forest["leaf_proba"].max()) < 1.0
    _check(monkeypatch, forest, _rows(2000, 9), TCSDN_RF_STREAM_RANGE=300)


@needs_gpu
@pytest.mark.gpu
def test_chain_next_to_stumps(monkeypatch):
    """A depth-14 chain between stumps: the longest and the shortest paths
    side by side in one wave, and in the two slots of one lane."""
    rng = np.random.default_rng(13)
    trees = []
    for i in range(12):
        trees.append(_chain(rng, 6, 14, _pure) if i % 3 == 1 else _tree(rng, 6, 1, _pure, min_depth=1))
    _check(monkeypatch, oc.rf_flatten(trees, 6), _rows(3000, 10), TCSDN_RF_STREAM_RANGE=400)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C,T", [(2, 40), (8, 120)])
def test_class_counts(monkeypatch, C, T):
    """Pure leaves of every class, and enough trees that single classes
    collect more than 15 votes; with C = 8 a 10-bit field per class would
    not fit one 64-bit register."""
    rng = np.random.default_rng(20 + C)
    forest = oc.rf_flatten([_tree(rng, C, 4, _pure, min_depth=2) for _ in range(T)], C)
    assert set(forest["leaf_proba"].argmax(dim=1).tolist()) == set(range(C))
    X = _rows(3000, 11)
    proba = oc.rf_predict_proba(X, forest)
    assert float(proba.max()) * T > 15
    ref = torch.argmax(proba, dim=1).to(torch.int32)
    _check(monkeypatch, forest, X, ref, TCSDN_RF_STREAM_RANGE=400)


@needs_gpu
@pytest.mark.gpu
def test_special_values(monkeypatch):
    """NaN compares false and goes right, -inf goes left, +inf goes right
    unless the threshold is +inf too, and a value equal to its threshold
    goes left — the oracle's routing."""
    rng = np.random.default_rng(14)
    trees = [_tree(rng, 6, 6, _pure, min_depth=3) for _ in range(16)]
    trees += [_tree(rng, 6, 4, _mixed, min_depth=2) for _ in range(4)]
    forest = oc.rf_flatten(trees, 6)
    X = _rows(4000, 12)
    inner = forest["feature"] >= 0
    thr, feat = forest["threshold"][inner], forest["feature"][inner].long()
    for i in range(1000):  # rows that sit exactly on some node's threshold
        j = int(rng.integers(thr.numel()))
        X[i, feat[j]] = thr[j]
    for lo, val in ((1000, float("nan")), (1500, float("inf")), (2000, float("-inf"))):
        mask = torch.from_numpy(rng.random((500, 12)) < 0.3)
        X[lo:lo + 500][mask] = val
    X[2500] = float("nan")
    X[2501] = float("inf")
    X[2502] = float("-inf")
    _check(monkeypatch, forest, X, TCSDN_RF_STREAM_RANGE=500)


# ----------------------------------------------------------------------
# tables too big for two sets of feature rows
# ----------------------------------------------------------------------


def _forest_of(rng, n_nodes):
    """Trees of 63 to 255 nodes until the forest has at least n_nodes."""
    trees, total = [], 0
    while total < n_nodes:
        trees.append(_tree(rng, 6, 7, _pure if len(trees) % 5 else _mixed, p_split=0.85, min_depth=5))
        total += trees[-1]["feature"].size
    assert len(trees) < 1024  # the packed vote register's 10 bits per class
    return oc.rf_flatten(trees, 6), total


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("target,lo,hi", [
    (8_000, TWO_ROWS_MAX_NODES, ONE_ROW_MAX_NODES),  # runs as mode 5
    (15_000, ONE_ROW_MAX_NODES, 1 << 20),            # runs as mode 4
])
def test_big_tables_fall_back(monkeypatch, target, lo, hi):
    forest, n_nodes = _forest_of(np.random.default_rng(target), target)
    assert lo < n_nodes <= hi and n_nodes == forest["feature"].numel()
    _check(monkeypatch, forest, _rows(3000, 15), TCSDN_RF_STREAM_RANGE=400)
