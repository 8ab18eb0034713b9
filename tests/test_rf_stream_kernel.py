"""Streaming forest-predict kernel (TCSDN_RF_MODE=5, the large-batch
default, and 4, the same walk with the node table in L2) against the CPU
oracle ops.cpu.rf_argmax, label for label, and the pack-time order checks
the kernel's termination argument rests on.

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

BLOCKS = (256, 1024)  # threads per block, hence rows of one full refill: modes 4 and 5


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


def _check(monkeypatch, forest, X, ref=None, **env):
    """Labels of the streaming kernel, in both table placements, equal the
    oracle's, row for row."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    if ref is None:
        ref = oc.rf_argmax(X, forest)
    Xd, packed = X.cuda(), dict(forest)
    for mode in ("5", "4"):
        monkeypatch.setenv("TCSDN_RF_MODE", mode)
        got = og.rf_argmax(Xd, packed).cpu()
        assert got.dtype == torch.int32 and got.shape == ref.shape
        assert torch.equal(got, ref), f"mode {mode}"


# ----------------------------------------------------------------------
# shipped forest: refill machinery and the tiled default
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


# rows per wave: the launcher's own choice (64 at these sizes: one refill per
# wave, a cursor that runs dry inside it) and one range for everything (the
# wave refills until a single lane is left)
@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("rows_per_wave", [None, 1 << 20])
@pytest.mark.parametrize(
    "n", [1, 63, 64, 65] + [k for b in BLOCKS for k in (b - 1, b + 1, 2 * b + 7)] + [20_000])
def test_row_counts(monkeypatch, shipped, n, rows_per_wave):
    forest, X, ref = shipped
    env = {} if rows_per_wave is None else {"TCSDN_RF_STREAM_RANGE": rows_per_wave}
    _check(monkeypatch, forest, X[:n], ref[:n], **env)


# refill as soon as one lane is idle, and only when all are
@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("refill", [1, 64])
def test_refill_thresholds(monkeypatch, shipped, refill):
    forest, X, ref = shipped
    _check(monkeypatch, forest, X[:5000], ref[:5000],
           TCSDN_RF_STREAM_RANGE=700, TCSDN_RF_STREAM_REFILL=refill)


@needs_gpu
@pytest.mark.gpu
def test_tiled_default_is_exact(monkeypatch, shipped):
    """Through the public predict_index, nothing forced: 140 000 rows, just
    above the wave-per-row cutover, and 4 000 000, from where the launcher
    picks the streaming kernel itself.  Rows are independent, so copies of
    the 20 000 rows have copies of their labels."""
    from traffic_classifier_sdn_amd.models import load_model

    for k in ("TCSDN_RF_MODE", "TCSDN_RF_STREAM_RANGE", "TCSDN_RF_STREAM_REFILL"):
        monkeypatch.delenv(k, raising=False)
    _, X, ref = shipped
    model = load_model(RF_CKPT, device="cuda")
    Xd = X.cuda()
    for copies in (7, 200):
        got = model.predict_index(Xd.repeat(copies, 1)).cpu()
        assert torch.equal(got, ref.repeat(copies))


# ----------------------------------------------------------------------
# synthetic forests
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 13, 24])
def test_no_early_exit(monkeypatch, T):
    """Uniformly random pure leaf classes: no row is decided early, every
    lane runs to the last tree (T = 13 is no multiple of the 8-tree test
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
    side by side in one wave."""
    rng = np.random.default_rng(13)
    trees = []
    for i in range(12):
        trees.append(_chain(rng, 6, 14, _pure) if i % 3 == 1 else _tree(rng, 6, 1, _pure, min_depth=1))
    _check(monkeypatch, oc.rf_flatten(trees, 6), _rows(3000, 10), TCSDN_RF_STREAM_RANGE=400)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["stream", "wave_per_row"])
@pytest.mark.parametrize("C,T", [(2, 40), (8, 120)])
def test_class_counts(monkeypatch, C, T, kernel):
    """Pure leaves of every class, and enough trees that single classes
    collect more than 15 votes; with C = 8 a 10-bit field per class would
    not fit one 64-bit register.  The same forest also goes through the
    wave-per-row kernel, which is what runs below the cutover when no mode
    is set."""
    rng = np.random.default_rng(20 + C)
    forest = oc.rf_flatten([_tree(rng, C, 4, _pure, min_depth=2) for _ in range(T)], C)
    assert set(forest["leaf_proba"].argmax(dim=1).tolist()) == set(range(C))
    X = _rows(3000, 11)
    proba = oc.rf_predict_proba(X, forest)
    assert float(proba.max()) * T > 15
    ref = torch.argmax(proba, dim=1).to(torch.int32)
    if kernel == "stream":
        _check(monkeypatch, forest, X, ref, TCSDN_RF_STREAM_RANGE=400)
    else:
        monkeypatch.delenv("TCSDN_RF_MODE", raising=False)
        assert torch.equal(og.rf_argmax(X.cuda(), dict(forest)).cpu(), ref)


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
# pack validation (CPU)
# ----------------------------------------------------------------------


def test_pack_rejects_right_child_before_parent():
    rng = np.random.default_rng(15)
    forest = oc.rf_flatten([_tree(rng, 6, 4, _pure, min_depth=2) for _ in range(3)], 6)
    og.rf_pack(forest, "cpu")  # well-formed: accepted
    bad = dict(forest)
    right = forest["right"].clone()
    off = forest["tree_offset"]
    inner = torch.nonzero(forest["feature"] >= 0).flatten()
    j = int(inner[inner > int(off[1])][1])  # an inner node below the second tree's root
    right[j] = 0  # tree-local: back to its own root
    bad["right"] = right
    with pytest.raises(ValueError):
        og.rf_pack(bad, "cpu")
    right[j] = int(off[-1])  # past the end of its own tree
    with pytest.raises(ValueError):
        og.rf_pack(bad, "cpu")


def test_pack_next_root_chain_of_shipped_forest():
    from traffic_classifier_sdn_amd.models import load_model

    forest = load_model(RF_CKPT, device="cpu").forest
    packed = og.rf_pack(forest, "cpu")
    n_nodes = packed["nodes"].shape[0]
    w1 = packed["snodes"][:, 1].to(torch.int64) & 0xFFFFFFFF
    assert w1.numel() == n_nodes + 2
    byte, link = w1 & 0xFF, w1 >> 8
    # the two sentinels link to themselves: a flagged leaf, and an inner
    # node on the feature slot that holds NaN
    assert (int(link[n_nodes]), int(byte[n_nodes])) == (n_nodes, 0x80 | 0x40 | 60)
    assert (int(link[n_nodes + 1]), int(byte[n_nodes + 1])) == (n_nodes + 1, 12)
    byte, link = byte[:n_nodes], link[:n_nodes]
    assert bool((link > torch.arange(n_nodes)).all())  # every link, inner or leaf, points forward
    leaf = byte >= 0x80
    assert torch.equal(leaf, forest["feature"] < 0)
    roots = packed["roots"].to(torch.int64)
    # leaf links, in node order, are the roots of trees 1..T-1 and then n_nodes
    chain = torch.unique_consecutive(link[leaf])
    assert torch.equal(chain, torch.cat([roots[1:], torch.tensor([n_nodes])]))
    assert bool((chain[1:] > chain[:-1]).all()) and int(chain[-1]) == n_nodes
    # flagged: trees 55, 63, ..., 95 of the 100, and the last
    T = roots.numel()
    tree = torch.bucketize(torch.arange(n_nodes), roots, right=True) - 1
    flagged = set(tree[leaf & (byte >= 0xC0)].tolist())
    assert flagged == {t for t in range(T) if (t & 7 == 7 and 2 * t + 2 >= T) or t == T - 1}
    # shifts: a class field, or 61 with the distribution's row + 1 in word0
    shift = byte[leaf] & 63
    w0 = packed["snodes"][:n_nodes, 0][leaf]
    rows = forest["leaf_index"][leaf]
    mixed = shift == 61
    assert bool(mixed.any()) and bool((~mixed).any())
    assert torch.equal(w0[mixed], (rows[mixed] + 1).to(torch.int32))
    assert bool((w0[~mixed] == 0).all())
    assert torch.equal(shift[~mixed], 10 * forest["leaf_proba"][rows[~mixed].long()].argmax(dim=1))


def test_pack_wide_forests_have_no_pure_leaves():
    """Seven classes or more do not fit the packed vote register."""
    rng = np.random.default_rng(16)
    for C, pure in ((6, True), (7, False), (8, False)):
        forest = oc.rf_flatten([_tree(rng, C, 3, _pure, min_depth=1) for _ in range(4)], C)
        packed = og.rf_pack(forest, "cpu")
        byte = packed["nodes"][:, 1] & 0xFF
        leaf = byte >= 0xF0
        assert bool(leaf.any())
        assert bool((byte[leaf] != 0xFF).all()) == pure
        assert bool((byte[leaf] == 0xFF).all()) == (not pure)
        shift = packed["snodes"][:-2, 1][leaf] & 63
        assert bool((shift != 61).all()) == pure
        assert bool((shift == 61).all()) == (not pure)


# ----------------------------------------------------------------------
# class counts at the edges of the launcher's dispatch
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
def test_twelve_classes_below_the_wave_cutover(monkeypatch):
    """The wave-per-row kernel exists for 2..8 classes only: 300 rows of a
    12-class forest fall through to the row-per-lane kernel and get the
    oracle's labels."""
    for k in ("TCSDN_RF_MODE", "TCSDN_RF_STREAM_RANGE", "TCSDN_RF_STREAM_REFILL"):
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(12)
    forest = oc.rf_flatten([_tree(rng, 12, 5, _mixed, min_depth=1) for _ in range(9)], 12)
    X = _rows(300, 13)
    ref = oc.rf_argmax(X, forest)
    assert len(torch.unique(ref)) > 2
    assert torch.equal(og.rf_argmax(X.cuda(), dict(forest)).cpu(), ref)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 131073])  # wave-per-row and row-per-lane path
def test_class_count_without_kernel_raises(monkeypatch, n):
    """Nine classes have no instantiation on either path: an error, not a
    label tensor that no kernel wrote."""
    from traffic_classifier_sdn_amd.ops.gpu import _ext

    monkeypatch.delenv("TCSDN_RF_MODE", raising=False)
    rng = np.random.default_rng(9)
    forest = oc.rf_flatten([_tree(rng, 9, 3, _mixed, min_depth=1)], 9)
    packed = og.rf_pack(forest, "cuda")
    assert packed["n_classes"] == 9 and packed["roots"].numel() == 1
    X = torch.zeros(n, 12, device="cuda")
    with pytest.raises(RuntimeError, match="no kernel for 9 classes"):
        _ext.rf_predict(X, packed["nodes"], packed["snodes"], packed["roots"],
                        packed["leaf_proba"], packed["n_leaves"], 9)
