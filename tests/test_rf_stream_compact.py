"""Compact node form of the streaming forest-predict kernel's LDS table
(TCSDN_RF_MODE=5 and 6): the staging loop re-encodes every node (links as
16-bit LDS byte addresses, the feature slot pre-shifted, all clamps made
there, a flagged leaf linking to PARK with its next root kept in word 0),
and the walk trusts what it finds.  Every case compares the kernel's labels
with the CPU oracle ops.cpu.rf_argmax, label for label; the one table that
rf_pack did not make is compared with a row-by-row walk of what the clamped
table means.

Synthetic forests use leaf distributions in eighths, so every score the
oracle and the kernel form is an exact f32 value whatever the summation
order, and ties fall to the first maximum on both sides: equality is exact,
not approximate.
"""

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd.ops import cpu as oc

og = pytest.importorskip("traffic_classifier_sdn_amd.ops.gpu")

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# nodes (without the two sentinels) whose LDS byte addresses fit 16 bits, and
# up to which the table and one set of 1024 13-slot feature rows fit in LDS
COMPACT_MAX_NODES = 65536 // 8 - 2
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


def _either(rng, C):
    return _pure(rng, C) if rng.random() < 0.5 else _mixed(rng, C)


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


def _one_leaf(C, cls):
    """A tree that is a single pure leaf of class `cls`."""
    values = np.zeros((1, C))
    values[0, cls] = 5.0
    return {"left": np.asarray([-1]), "right": np.asarray([-1]), "feature": np.asarray([-2]),
            "threshold": np.asarray([-2.0]), "values": values}


def _chain(rng, C, depth, leaf):
    """Every inner node's left child is a leaf and its right child the next
    inner node: 2 * depth + 1 nodes, the last one the leaf at the end."""
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


def _check(monkeypatch, forest, X, modes, ref=None, **env):
    """Labels of the kernels that TCSDN_RF_MODE in `modes` runs equal the
    oracle's, row for row."""
    monkeypatch.delenv("TCSDN_RF_STREAM_REFILL", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    if ref is None:
        ref = oc.rf_argmax(X, forest)
    Xd, packed = X.cuda(), dict(forest)
    for mode in modes:
        monkeypatch.setenv("TCSDN_RF_MODE", mode)
        got = og.rf_argmax(Xd, packed).cpu()
        assert got.dtype == torch.int32 and got.shape == ref.shape
        assert torch.equal(got, ref), f"mode {mode}"


# ----------------------------------------------------------------------
# both sides of the 16-bit link limit
# ----------------------------------------------------------------------


def _forest_of_exactly(rng, n_nodes):
    """Trees of 63 to 255 nodes, pure and mixed leaves, then a chain (and a
    single leaf where the parity asks for one) that brings the forest to
    exactly n_nodes."""
    trees, total = [], 0
    while total < n_nodes - 400:
        trees.append(_tree(rng, 6, 7, _either, p_split=0.85, min_depth=5))
        total += trees[-1]["feature"].size
    rest = n_nodes - total
    if rest % 2 == 0:
        trees.append(_one_leaf(6, 3))
        rest -= 1
    trees.append(_chain(rng, 6, (rest - 1) // 2, _either))
    assert len(trees) < 1024  # the packed vote register's 10 bits per class
    forest = oc.rf_flatten(trees, 6)
    assert forest["feature"].numel() == n_nodes
    return forest


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes", [COMPACT_MAX_NODES, COMPACT_MAX_NODES + 1, 13_001])
def test_link_limit(monkeypatch, n_nodes):
    """8190 nodes: n_nodes + 2 entries end at LDS byte 65536 exactly and the
    table walks in the compact form; 8191: one entry more, the launcher keeps
    the host format, as it does near 13 000 nodes."""
    assert COMPACT_MAX_NODES == 8190 and n_nodes <= ONE_ROW_MAX_NODES
    forest = _forest_of_exactly(np.random.default_rng(n_nodes), n_nodes)
    _check(monkeypatch, forest, _rows(2000, 21), ("5",), TCSDN_RF_STREAM_RANGE=300)


# ----------------------------------------------------------------------
# class counts, in both LDS-table kernels
# ----------------------------------------------------------------------


def _small_mixed_forest(rng, C):
    """T = 17, so trees 15 (t & 7 == 7, 2t + 2 >= T) and 16 (the last) are
    the tested ones.  Single-leaf trees at the front, in the middle and as
    tested tree 15; depth-20 chains; pure and mixed leaves."""
    trees = []
    for i in range(17):
        if i in (0, 6, 15):
            trees.append(_tree(rng, C, 0, _mixed if i == 6 else _pure))
        elif i % 4 == 1:
            trees.append(_chain(rng, C, 20, _either))
        else:
            trees.append(_tree(rng, C, 5, _either, min_depth=1))
    return oc.rf_flatten(trees, C)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C,modes", [(2, "65"), (3, "65"), (6, "65"), (8, "65"), (12, "5"), (16, "5")])
def test_class_counts(monkeypatch, C, modes):
    forest = _small_mixed_forest(np.random.default_rng(30 + C), C)
    _check(monkeypatch, forest, _rows(1000, 22), tuple(modes), TCSDN_RF_STREAM_RANGE=129)


@needs_gpu
@pytest.mark.gpu
def test_mixed_leaf_ends_tested_trees(monkeypatch):
    """The last node of tested tree 15 and of the last tree is a mixed leaf:
    word 0 of the LDS copy carries the distribution's row beside the next
    root that the pass reads back."""
    rng = np.random.default_rng(31)
    trees = [_tree(rng, 6, 5, _pure, min_depth=2) for _ in range(17)]
    trees[7] = _chain(rng, 6, 6, _mixed)   # t & 7 == 7, but 2t + 2 < T: not tested
    trees[15] = _chain(rng, 6, 20, _mixed)
    trees[16] = _tree(rng, 6, 4, _mixed, min_depth=2)
    forest = oc.rf_flatten(trees, 6)
    packed = og.rf_pack(forest, "cpu")
    byte = packed["snodes"][:, 1].to(torch.int64) & 0xFF
    off = forest["tree_offset"]
    for t, flagged in ((7, False), (15, True), (16, True)):
        last = int(byte[int(off[t + 1]) - 1])
        assert last & 63 == 61 and last >= 0x80 and (last >= 0xC0) == flagged
    X = _rows(1000, 23)
    X[:300] += 1.5  # more rows that keep going right, to the chains' ends
    _check(monkeypatch, forest, X, ("6", "5"), TCSDN_RF_STREAM_RANGE=129)


# ----------------------------------------------------------------------
# special values
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
def test_special_values(monkeypatch):
    """Rows hold NaN, +-inf and -0.0, thresholds include +-0.0.  NaN goes
    right, as `fv <= thr` does; -0.0 and 0.0 compare equal and go left."""
    rng = np.random.default_rng(32)
    trees = [_tree(rng, 6, 6, _either, min_depth=3) for _ in range(17)]
    forest = oc.rf_flatten(trees, 6)
    inner = torch.nonzero(forest["feature"] >= 0).flatten()
    thr = forest["threshold"].clone()
    pick = inner[torch.from_numpy(rng.permutation(inner.numel())[: inner.numel() // 3])]
    thr[pick[0::2]] = 0.0
    thr[pick[1::2]] = -0.0
    assert bool(torch.signbit(thr[pick[1::2]]).all()) and not bool(torch.signbit(thr[pick[0::2]]).any())
    forest["threshold"] = thr
    X = _rows(3000, 24)
    for lo, val in ((0, float("nan")), (500, float("inf")), (1000, float("-inf")),
                    (1500, -0.0), (2000, 0.0)):
        mask = torch.from_numpy(rng.random((500, 12)) < 0.3)
        X[lo:lo + 500][mask] = val
    X[2500] = float("nan")
    X[2501] = float("inf")
    X[2502] = float("-inf")
    X[2503] = -0.0
    assert bool(torch.signbit(X[2503]).all())
    _check(monkeypatch, forest, X, ("6", "5"), TCSDN_RF_STREAM_RANGE=300)


# ----------------------------------------------------------------------
# the vote field's range and the end of the table
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tie", "landslide", "too_many_trees"])
def test_single_leaf_forests(monkeypatch, case):
    """Single-leaf trees only, so the table is one chain of leaves.
    tie: 1023 trees, classes 1 and 4 in turn and one vote for class 0 at the
    end; the margin never exceeds 1, no row exits early, every row walks to
    the terminal entry and the tie at 511 falls to class 1.
    landslide: 1022 votes for class 5, the widest a 10-bit field gets with a
    second class present, then one for class 2.
    too_many_trees: 1023 trees of class 5 and one of class 2 are 1024 trees,
    which rf_pack gives no pure leaves: every vote is a distribution row."""
    if case == "tie":
        classes = [1, 4] * 511 + [0]
    elif case == "landslide":
        classes = [5] * 1022 + [2]
    else:
        classes = [5] * 1023 + [2]
    forest = oc.rf_flatten([_one_leaf(6, c) for c in classes], 6)
    X = _rows(1000, 25)
    ref = oc.rf_argmax(X, forest)
    assert bool((ref == (1 if case == "tie" else 5)).all())
    _check(monkeypatch, forest, X, ("6", "5"), ref, TCSDN_RF_STREAM_RANGE=129)


# ----------------------------------------------------------------------
# tables rf_pack did not make: the clamps of the staging loop
# ----------------------------------------------------------------------


def _walk_snodes(sn, n_nodes, n_leaves, proba, X, C):
    """What a streaming table MEANS, row by row, with the kernel's clamps: a
    feature byte above 11 reads NaN and goes right, a mixed leaf's row is at
    most n_leaves - 1, a link at or past n_nodes ends the row.  Entries
    n_nodes and n_nodes + 1 are never looked at.  Every tree counts; the
    kernel's early exit is exact, so the first-maximum argmax is the same."""
    w0 = sn[:, 0].astype(np.int64) & 0xFFFFFFFF
    w1 = sn[:, 1].astype(np.int64) & 0xFFFFFFFF
    thr = sn[:, 0].copy().view(np.float32)
    out = np.zeros(len(X), dtype=np.int32)
    for r, row in enumerate(X):
        score = np.zeros(C, dtype=np.float64)
        idx, visits = 0, 0
        while idx < n_nodes:
            visits += 1
            assert visits <= n_nodes  # links point forward in these tables
            byte, link = int(w1[idx]) & 0xFF, int(w1[idx]) >> 8
            if byte >= 0x80:
                shift = byte & 63
                if shift < 60:
                    score[shift // 10] += 1.0
                if w0[idx]:
                    score += proba[min(int(w0[idx]) - 1, n_leaves - 1)]
                idx = link
            else:
                left = byte < 12 and row[byte] <= thr[idx]
                idx = idx + 1 if left else link
        out[r] = int(np.argmax(score))
    return out


@needs_gpu
@pytest.mark.gpu
def test_foreign_table_is_clamped_while_staging(monkeypatch):
    """rf_pack's table with four kinds of damage, handed to the extension
    directly: inner nodes with a feature byte above 12, mixed leaves whose
    row lies past n_leaves, the last tree's leaves linking far past the
    table, and both sentinels overwritten (the PARK entry by a flagged leaf
    that links backward).  The compact form applies its clamps and writes
    its own sentinels in the staging loop, so modes 5 and 6 give the labels
    of the clamped table."""
    from traffic_classifier_sdn_amd.ops.gpu import _ext

    rng = np.random.default_rng(41)
    forest = _small_mixed_forest(rng, 6)
    packed = og.rf_pack(forest, "cpu")
    sn = packed["snodes"].numpy().copy()
    n_nodes, n_leaves = sn.shape[0] - 2, packed["n_leaves"]
    w1 = sn[:n_nodes, 1].astype(np.int64) & 0xFFFFFFFF
    byte = w1 & 0xFF
    inner = np.nonzero(byte < 0x80)[0]
    mixed = np.nonzero((byte >= 0x80) & (sn[:n_nodes, 0] != 0))[0]
    last = np.nonzero((byte >= 0x80) & ((w1 >> 8) == n_nodes))[0]
    assert len(inner) > 20 and len(mixed) > 20 and len(last) > 1
    odd = inner[rng.permutation(len(inner))[: len(inner) // 8]]
    far = mixed[rng.permutation(len(mixed))[: len(mixed) // 8]]

    def put(i, word0, link, b):
        sn[i, 0] = np.int64(word0).astype(np.int32) if word0 is not None else sn[i, 0]
        sn[i, 1] = np.array([(link << 8) | b], dtype=np.int64).astype(np.uint32).view(np.int32)[0]

    for i in odd:
        put(i, None, int(w1[i] >> 8), 0x0D + int(rng.integers(0x70)))
    for i in far:
        put(i, n_leaves + 1 + int(rng.integers(1000)), int(w1[i] >> 8), int(byte[i]))
    for i in last:
        put(i, None, (1 << 24) - 1, int(byte[i]))
    put(n_nodes, 0x3F800000, 3, 0x05)            # terminal entry: an inner node
    put(n_nodes + 1, 7, 0, 0x80 | 0x40 | 20)     # PARK: a flagged leaf linking to node 0

    X = _rows(600, 26)
    ref = torch.from_numpy(_walk_snodes(sn, n_nodes, n_leaves, packed["leaf_proba"].numpy().astype(np.float64),
                                        X.numpy(), 6))
    assert len(torch.unique(ref)) > 2
    monkeypatch.setenv("TCSDN_RF_STREAM_RANGE", "129")
    monkeypatch.delenv("TCSDN_RF_STREAM_REFILL", raising=False)
    args = (packed["nodes"].cuda(), torch.from_numpy(sn).cuda(), packed["roots"].cuda(),
            packed["leaf_proba"].cuda(), n_leaves, 6)
    for mode in ("6", "5"):
        monkeypatch.setenv("TCSDN_RF_MODE", mode)
        got = _ext.rf_predict(X.cuda(), *args).cpu()
        assert torch.equal(got, ref), f"mode {mode}"


@needs_gpu
@pytest.mark.gpu
def test_too_many_leaf_rows_walk_the_host_format(monkeypatch):
    """65 535 rows of leaf_proba do not fit the compact form's 16-bit row
    field: the launcher runs modes 6 and 5 as mode 5 in the host format."""
    from traffic_classifier_sdn_amd.ops.gpu import _ext

    forest = _small_mixed_forest(np.random.default_rng(42), 6)
    X = _rows(600, 27)
    ref = oc.rf_argmax(X, forest)
    packed = og.rf_pack(forest, "cuda")
    n_leaves = 65535
    proba = torch.zeros(n_leaves, 6)
    proba[: packed["n_leaves"]] = packed["leaf_proba"].cpu()
    monkeypatch.setenv("TCSDN_RF_STREAM_RANGE", "129")
    monkeypatch.delenv("TCSDN_RF_STREAM_REFILL", raising=False)
    for mode in ("6", "5"):
        monkeypatch.setenv("TCSDN_RF_MODE", mode)
        got = _ext.rf_predict(X.cuda(), packed["nodes"], packed["snodes"], packed["roots"],
                              proba.cuda(), n_leaves, 6).cpu()
        assert torch.equal(got, ref), f"mode {mode}"
