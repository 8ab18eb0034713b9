"""Forest class-score kernels (csrc/rf_proba_kernels.hip) against the CPU
oracle ops.cpu.rf_predict_scores and an f64 traversal.

Every case runs through the wave-per-row kernel (TCSDN_RF_PROBA_MODE=wave)
and the row-per-lane kernel (=lane); the lane cases run again with
TCSDN_RF_PROBA_BLOCKS=2, so each block loops over several row tiles and the
last one is partial.

Exact cases use leaf distributions in eighths: every class sum is then an
exact f32 value in any summation order, the division by T is IEEE on both
sides, and proba, labels and conf must be equal bit for bit.  Inexact leaves
are compared against an f64 traversal at atol = T * 2^-23: a row's sum is
two f32 chains (mixed-leaf rows, then the pure count) of at most T terms in
[0, 1]; partial sums stay below T, so each chain errs by at most
T * T * 2^-24 before and T * 2^-24 after the division by T.
"""

import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.ops import gpu as og

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RF_CKPT = os.path.join(REPO, "data", "ref_models", "RandomForestClassifier.npz")

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

WAVE_ROWS = (1, 3, 4, 5, 257)  # 4 rows per block: partial, full, second block
LANE_ROWS = (1, 511, 512, 513, 2000)  # 512 rows per block and loop pass
N_ROWS = max(WAVE_ROWS + LANE_ROWS)


# ----------------------------------------------------------------------
# forest builders (trees_-style dicts, depth-first layout), as in
# test_rf_stream_kernel.py
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


def _inexact(rng, C):
    """Counts 1..7 per class: probabilities that are no dyadic fractions."""
    return rng.integers(1, 8, size=C).astype(np.float64)


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


def _chain(rng, C, depth, leaf):
    """Every inner node's left child is a leaf and its right child the next
    inner node: rows that keep going right walk `depth` nodes."""
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


def _proba_f64(X, trees, forest):
    """Class probabilities in f64, one numpy traversal per tree: the leaf
    distributions are normalised in f64 from the trees' counts (the
    forest's own table is their f32 rounding), summed in f64 and divided by
    T.  Routing is the kernels': f32 feature <= f32 threshold goes left."""
    leaf_proba = []
    for t in trees:
        v = np.asarray(t["values"], dtype=np.float64)[np.asarray(t["left"]) == -1]
        leaf_proba.append(v / v.sum(axis=1, keepdims=True))
    leaf_proba = np.concatenate(leaf_proba)
    assert np.array_equal(leaf_proba.astype(np.float32), forest["leaf_proba"].numpy())
    thr = forest["threshold"].numpy()
    right = forest["right"].numpy().astype(np.int64)
    feat = forest["feature"].numpy().astype(np.int64)
    leaf_index = forest["leaf_index"].numpy().astype(np.int64)
    offsets = forest["tree_offset"].numpy().astype(np.int64)
    Xn = X.numpy()
    n, T = Xn.shape[0], offsets.size - 1
    acc = np.zeros((n, leaf_proba.shape[1]), dtype=np.float64)
    for t in range(T):
        base = int(offsets[t])
        idx = np.full(n, base, dtype=np.int64)
        while True:
            rows = np.nonzero(feat[idx] >= 0)[0]
            if rows.size == 0:
                break
            g = idx[rows]
            go_left = Xn[rows, feat[g]] <= thr[g]
            idx[rows] = np.where(go_left, g + 1, base + right[g])
        acc += leaf_proba[leaf_index[idx]]
    return torch.from_numpy(acc / T)


# ----------------------------------------------------------------------
# running the kernels
# ----------------------------------------------------------------------


def _variants():
    """(mode, block cap, row counts) of every kernel path."""
    return (("wave", None, WAVE_ROWS), ("lane", None, LANE_ROWS), ("lane", 2, LANE_ROWS))


def _set_mode(monkeypatch, mode, blocks):
    monkeypatch.setenv("TCSDN_RF_PROBA_MODE", mode)
    if blocks is None:
        monkeypatch.delenv("TCSDN_RF_PROBA_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("TCSDN_RF_PROBA_BLOCKS", str(blocks))


def _check_exact(monkeypatch, forest, X):
    """proba, labels and conf of both kernels equal the oracle's bit for bit
    at every row count, with and without the proba store, and the labels
    equal the argmax kernel's."""
    monkeypatch.delenv("TCSDN_RF_MODE", raising=False)
    ref_p, ref_l, ref_c = oc.rf_predict_scores(X, forest)
    assert ref_l.dtype == torch.int32 and ref_c.dtype == torch.float32
    Xd, packed = X.cuda(), dict(forest)
    for mode, blocks, row_counts in _variants():
        _set_mode(monkeypatch, mode, blocks)
        for n in row_counts:
            if n > X.shape[0]:
                continue
            tag = f"mode {mode} blocks {blocks} n {n}"
            proba, labels, conf = og.rf_predict_scores(Xd[:n], packed)
            assert proba.dtype == torch.float32 and proba.shape == (n, ref_p.shape[1]), tag
            assert labels.dtype == torch.int32 and conf.dtype == torch.float32, tag
            assert torch.equal(proba.cpu(), ref_p[:n]), tag
            assert torch.equal(labels.cpu(), ref_l[:n]), tag
            assert torch.equal(conf.cpu(), ref_c[:n]), tag
            assert torch.equal(labels, og.rf_argmax(Xd[:n], packed)), tag
            none, labels2, conf2 = og.rf_predict_scores(Xd[:n], packed, want_proba=False)
            assert none is None, tag
            assert torch.equal(labels2, labels) and torch.equal(conf2, conf), tag


# ----------------------------------------------------------------------
# exact cases
# ----------------------------------------------------------------------

TREES = (1, 7, 64, 65, 100, 129)  # idle lanes, one pass of the wave, a second pass
CLASSES = (2, 3, 6, 8)  # 8 classes: no packed pure leaves
LEAVES = (_pure, _mixed, _either)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("T", TREES)
def test_exact_scores(monkeypatch, T, C):
    """Every T with every C; the leaf kind (all pure, all mixed, both)
    rotates so that each T and each C meets all three."""
    leaf = LEAVES[(TREES.index(T) + CLASSES.index(C)) % 3]
    rng = np.random.default_rng(1000 * T + C)
    forest = oc.rf_flatten([_tree(rng, C, 5, leaf, min_depth=1) for _ in range(T)], C)
    _check_exact(monkeypatch, forest, _rows(N_ROWS, T + C))


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("leaf", LEAVES)
def test_exact_leaf_kinds_six_classes(monkeypatch, leaf):
    """The shipped shape, 100 trees and 6 classes, with each leaf kind."""
    rng = np.random.default_rng(31)
    forest = oc.rf_flatten([_tree(rng, 6, 6, leaf, min_depth=1) for _ in range(100)], 6)
    pure = forest["leaf_proba"].max(dim=1).values >= 1.0
    assert bool(pure.all()) == (leaf is _pure) and bool((~pure).all()) == (leaf is _mixed)
    _check_exact(monkeypatch, forest, _rows(N_ROWS, 32))


@needs_gpu
@pytest.mark.gpu
def test_single_leaf_trees(monkeypatch):
    """Trees whose root is a leaf: at the first, a middle and the last
    position, and a forest of nothing else."""
    rng = np.random.default_rng(33)
    trees = [_tree(rng, 6, 5, _either, min_depth=1) for _ in range(9)]
    for pos, leaf in ((0, _pure), (4, _mixed), (8, _pure)):
        trees[pos] = _tree(rng, 6, 0, leaf)
    _check_exact(monkeypatch, oc.rf_flatten(trees, 6), _rows(N_ROWS, 34))
    stumps = [_tree(rng, 6, 0, _either) for _ in range(70)]
    _check_exact(monkeypatch, oc.rf_flatten(stumps, 6), _rows(N_ROWS, 35))


@needs_gpu
@pytest.mark.gpu
def test_depth_40_chain(monkeypatch):
    """Depth-40 chains between stumps; rows of +1e30 go right at every node
    and walk a whole chain."""
    rng = np.random.default_rng(36)
    trees = [_chain(rng, 6, 40, _either) if i % 3 == 1 else _tree(rng, 6, 1, _either, min_depth=1)
             for i in range(12)]
    forest = oc.rf_flatten(trees, 6)
    X = _rows(N_ROWS, 37)
    X[::7] = 1e30
    _check_exact(monkeypatch, forest, X)


@needs_gpu
@pytest.mark.gpu
def test_more_trees_than_the_vote_counter_holds(monkeypatch):
    """1100 one-split trees with pure leaves: a 10-bit field per class would
    overflow past 1023 trees, so such a forest is packed without pure
    leaves and every vote goes through the f32 sums."""
    rng = np.random.default_rng(38)
    forest = oc.rf_flatten([_tree(rng, 6, 1, _pure, min_depth=1) for _ in range(1100)], 6)
    _check_exact(monkeypatch, forest, _rows(513, 39))


# ----------------------------------------------------------------------
# inexact leaves
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("T", [7, 100, 129])
def test_inexact_leaves(monkeypatch, T):
    rng = np.random.default_rng(40 + T)
    trees = [_tree(rng, 3, 5, _inexact, min_depth=1) for _ in range(T)]
    forest = oc.rf_flatten(trees, 3)
    X = _rows(N_ROWS, 41)
    ref = _proba_f64(X, trees, forest)
    atol = T * 2.0 ** -23
    Xd, packed = X.cuda(), dict(forest)
    for mode, blocks, row_counts in _variants():
        _set_mode(monkeypatch, mode, blocks)
        for n in row_counts:
            proba, _, conf = og.rf_predict_scores(Xd[:n], packed)
            err = float((proba.cpu().double() - ref[:n]).abs().max())
            print(f"T {T} mode {mode} blocks {blocks} n {n}: max err {err:.3e} (atol {atol:.3e})")
            assert err <= atol
            assert torch.equal(conf, proba.max(dim=1).values)


# ----------------------------------------------------------------------
# shipped forest
# ----------------------------------------------------------------------


@pytest.fixture(scope="module")
def shipped():
    """(forest, {name: (X f32, proba f64)}) for all dataset rows and the
    off-distribution synthetic rows."""
    from traffic_classifier_sdn_amd.models import load_model
    from traffic_classifier_sdn_amd.utils.datasets import load_reference_dataset, synthetic_flow_rows

    model = load_model(RF_CKPT, device="cpu")
    forest = model.forest
    X_real, _ = load_reference_dataset()
    inputs = {
        "dataset": torch.from_numpy(np.asarray(X_real, dtype=np.float32)),
        "synthetic": torch.from_numpy(synthetic_flow_rows(4096, seed=3).astype(np.float32)),
    }
    assert inputs["dataset"].shape == (7653, 12)
    return forest, {k: (X, _proba_f64(X, model.trees_, forest)) for k, X in inputs.items()}


def test_shipped_forest_oracle_and_gaps(shipped):
    """What the GPU comparison below rests on: the f32 CPU oracle is within
    5.5e-8 of the f64 traversal, and no row's two best classes are closer
    than 0.14 (dataset) / 0.01 (synthetic), far above the tolerance."""
    forest, inputs = shipped
    T = forest["tree_offset"].numel() - 1
    assert T == 100
    for name, min_gap in (("dataset", 0.14), ("synthetic", 0.01)):
        X, ref = inputs[name]
        err = float((oc.rf_predict_proba(X, forest).double() - ref).abs().max())
        top2 = torch.topk(ref, 2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1]).min())
        print(f"{name}: oracle max err {err:.3e}, smallest top-two gap {gap:.4f}")
        assert err <= 5.5e-8
        assert gap > min_gap - 1e-6 and gap > 100 * T * 2.0 ** -23


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("mode,blocks", [("wave", None), ("lane", None), ("lane", 2)])
@pytest.mark.parametrize("name", ["dataset", "synthetic"])
def test_shipped_forest(monkeypatch, shipped, name, mode, blocks):
    forest, inputs = shipped
    X, ref = inputs[name]
    T, C = forest["tree_offset"].numel() - 1, int(forest["n_classes"])
    atol = T * 2.0 ** -23  # 1.19e-5
    monkeypatch.delenv("TCSDN_RF_MODE", raising=False)
    _set_mode(monkeypatch, mode, blocks)
    Xd = X.cuda()
    proba, labels, conf = og.rf_predict_scores(Xd, forest)
    err = float((proba.cpu().double() - ref).abs().max())
    row_err = float((proba.double().sum(dim=1) - 1.0).abs().max())
    print(f"{name} {mode} blocks {blocks}: max err {err:.3e}, row-sum err {row_err:.3e}")
    assert err <= atol
    assert row_err <= C * atol
    assert torch.equal(conf, proba.max(dim=1).values)
    assert torch.equal(labels, og.rf_argmax(Xd, forest))
    assert torch.equal(labels.cpu(), torch.argmax(ref, dim=1).to(torch.int32))


# ----------------------------------------------------------------------
# stream capture, unsupported class counts
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["wave", "lane"])
def test_graph_capture(monkeypatch, shipped, mode):
    """Captured at n = 8192 on a side stream, as the serve engine does;
    replayed over new rows in the static input, the outputs equal the eager
    call's."""
    forest, inputs = shipped
    _set_mode(monkeypatch, mode, None)
    rows = torch.cat([inputs["dataset"][0], inputs["synthetic"][0]])
    static_x = rows[:8192].cuda()
    other = rows[-8192:].cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # packs the forest and warms the allocator
            og.rf_predict_scores(static_x, forest)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = og.rf_predict_scores(static_x, forest)
    static_x.copy_(other)
    g.replay()
    torch.cuda.synchronize()
    eager = og.rf_predict_scores(other, forest)
    for got, want in zip(out, eager):
        assert torch.equal(got, want)
    assert not torch.equal(out[1], og.rf_predict_scores(rows[:8192].cuda(), forest)[1])


@needs_gpu
@pytest.mark.gpu
def test_nine_classes_fall_back_and_raw_call_raises():
    """Nine classes run the torch traversal on the device.  Eight trees:
    torch divides a CUDA tensor by a scalar through its reciprocal, which is
    exact for a power of two, so the comparison can stay bitwise."""
    rng = np.random.default_rng(50)
    forest = oc.rf_flatten([_tree(rng, 9, 4, _either, min_depth=1) for _ in range(8)], 9)
    X = _rows(300, 51)
    got = og.rf_predict_proba(X.cuda(), forest)
    assert got.is_cuda and torch.equal(got.cpu(), oc.rf_predict_proba(X, forest))
    packed = og.rf_pack(forest, "cuda")
    with pytest.raises(RuntimeError):
        og._ext.rf_predict_scores(
            X.cuda(), packed["nodes"], packed["roots"], packed["leaf_proba"],
            packed["n_leaves"], 9, True)
