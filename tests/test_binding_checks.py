"""Every bound op of the extension (csrc/ext.cpp), called directly: one valid
call at the smallest shape, and one rejection per argument that a kernel
indexes.

The kernels index by their counts alone, so a tensor that is too short must
never reach a launch.  Every rejection here is raised by the binding's checks
before anything is launched: no case lets a kernel run on bad arguments, and
none could only be told apart by doing so.

Valid calls are compared with the oracles of ops/cpu.py (or a few lines of
torch where the op has none) at the tolerance of the op's own test:
  labels, indices, counts, histograms   equal
  gnb_proba, linear_proba                atol 2^-23   (test_proba_kernels)
  rf_predict_scores                      atol T * 2^-23 (test_rf_proba_kernel)
  ensemble_vote                          atol M * 2^-23 (test_ensemble_vote_kernel)
  proba_smooth                           atol 2^-23   (test_proba_smooth_kernel)
  svc_decision                           atol Sd * 2^-16 per pair, svc_couple
                                         atol 2^-22   (test_svc_proba_kernels)
  knn distances, kmeans sums             rtol 1e-3    (test_gpu_kernels)
  gnb_fit_stats, logistic_grad           rtol 1e-10, 1e-8 (test_gpu_kernels)
  flow_features                          rtol 1e-6    (test_gpu_kernels)
The SMO updates have no test of their own values; kernel and torch both
evaluate exp(-gamma * d2) in f32 on |gamma * d2| of a few units, where a
hardware exp good to a few ulp and 15 roundings of its argument stay below a
relative 2^-20 (the derivation of test_svc_proba_kernels), and the f64 sum of
two such terms keeps that: rtol 2^-19.
"""

import re

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd.ops import cpu as oc

og = pytest.importorskip("traffic_classifier_sdn_amd.ops.gpu")  # needs the built extension

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

N, C = 3, 3
GAMMA = float(np.float32(0.05))
LDS_LIMIT = 64 * 1024  # dynamic LDS of a launch that raised no limit


def _rng(seed):
    return np.random.default_rng(seed)


def f32(seed, *shape):
    return torch.from_numpy(_rng(seed).normal(size=shape).astype(np.float32))


def f64(seed, *shape):
    return torch.from_numpy(_rng(seed).normal(size=shape))


def i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def u8(*v):
    return torch.tensor(v, dtype=torch.uint8)


def key(value, row):
    """A packed select key as the SMO kernels read it: value << 32 | row."""
    return (value << 32) | row


X = f32(1, N, 12)
Y_PM = torch.tensor([1.0, -1.0, 1.0])  # SMO labels
GRAD = torch.tensor([-3.0, -2.0, -1.0], dtype=torch.float64)
BINS = torch.from_numpy(_rng(2).integers(0, 256, size=(N, 12)).astype(np.uint8))
NID = i32(0, 1, -1)
N_SUPPORT = torch.tensor([2, 1, 1])


def _forest():
    """Two one-split trees, mixed leaves in the first, pure ones in the second."""
    def tree(feature, values):
        return {"left": [1, -1, -1], "right": [2, -1, -1], "feature": [feature, -2, -2],
                "threshold": [0.0, 0.0, 0.0], "values": [[1, 1, 1]] + values}

    return oc.rf_flatten([tree(0, [[3, 1, 0], [0, 1, 3]]), tree(1, [[4, 0, 0], [0, 0, 4]])], C)


def _packed():
    return og.rf_pack(_forest(), "cpu")


# ----------------------------------------------------------------------
# the ops: arguments of one valid call (CPU tensors, moved by _call), and
# for each a check of what it returns or updates
# ----------------------------------------------------------------------


def _close(got, ref, atol=0.0, rtol=0.0):
    got, ref = got.cpu().double(), ref.cpu().double()
    assert got.shape == ref.shape
    assert bool(((got - ref).abs() <= atol + rtol * ref.abs()).all()), (got, ref)


def _is(t, dtype, *shape):
    assert t.dtype == dtype and tuple(t.shape) == shape and t.is_cuda, (t.dtype, t.shape)


def a_gnb_predict():
    return dict(X=X, theta=f32(3, C, 12), inv_var=f32(4, C, 12).abs() + 0.5, cconst=f32(5, C))


def c_gnb_predict(out, a):
    _is(out, torch.int32, N)
    d = X.double()[:, None, :] - a["theta"].double()
    score = a["cconst"].double() - 0.5 * (d * d * a["inv_var"].double()).sum(-1)
    assert torch.equal(out.cpu().long(), score.argmax(1))


def a_linear_argmax():
    return dict(X=X, W=f32(6, C, 12), b=f32(7, C))


def c_linear_argmax(out, a):
    _is(out, torch.int32, N)
    assert torch.equal(out.cpu(), oc.linear_argmax(X, a["W"], a["b"]).to(torch.int32))


def a_kmeans_assign():
    return dict(X=X, centers=f32(8, C, 12), want_update=True)


def c_kmeans_assign(out, a):
    labels, counts, sums, inertia = out
    _is(labels, torch.int32, N), _is(counts, torch.float64, C)
    _is(sums, torch.float64, C, 12), _is(inertia, torch.float64, 1)
    rl, rc, rs, ri = oc.kmeans_assign(X.double(), a["centers"].double())
    assert torch.equal(labels.cpu(), rl)
    _close(counts, rc), _close(sums, rs, rtol=1e-3), _close(inertia[0], ri, rtol=1e-3)


def a_rf_predict():
    p = _packed()
    return dict(X=X, nodes=p["nodes"], snodes=p["snodes"], roots=p["roots"],
                leaf_proba=p["leaf_proba"], n_leaves=p["n_leaves"], C=C)


def c_rf_predict(out, a):
    _is(out, torch.int32, N)
    assert torch.equal(out.cpu(), oc.rf_argmax(X, _forest()))


def a_rf_predict_scores():
    a = a_rf_predict()
    del a["snodes"]
    return dict(a, want_proba=True)


def c_rf_predict_scores(out, a):
    proba, labels, conf = out
    _is(proba, torch.float32, N, C), _is(labels, torch.int32, N), _is(conf, torch.float32, N)
    rp, rl, rc = oc.rf_predict_scores(X, _forest())
    _close(proba, rp, atol=2 * 2.0 ** -23), _close(conf, rc, atol=2 * 2.0 ** -23)
    assert torch.equal(labels.cpu(), rl)


def _gnb64():
    return f64(9, C, 12), f64(10, C, 12).abs() + 0.5, torch.tensor([0.2, 0.3, 0.5], dtype=torch.float64)


def a_gnb_proba():
    theta, var, prior = _gnb64()
    const = torch.log(prior) - 0.5 * torch.log(2.0 * torch.pi * var).sum(dim=1)
    return dict(X=X, theta=theta, inv_var=1.0 / var, cconst=const)


def c_gnb_proba(out, a):
    _is(out, torch.float32, N, C)
    _close(out, oc.gnb_proba(X, *_gnb64()), atol=2.0 ** -23)


def a_linear_proba():
    return a_linear_argmax()


def c_linear_proba(out, a):
    _is(out, torch.float32, N, C)
    _close(out, oc.linear_proba(X, a["W"], a["b"]), atol=2.0 ** -23)


def a_knn_vote_proba():
    return dict(idx=torch.tensor([[0, 1], [4, 4], [2, 3]], dtype=torch.int32), y=u8(0, 1, 2, 2, 1), C=C)


def c_knn_vote_proba(out, a):
    _is(out, torch.float32, N, C)
    assert torch.equal(out.cpu(), oc.knn_vote_proba(a["idx"], a["y"], C))


def _members():
    p = [torch.softmax(f32(11, N, 3), 1), torch.softmax(f32(12, N, 2), 1)]
    return p, [[0, 1, 2], [0, 2]]


def a_ensemble_vote():
    p, maps = _members()
    return dict(probas=p, colmaps=maps, weights=[0.5, 0.5], C=C, want_proba=True)


def c_ensemble_vote(out, a):
    avg, labels, conf = out
    _is(avg, torch.float32, N, C), _is(labels, torch.int32, N), _is(conf, torch.float32, N)
    ra, rl, rc = oc.ensemble_vote(*_members(), [1.0, 1.0], C)
    _close(avg, ra, atol=2 * 2.0 ** -23), _close(conf, rc, atol=2 * 2.0 ** -23)
    assert torch.equal(labels.cpu(), rl)


def _smooth_state():
    return torch.softmax(f32(14, N, C), 1), i32(0, -1, 2)


def a_proba_smooth():
    state, held = _smooth_state()
    return dict(proba=torch.softmax(f32(13, N, C), 1), state=state, held=held,
                n_live=i32(2), alpha=0.5, margin=0.0)


def c_proba_smooth(out, a, moved):
    labels, conf = out
    _is(labels, torch.int32, N), _is(conf, torch.float32, N)
    state, held = _smooth_state()
    rl, rc = oc.proba_smooth(a["proba"], state, held, 0.5, 0.0, a["n_live"])
    assert torch.equal(labels.cpu(), rl) and torch.equal(moved["held"].cpu(), held)
    _close(conf, rc, atol=2.0 ** -23), _close(moved["state"], state, atol=2.0 ** -23)


def a_class_traffic():
    return dict(X=X, labels=i32(2, 0, 7), n_classes=C, conf=torch.tensor([0.9, 0.1, 0.8]),
                min_conf=0.5, n_live=i32(3))


def c_class_traffic(out, a):
    _is(out, torch.float64, C + 1, 13)
    _close(out, oc.class_traffic(*a.values()), rtol=2.0 ** -50)


def a_svc_predict():
    return dict(X=X, SV=f32(15, 4, 12), dual=f32(16, C - 1, 4), svclass=u8(0, 0, 1, 2),
                intercept=f32(17, 3), gamma=GAMMA)


def _svc_dec(a):
    K = oc.rbf_kernel(X.double(), a["SV"].double(), GAMMA)
    return oc.svc_ovo_decision(K, a["dual"].double(), a["intercept"].double(), N_SUPPORT)


def c_svc_predict(out, a):
    _is(out, torch.int32, N)
    assert torch.equal(out.cpu(), oc.svc_vote(_svc_dec(a), C))


a_svc_decision = a_svc_predict


def c_svc_decision(out, a):
    _is(out, torch.float64, N, 3)
    d = a["dual"].double().abs()  # Sd per pair: |dual| over the pair's SVs
    sd = torch.stack([d[0, 2] + d[0, :2].sum(), d[1, :2].sum() + d[0, 3], d[1, 2] + d[1, 3]])
    assert bool(((out.cpu() - _svc_dec(a)).abs() <= sd * 2.0 ** -16).all())


def a_svc_couple():
    return dict(dec=f64(18, N, 3), probA=-f64(19, 3).abs() - 0.5, probB=f64(20, 3) * 0.1, C=C)


def c_svc_couple(out, a):
    proba, idx, conf = out
    _is(proba, torch.float32, N, C), _is(idx, torch.int32, N), _is(conf, torch.float32, N)
    rp, ri, rc, margin = oc.svc_couple(a["dec"], a["probA"], a["probB"], C, with_margin=True)
    assert float(margin.min()) > 1e-9  # kernel and oracle make the same sweeps
    _close(proba, rp, atol=2.0 ** -22), _close(conf, rc, atol=2.0 ** -22)
    assert torch.equal(idx.cpu(), ri)


R = f32(21, 5, 12)


def a_knn_topk():
    return dict(Q=X, R=R, ry=u8(0, 1, 2, 2, 1), k=2, C=C, idx_base=0)


def c_knn_topk(out, a):
    dist, idx, lab = out
    _is(dist, torch.float32, N, 2), _is(idx, torch.int32, N, 2), _is(lab, torch.int32, N)
    rd, ri = torch.topk(torch.cdist(X.double(), R.double()).pow(2), 2, dim=1, largest=False)
    assert torch.equal(idx.cpu().long(), ri)
    _close(dist, rd, rtol=1e-3)
    assert torch.equal(lab.cpu(), oc.knn_vote(ri, a["ry"], C))


def a_knn_topk_mfma():
    a = a_knn_topk()
    return dict(Q=X, R=R, cmean=R.mean(0), ry=a["ry"], k=2, C=C, idx_base=0, n_shards=1, approx=0)


c_knn_topk_mfma = c_knn_topk


def a_gnb_fit_stats():
    return dict(X=X.double(), y=torch.tensor([0, 2, 0]), C=C)


def c_gnb_fit_stats(out, a):
    for got, ref, shape in zip(out, oc.gnb_fit_stats(a["X"], a["y"], C), ((C,), (C, 12), (C, 12))):
        _is(got, torch.float64, *shape)
        _close(got, ref, rtol=1e-10)


def a_logistic_grad():
    return dict(X=X.double(), y=torch.tensor([0, 2, 1]), W=f64(22, C, 12), b=f64(23, C))


def c_logistic_grad(out, a):
    grad, loss = out
    _is(grad, torch.float64, C, 13), _is(loss, torch.float64, 1)
    rl, rw, rb = oc.logistic_loss_grad(a["X"], a["y"], a["W"], a["b"], l2=0.0)
    _close(loss[0], rl, rtol=1e-10), _close(grad[:, :12], rw, rtol=1e-8), _close(grad[:, 12], rb, rtol=1e-8)


def a_flow_features():
    prev = torch.from_numpy(_rng(24).integers(0, 10_000, (N, 4)).astype(np.float64))
    t0 = torch.full((N, 1), 100.0, dtype=torch.float64)
    times = torch.cat([t0 + 10, t0 + 9, t0 + 10, t0 + 8, t0, t0 * 0], dim=1)
    times[0, 1] = times[0, 0]  # a zero time delta
    return dict(cur=prev + 7.0, prev=prev, times=times)


def c_flow_features(out, a):
    _is(out, torch.float32, N, 12)
    _close(out, oc.flow_features(*a.values()), rtol=1e-6)


# SMO: rows 0 and 2 are in I_up, rows 1 and 2 in I_low (0 < alpha[2] < C)
ALPHA = torch.tensor([0.0, 0.0, 0.5], dtype=torch.float64)
KROW = torch.tensor([1.0, 0.5, 0.25])
ROWS = torch.cat([X[0], X[1]])
SOL = torch.tensor([0.5, -0.25, 0.0, 0.0], dtype=torch.float64)
SMO_RTOL = 2.0 ** -19


def _krow(i):
    return torch.exp(-GAMMA * (X - X[i]).pow(2).sum(1)).double()


def a_smo_select():
    return dict(y=Y_PM, alpha=ALPHA, grad=GRAD, C=1.0, out=torch.zeros(2, dtype=torch.int64))


def c_smo_select(out, a, moved):
    # -y * grad = 3, -2, 1: the largest of I_up is row 0, the smallest of I_low row 1
    assert (moved["out"].cpu() & 0xFFFFFFFF).tolist() == [0, 1]


def a_smo_solve():  # an empty selection: the solve reports convergence
    return dict(X=X, y=Y_PM, alpha=ALPHA, grad=GRAD, sel=torch.zeros(2, dtype=torch.int64),
                rows=torch.zeros(24), sol=torch.zeros(4, dtype=torch.float64), C=1.0, tol=1e-3, gamma=GAMMA)


def c_smo_solve(out, a, moved):
    assert moved["sol"].cpu().tolist() == [0.0, 0.0, 1.0, 0.0]
    assert torch.equal(moved["alpha"].cpu(), ALPHA)


def a_smo_solve2():
    return dict(a_smo_solve(), sel=torch.zeros(3, dtype=torch.int64))


c_smo_solve2 = c_smo_solve


def a_smo_update_dev():
    return dict(X=X, y=Y_PM, grad=GRAD, rows=ROWS, sol=SOL, gamma=GAMMA)


def c_smo_update_dev(out, a, moved):
    _close(moved["grad"], GRAD + Y_PM.double() * (0.5 * _krow(0) - 0.25 * _krow(1)), rtol=SMO_RTOL)


def a_smo_update():
    return dict(X=X, y=Y_PM, grad=GRAD, rows=ROWS, yidai=0.5, yjdaj=-0.25, gamma=GAMMA)


c_smo_update = c_smo_update_dev


def a_smo_row():
    return dict(X=X, sel=torch.tensor([key(1, 1)]), sol=torch.zeros(4, dtype=torch.float64),
                krow=torch.zeros(N), gamma=GAMMA)


def c_smo_row(out, a, moved):
    _close(moved["krow"], _krow(1), rtol=SMO_RTOL)


def a_smo_select2():
    return dict(y=Y_PM, alpha=ALPHA, grad=GRAD, krow=KROW, sel=torch.tensor([key(1, 0), 0, 0]),
                sol=torch.zeros(4, dtype=torch.float64), C=1.0)


def c_smo_select2(out, a, moved):
    # i = 0, Gmax = 3.  Row 1: gd = 5, a = 2 + 2 * 0.5, gain 25 / 3; row 2:
    # gd = 2, a = 2 - 2 * 0.25, gain 4 / 1.5: row 1
    assert int(moved["sel"][2].cpu()) & 0xFFFFFFFF == 1


def a_smo_update_dev2():
    return dict(X=X, y=Y_PM, grad=GRAD, rows=ROWS, sol=SOL, krow=KROW, gamma=GAMMA)


def c_smo_update_dev2(out, a, moved):
    _close(moved["grad"], GRAD + Y_PM.double() * (0.5 * KROW.double() - 0.25 * _krow(1)), rtol=SMO_RTOL)


Y_CLS = u8(0, 2, 1)


def a_rf_hist():
    return dict(bins=BINS, y=Y_CLS, nid=NID, hist=torch.zeros(2, 12, 256, C, dtype=torch.int32),
                fsel=torch.ones(2, 12, dtype=torch.uint8))


def c_rf_hist(out, a, moved):
    assert torch.equal(moved["hist"].cpu(), oc.rf_hist(BINS, Y_CLS, NID, 2, C))


def a_rf_split():
    return dict(hist=oc.rf_hist(BINS, Y_CLS, NID, 2, C), fsel=torch.ones(2, 12, dtype=torch.uint8))


def c_rf_split(out, a):
    best, cnt = out
    _is(best, torch.int64, 2), _is(cnt, torch.int32, 2, C)
    assert torch.equal(cnt.cpu(), a["hist"][:, 0].sum(dim=1).to(torch.int32))
    assert best.cpu().tolist() == [-1, -1]  # one row per node: nothing to split


def a_rf_level_compact():
    frank = torch.full((2, 12), 0xFF, dtype=torch.uint8)
    frank[:, 0], frank[:, 1] = 0, 1
    return dict(bins=BINS, y=Y_CLS, nid=NID, frank=frank, fidx=u8(0, 1, 0, 1).reshape(2, 2), L=2, C=C)


def c_rf_level_compact(out, a):
    c_rf_split(out, dict(hist=oc.rf_hist(BINS, Y_CLS, NID, 2, C)))


def a_rf_partition():
    return dict(B=BINS, nid=NID, lmap=i32(4, -1), feat=i32(5, 0), binthr=i32(int(BINS[0, 5]), 0))


def c_rf_partition(out, a, moved):
    assert moved["nid"].cpu().tolist() == [4, -1, -1]  # bin <= threshold: the left child


OPS = [
    "gnb_predict", "linear_argmax", "kmeans_assign", "rf_predict", "rf_predict_scores",
    "gnb_proba", "linear_proba", "knn_vote_proba", "ensemble_vote", "proba_smooth",
    "class_traffic", "svc_predict", "svc_decision", "svc_couple", "knn_topk", "knn_topk_mfma",
    "gnb_fit_stats", "logistic_grad", "flow_features", "smo_select", "smo_solve", "smo_solve2",
    "smo_update_dev", "smo_update", "smo_row", "smo_select2", "smo_update_dev2", "rf_hist",
    "rf_split", "rf_level_compact", "rf_partition",
]


def _args(op):
    return globals()["a_" + op]()


def _cuda(v):
    if isinstance(v, torch.Tensor):
        return v.cuda()
    if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
        return [t.cuda() for t in v]
    return v


def _call(op, args):
    """Runs the op on `args` moved to the GPU; returns (result, moved args)."""
    moved = {k: _cuda(v) for k, v in args.items()}
    return getattr(og._ext, op)(*moved.values()), moved


def test_every_bound_op_is_listed():
    src = open(_src("ext.cpp")).read()
    assert sorted(re.findall(r'm\.def\("(\w+)"', src)) == sorted(OPS) and len(OPS) == 31


def _src(name):
    import os

    import traffic_classifier_sdn_amd as pkg

    return os.path.join(os.path.dirname(pkg.__file__), "csrc", name)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_valid_call(op):
    args = _args(op)
    out, moved = _call(op, args)
    check = globals()["c_" + op]
    if check.__code__.co_argcount == 3:  # the op updates its arguments in place
        assert out is None or isinstance(out, (list, tuple))
        check(out, args, moved)
    else:
        check(out, args)


# ----------------------------------------------------------------------
# rejections
# ----------------------------------------------------------------------

# Per op: the arguments that are too short with their last element (or last
# row, for a matrix) gone, and the argument the message then names.  A tensor
# that only DEFINES a count (X and n, roots and T) cannot be too short; one
# that defines a count other tensors must match (theta and C) is, and the
# message names the tensor that no longer matches.
SHORT = {
    "gnb_predict": {"theta": "inv_var", "inv_var": "inv_var", "cconst": "cconst"},
    "linear_argmax": {"W": "b", "b": "b"},
    "rf_predict": {"nodes": "snodes", "snodes": "snodes", "leaf_proba": "leaf_proba"},
    "rf_predict_scores": {"leaf_proba": "leaf_proba"},
    "gnb_proba": {"theta": "theta", "inv_var": "inv_var", "cconst": "theta"},
    "linear_proba": {"W": "W", "b": "W"},
    "ensemble_vote": {"probas": "members"},
    "proba_smooth": {"state": "state", "held": "held", "n_live": "n_live"},
    "class_traffic": {"labels": "labels", "conf": "conf", "n_live": "n_live"},
    "svc_predict": {"SV": "dual", "dual": "intercept", "svclass": "svclass", "intercept": "intercept"},
    "svc_decision": {"SV": "dual", "dual": "intercept", "svclass": "svclass", "intercept": "intercept"},
    "svc_couple": {"probA": "probA", "probB": "probB"},
    "knn_topk": {"R": "ry", "ry": "ry"},
    "knn_topk_mfma": {"R": "ry", "ry": "ry", "cmean": "cmean"},
    "gnb_fit_stats": {"y": "y"},
    "logistic_grad": {"y": "y", "W": "b", "b": "b"},
    "flow_features": {"cur": "prev", "prev": "prev", "times": "times"},
    "smo_select": {"alpha": "alpha", "grad": "grad", "out": "out"},
    "smo_solve": {k: k for k in ("y", "alpha", "grad", "sel", "rows", "sol")},
    "smo_solve2": {k: k for k in ("y", "alpha", "grad", "sel", "rows", "sol")},
    "smo_update_dev": {k: k for k in ("y", "grad", "rows", "sol")},
    "smo_update": {k: k for k in ("y", "grad", "rows")},
    "smo_row": {k: k for k in ("sel", "sol", "krow")},
    "smo_select2": {k: k for k in ("alpha", "grad", "krow", "sel", "sol")},
    "smo_update_dev2": {k: k for k in ("y", "grad", "rows", "sol", "krow")},
    "rf_hist": {"y": "y", "nid": "nid", "fsel": "fsel"},
    "rf_split": {"fsel": "fsel"},
    "rf_level_compact": {"y": "y", "nid": "nid", "frank": "frank"},
    "rf_partition": {"nid": "nid", "feat": "feat", "binthr": "binthr"},
}

# Per op: the arguments whose dim() the binding checks (the rest are flat
# buffers: only their length matters to a kernel).
DIM = {
    "gnb_predict": ("X", "theta"), "linear_argmax": ("X", "W"), "kmeans_assign": ("X", "centers"),
    "rf_predict": ("X", "nodes", "snodes", "roots"), "rf_predict_scores": ("X", "nodes", "roots"),
    "gnb_proba": ("X",), "linear_proba": ("X",), "knn_vote_proba": ("idx",),
    "ensemble_vote": ("probas",), "proba_smooth": ("proba", "state", "held"),
    "class_traffic": ("X", "labels"), "svc_predict": ("X", "SV", "dual"),
    "svc_decision": ("X", "SV", "dual"), "svc_couple": ("dec",), "knn_topk": ("Q", "R"),
    "knn_topk_mfma": ("Q", "R"), "gnb_fit_stats": ("X",), "logistic_grad": ("X", "W"),
    "flow_features": ("cur", "prev", "times"), "smo_select": ("y",), "smo_solve": ("X",),
    "smo_solve2": ("X",), "smo_update_dev": ("X",), "smo_update": ("X",), "smo_row": ("X",),
    "smo_select2": ("y",), "smo_update_dev2": ("X",), "rf_hist": ("bins", "hist"),
    "rf_split": ("hist",), "rf_level_compact": ("bins",), "rf_partition": ("B",),
}

# Per op: (argument, value outside its range, what the message says).
COUNT = {
    "rf_predict": [("C", 17, "rf_predict"), ("C", 1, "rf_predict"), ("n_leaves", -1, "leaf_proba")],
    "rf_predict_scores": [("C", 9, "rf_predict_scores"), ("C", 1, "rf_predict_scores")],
    "gnb_proba": [("cconst", f64(30, 9), "2..8 classes"), ("cconst", f64(30, 1), "2..8 classes")],
    "linear_proba": [("b", f32(30, 9), "2..8 classes")],
    "knn_vote_proba": [("C", 9, "2..8 classes"), ("C", 1, "2..8 classes")],
    "ensemble_vote": [("C", 9, "2..8 classes"), ("weights", [0.5, 0.0], "weights"),
                      ("colmaps", [[0, 1, 2], [0, 3]], "column map")],
    "proba_smooth": [("alpha", 0.0, "alpha"), ("margin", -1.0, "margin"),
                     ("proba", torch.full((N, 9), 1 / 9), "2..8 classes")],
    "class_traffic": [("n_classes", 9, "no kernel for"), ("n_classes", 1, "no kernel for"),
                      ("min_conf", float("nan"), "min_conf")],
    "svc_predict": [("dual", f32(30, 6, 4), "2..6 classes")],
    "svc_decision": [("dual", f32(30, 6, 4), "2..6 classes")],
    "svc_couple": [("C", 7, "2..6 classes"), ("C", 1, "2..6 classes")],
    "knn_topk": [("k", 0, "knn_topk"), ("k", 33, "knn_topk"), ("k", 9, "no kernel for k = 9")],
    "knn_topk_mfma": [("k", 0, "knn_topk_mfma"), ("k", 9, "knn_topk_mfma"), ("C", 17, "knn_topk_mfma"),
                      ("R", torch.zeros(0, 12), r"\bR\b")],
    "gnb_fit_stats": [("C", 0, "gnb_fit_stats")],
    "logistic_grad": [("W", f64(30, 17, 12), "logistic_grad")],
    "rf_hist": [("hist", torch.zeros(2, 12, 256, 0, dtype=torch.int32), "hist")],
    "rf_split": [("hist", torch.zeros(2, 12, 256, 1, dtype=torch.int32), "rf_split"),
                 ("hist", torch.zeros(2, 12, 256, 9, dtype=torch.int32), "no kernel for 9 classes")],
    # fidx is (L,mf) for whatever mf its length gives: only a length that L
    # does not divide, or more than 12 slots, is wrong
    "rf_level_compact": [("L", 0, "rf_level_compact"), ("C", 1, "rf_level_compact"),
                         ("fidx", u8(0, 1, 0), "fidx"), ("fidx", torch.zeros(2, 13, dtype=torch.uint8), "fidx")],
}

OTHER_DTYPE = {torch.float32: torch.float64, torch.float64: torch.float32, torch.int32: torch.int64,
               torch.int64: torch.int32, torch.uint8: torch.int32}


def _mutate(kind, t):
    if isinstance(t, list):  # ensemble_vote's members: the second one
        return [t[0], _mutate(kind, t[1])]
    if kind == "dtype":
        return t.to(OTHER_DTYPE[t.dtype])
    if kind == "short":
        return t[:-1].contiguous()
    if kind == "dim":
        return t.unsqueeze(0)
    if kind == "strided":
        return torch.stack([t, t], dim=-1)[..., 0]
    return t  # "cpu": handled by _reject


def _tensor_args(op):
    for name, v in _args(op).items():
        if isinstance(v, torch.Tensor) or (isinstance(v, list) and isinstance(v[0], torch.Tensor)):
            yield name, v


def _cases():
    for op in OPS:
        for name, v in _tensor_args(op):
            blame = "member" if isinstance(v, list) else rf"\b{name}\b"
            yield op, name, "dtype", blame
            yield op, name, "cpu", blame
            if isinstance(v, list) or v.numel() > 1:  # one element is always contiguous
                yield op, name, "strided", blame
            if name in DIM[op]:
                yield op, name, "dim", blame
        for name, blame in SHORT.get(op, {}).items():
            yield op, name, "short", rf"\b{blame}\b"
        for i, (name, _, says) in enumerate(COUNT.get(op, [])):
            yield op, name, f"count{i}", says if "\\" in says else re.escape(says)


CASES = list(_cases())


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("op,name,kind,says", CASES, ids=[f"{o}-{n}-{k}" for o, n, k, _ in CASES])
def test_rejected_before_launch(op, name, kind, says):
    args = _args(op)
    moved = {k: _cuda(v) for k, v in args.items()}
    if kind.startswith("count"):
        moved[name] = _cuda(COUNT[op][int(kind[5:])][1])
    elif kind == "cpu":
        moved[name] = _mutate(kind, args[name])
        if isinstance(moved[name], list):
            moved[name] = [moved[name][0].cuda(), moved[name][1]]
    else:
        moved[name] = _mutate(kind, moved[name])
    with pytest.raises(RuntimeError, match=says):
        getattr(og._ext, op)(*moved.values())


def test_every_argument_a_kernel_indexes_has_a_rejection():
    """Each tensor argument of each op has a too-short case, in SHORT or in
    COUNT, unless it only defines a count."""
    defines = {"X", "Q", "B", "bins", "cur", "dec", "idx", "proba", "roots", "centers", "lmap", "hist"}
    free = {("knn_vote_proba", "y"),  # the kernel skips an index outside y
            ("rf_predict_scores", "nodes"),  # reached through the node links alone
            ("smo_select", "y"), ("smo_select2", "y")}  # y is what n is taken from
    for op in OPS:
        counted = {name for name, _, _ in COUNT.get(op, [])}
        for name, _ in _tensor_args(op):
            assert name in SHORT.get(op, {}) or name in counted or name in defines or (op, name) in free, (op, name)


# ----------------------------------------------------------------------
# the LDS bound of the three predict kernels whose LDS grows with a count
# ----------------------------------------------------------------------

# bytes per class or cluster, as the kernels lay their LDS out
LDS_PER_COUNT = {
    "gnb_predict": (2 * 12 + 1) * 4,  # theta, inv_var [C,12] and const [C], f32
    "linear_argmax": (12 + 1) * 4,  # W [C,12] and b [C], f32
    "kmeans_assign": (12 + 1) * 8 + 12 * 4,  # f64 sums [K,12], counts [K]; f32 centers [K,12]
}


def _lds_args(op, count):
    if op == "gnb_predict":
        return dict(X=X, theta=f32(40, count, 12), inv_var=f32(41, count, 12).abs() + 0.5,
                    cconst=f32(42, count))
    if op == "linear_argmax":
        return dict(X=X, W=f32(43, count, 12), b=f32(44, count))
    return dict(X=X, centers=f32(45, count, 12), want_update=True)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(LDS_PER_COUNT))
def test_lds_bound(op):
    bound = LDS_LIMIT // LDS_PER_COUNT[op]
    args = _lds_args(op, bound)
    out, _ = _call(op, args)
    if op == "gnb_predict":
        d = X.double()[:, None, :] - args["theta"].double()
        score = args["cconst"].double() - 0.5 * (d * d * args["inv_var"].double()).sum(-1)
    elif op == "linear_argmax":
        score = X.double() @ args["W"].double().T + args["b"].double()
    else:
        score = -torch.cdist(X.double(), args["centers"].double()).pow(2)
        out = out[0]
    top = score.topk(2, dim=1).values
    # the f32 kernels keep the f64 order where the two best are this far apart
    assert bool((top[:, 0] - top[:, 1] > 1e-4 * score.abs().max()).all())
    assert torch.equal(out.cpu().long(), score.argmax(1))
    assert int(score.argmax(1).max()) >= 12  # a class past what other tests reach
    with pytest.raises(RuntimeError, match=op):
        _call(op, _lds_args(op, bound + 1))


# ----------------------------------------------------------------------
# tensors on a device that is not the current one
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
def test_tensors_on_the_other_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    args = {k: v.to("cuda:1") for k, v in a_flow_features().items()}
    assert torch.cuda.current_device() == 0
    got = og._ext.flow_features(*args.values())
    with torch.cuda.device(1):
        ref = og._ext.flow_features(*args.values())
    assert got.device == ref.device == torch.device("cuda:1")
    assert torch.equal(got, ref)
    c_flow_features(got, a_flow_features())
