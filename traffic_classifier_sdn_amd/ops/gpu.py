"""GPU op bindings: hand-written CDNA4 HIP kernels (csrc/*.hip).

Every op the models call on CUDA tensors is bound here explicitly.  Hot ops
run the HIP kernels; a handful of cold diagnostic ops (decision functions,
seeding distances) deliberately alias the torch implementations — they are
not part of any benched path.  Import fails loudly when the extension is
missing (see ops.__init__)."""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import cpu as _cpu
from . import _tcsdn_hip as _ext  # type: ignore  # built by setup.py

# cold / diagnostic aliases (torch ops, not benched)
linear_logits = _cpu.linear_logits
gnb_joint_loglik = _cpu.gnb_joint_loglik
pairwise_sqdist = _cpu.pairwise_sqdist
rbf_kernel = _cpu.rbf_kernel
svc_ovo_decision = _cpu.svc_ovo_decision
svc_vote = _cpu.svc_vote
knn_vote = _cpu.knn_vote
rf_flatten = _cpu.rf_flatten


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


# Model parameters are fixed between fits, but a `.to(float32)` or a derived
# constant per predict call launches a kernel every time — inside the
# hipGraph-captured serve path that was ~9 stray elementwise kernels per
# replay.  The caches below keep such tensors keyed by source buffer address,
# and every entry holds a reference to its SOURCE tensors: torch's caching
# allocator reuses freed addresses, so a data_ptr key alone could serve a
# stale value after a model is freed and a same-shape tensor lands at the
# recycled address.  Pinning the sources keeps their addresses
# out of the free pool for the lifetime of the entry, which makes the key
# unambiguous (the models never mutate parameters in place).
def _cached(cache: dict, cap: int, key: tuple, sources: tuple, build) -> tuple:
    """The entry ``(*sources, *build())`` of ``cache`` under ``key``, built on
    a miss; a cache past ``cap`` entries is cleared first."""
    ent = cache.get(key)
    if ent is None:
        if len(cache) > cap:
            cache.clear()
        ent = (*sources, *build())
        cache[key] = ent
    return ent


# entry = (source, f32 copy)
_cast_cache: Dict[Tuple[int, int, torch.dtype], Tuple[torch.Tensor, torch.Tensor]] = {}


def _f32_cached(t: torch.Tensor) -> torch.Tensor:
    if t.dtype == torch.float32 and t.is_contiguous():
        return t
    key = (t.data_ptr(), t.numel(), t.dtype)
    return _cached(_cast_cache, 64, key, (t,), lambda: (_f32(t),))[1]


def _f64(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float64).contiguous()


# ----------------------------------------------------------------------
# predict ops
# ----------------------------------------------------------------------


def linear_argmax(X: torch.Tensor, coef: torch.Tensor, intercept: torch.Tensor) -> torch.Tensor:
    if X.shape[1] != 12:  # HIP kernels are specialised for the 12-feature
        return _cpu.linear_argmax(X, coef, intercept)  # schema; torch ops run
    return _ext.linear_argmax(_f32(X), _f32_cached(coef), _f32_cached(intercept))


# entry = (var, prior, theta32, inv_var, const32)
_gnb_cache: Dict[Tuple[int, int], Tuple[torch.Tensor, ...]] = {}


def _gnb_consts(var: torch.Tensor, class_prior: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(1 / var, log prior - 0.5 * sum log(2 pi var)), both f64."""
    var64 = var.double()
    const = torch.log(class_prior.double()) - 0.5 * torch.log(2.0 * torch.pi * var64).sum(dim=1)
    return (1.0 / var64).contiguous(), const.contiguous()


def gnb_argmax(
    X: torch.Tensor, theta: torch.Tensor, var: torch.Tensor, class_prior: torch.Tensor
) -> torch.Tensor:
    # per-class constants derived in f64 for stability, cached per model so
    # the serve path replays no derivation kernels
    if X.shape[1] != 12:
        return _cpu.gnb_argmax(X, theta, var, class_prior)
    key = (var.data_ptr(), class_prior.data_ptr())
    ent = _cached(
        _gnb_cache, 32, key, (var, class_prior),
        lambda: (_f32(theta), *(t.float() for t in _gnb_consts(var, class_prior))),
    )
    return _ext.gnb_predict(_f32(X), *ent[2:])


def kmeans_assign(
    X: torch.Tensor, centers: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    if X.shape[1] != 12:
        return _cpu.kmeans_assign(X, centers)
    labels, counts, sums, inertia = _ext.kmeans_assign(_f32(X), _f32(centers), True)
    dt = X.dtype if X.dtype in (torch.float32, torch.float64) else torch.float32
    return labels, counts.to(dt), sums.to(dt), inertia[0].to(dt)


# MFMA path cutover: below this reference-set size the scalar kernel's
# launch simplicity wins; above it the v_mfma_f32_32x32x2_f32 distance
# GEMM dominates (csrc/knn_mfma.hip)
_KNN_MFMA_MIN_ROWS = 100_000
# entry = (R, cmean)
_knn_cmean_cache: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}


def _knn_cmean(R: torch.Tensor) -> torch.Tensor:
    """Reference column means (centering makes the expanded-form distance
    cancellation-safe); cached per reference buffer."""
    key = (R.data_ptr(), R.shape[0])
    return _cached(_knn_cmean_cache, 16, key, (R,), lambda: (R.mean(dim=0).float().contiguous(),))[1]


def _knn_shards(nr: int) -> int:
    # enough (query-block x shard) workgroups to fill 256 CUs at 2 WG/CU,
    # with shards of at least ~256K rows to amortize seeding
    return max(1, min(64, nr // 262_144))


def knn_topk(Q: torch.Tensor, R: torch.Tensor, k: int, approx: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    if Q.shape[1] != 12:
        return _cpu.knn_topk(Q, R, k)
    Qf, Rf = _f32(Q), _f32(R)
    if (approx or R.shape[0] >= _KNN_MFMA_MIN_ROWS) and k <= 8:
        dist, idx = _ext.knn_topk_mfma(
            Qf, Rf, _knn_cmean(Rf), None, k, 0, 0, _knn_shards(R.shape[0]),
            1 if approx else 0,
        )
        return dist, idx
    dist, idx = _ext.knn_topk(Qf, Rf, None, k, 0, 0)
    return dist, idx


def knn_classify(
    Q: torch.Tensor, R: torch.Tensor, y: torch.Tensor, k: int, n_classes: int,
    idx_base: int = 0, approx: bool = False
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Fused top-k + uniform vote (labels also returned for sharded merge).

    ``approx=True`` selects the bf16 coarse-pass kernel: 16x the f32 MFMA
    rate, exact-f32 refine over a 16-candidate pool per query (measured
    recall, not proven — see csrc/knn_mfma.hip)."""
    if Q.shape[1] != 12:
        return _cpu.knn_classify(Q, R, y, k, n_classes, idx_base)
    y8 = y.to(torch.uint8).contiguous()
    Qf, Rf = _f32(Q), _f32(R)
    if (approx or R.shape[0] >= _KNN_MFMA_MIN_ROWS) and k <= 8 and n_classes <= 16:
        dist, idx, lab = _ext.knn_topk_mfma(
            Qf, Rf, _knn_cmean(Rf), y8, k, n_classes, idx_base,
            _knn_shards(R.shape[0]), 1 if approx else 0
        )
        return dist, idx, lab
    dist, idx, lab = _ext.knn_topk(Qf, Rf, y8, k, n_classes, idx_base)
    return dist, idx, lab


def _svc_args(X, SV, dual_coef, intercept, n_support, gamma, svclass):
    """The arguments of the extension's svc_predict and svc_decision."""
    if svclass is None:
        # the class of every support vector: static per model; callers on the
        # hipGraph path precompute it (repeat_interleave is not stream-capture
        # safe)
        svclass = torch.repeat_interleave(
            torch.arange(n_support.numel(), device=X.device), n_support.to(X.device)
        ).to(torch.uint8)
    return (
        _f32(X), _f32_cached(SV), _f32_cached(dual_coef), svclass.contiguous(),
        _f32_cached(intercept), float(gamma),
    )


def svc_predict(
    X: torch.Tensor,
    SV: torch.Tensor,
    dual_coef: torch.Tensor,
    intercept: torch.Tensor,
    n_support: torch.Tensor,
    gamma: float,
    svclass: torch.Tensor = None,
) -> torch.Tensor:
    if X.shape[1] != 12:
        return _cpu.svc_predict(X, SV, dual_coef, intercept, n_support, gamma, svclass)
    return _ext.svc_predict(*_svc_args(X, SV, dual_coef, intercept, n_support, gamma, svclass))


# ----------------------------------------------------------------------
# SVC class probabilities (csrc/svc_kernels.hip)
# ----------------------------------------------------------------------

platt_fit = _cpu.platt_fit  # cold: a fit-time Newton iteration on the host


def svc_decision(
    X: torch.Tensor,
    SV: torch.Tensor,
    dual_coef: torch.Tensor,
    intercept: torch.Tensor,
    n_support: torch.Tensor,
    gamma: float,
    svclass: torch.Tensor = None,
) -> torch.Tensor:
    """f64 [n, C(C-1)/2] one-vs-one decision values, accumulated exactly as
    ``svc_predict`` accumulates them, so their signs give its votes."""
    if X.shape[1] != 12:
        return _cpu.svc_decision(X, SV, dual_coef, intercept, n_support, gamma, svclass)
    return _ext.svc_decision(*_svc_args(X, SV, dual_coef, intercept, n_support, gamma, svclass))


def svc_couple(
    dec: torch.Tensor, probA: torch.Tensor, probB: torch.Tensor, n_classes: int
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(proba[n,C] f32, idx[n] int32, conf[n] f32): Platt sigmoids of the
    decision values coupled as libsvm couples them, the one-vs-one vote of
    the same decisions, and the coupled probability of the voted class.
    A CalibratedSVC keeps its sigmoids as f64 device tensors, so nothing is
    converted or copied here and a captured graph replays the kernel alone."""
    return _ext.svc_couple(
        _f64(dec), _f64(probA.to(dec.device)), _f64(probB.to(dec.device)), int(n_classes)
    )


def rf_hist(bins: torch.Tensor, y: torch.Tensor, nid: torch.Tensor, n_nodes: int,
            n_classes: int, fsel: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-node per-feature class histograms.  With ``fsel`` (u8
    [n_nodes,12] mtry mask) only the selected feature planes are scattered
    — 3 atomics per row instead of 12 at sklearn's max_features=3; the
    unselected planes stay zero and must not be read."""
    if bins.shape[1] != 12:  # HIP kernel is specialised for the 12-feature schema
        return _cpu.rf_hist(bins, y, nid, n_nodes, n_classes)
    hist = torch.zeros(n_nodes, 12, 256, n_classes, dtype=torch.int32, device=bins.device)
    _ext.rf_hist(bins.contiguous(), y.contiguous(), nid.contiguous(), hist,
                 None if fsel is None else fsel.contiguous())
    return hist


def rf_pack(forest: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    """Pack the SoA forest (ops.cpu.rf_flatten layout) into the traversal
    kernels' uint2 node tables.

    ``nodes`` (row-per-lane and wave-per-row kernels), n_nodes entries:
      word0 = f32 threshold bits (inner) | leaf-probability row (mixed leaf)
      word1 = (right_child_GLOBAL << 8) | feature byte
    Feature byte: 0..0xef = inner-node feature id; 0xf0|class = PURE leaf
    (one-hot distribution, counted in-register by the kernels); 0xff = mixed
    leaf (distribution row in word0).

    ``snodes`` (streaming kernel), n_nodes + 2 entries:
      word0 = f32 threshold bits (inner) | 0 (pure leaf) |
              leaf-probability row + 1 (mixed leaf)
      word1 = (link_GLOBAL << 8) | byte
    The link is the right child for an inner node and the NEXT TREE'S ROOT
    for a leaf; after the last tree it is ``n_nodes``, the terminal value.
    Byte: 0..0x7f = inner-node feature id; 0x80 | flag << 6 | shift = leaf,
    where shift is 10 * class for a pure leaf, 61 for a mixed one and 60 for
    neither (the kernel adds 1 << shift to its packed vote register, whose
    bits 60..63 belong to no class), and flag marks the leaves of the trees
    after which the kernel runs its majority test: t & 7 == 7 once
    2t + 2 >= T (before that leader - runner-up <= t + 1 cannot exceed the
    T - 1 - t trees left), and the last tree.  Entry n_nodes is a flagged
    leaf linked to itself, which ends any row that gets there; entry
    n_nodes + 1 is the PARK node the kernel's idle lanes spin on: an inner
    node with feature id 12 (no such feature: the kernel's slot 12 holds
    NaN, so the step goes right) whose right child is itself.

    The kernels count pure leaves in 10-bit fields of one 64-bit register,
    which holds 6 classes and 1023 trees; a forest beyond either gets no
    pure leaves in either table.

    The streaming kernel walks one strictly increasing chain of node
    indices per row, from the first root to the terminal value, so the
    order is checked here: ``ValueError`` unless every right child lies
    after its parent inside the same tree and every next-root after its
    leaf.
    """
    thr = forest["threshold"].cpu()
    right = forest["right"].cpu().to(torch.int64)
    feat = forest["feature"].cpu().to(torch.int64)
    leaf_index = forest["leaf_index"].cpu().to(torch.int64)
    offsets = forest["tree_offset"].cpu().to(torch.int64)
    n_nodes = thr.numel()
    n_trees = offsets.numel() - 1
    n_classes = int(forest["n_classes"])
    counts = offsets[1:] - offsets[:-1]
    if int(offsets[0]) != 0 or int(offsets[-1]) != n_nodes or bool((counts < 1).any()):
        raise ValueError("tree_offset must rise from 0 to n_nodes, one or more nodes per tree")
    if n_nodes + 2 >= 1 << 24:
        raise ValueError("packed node format holds at most 2^24 - 3 nodes")
    base = torch.repeat_interleave(offsets[:-1], counts)
    next_root = torch.repeat_interleave(offsets[1:], counts)
    tree = torch.repeat_interleave(torch.arange(n_trees, dtype=torch.int64), counts)
    index = torch.arange(n_nodes, dtype=torch.int64)
    is_leaf = feat < 0
    if bool((feat[~is_leaf] > 0x7F).any()):
        raise ValueError("feature ids above 0x7f do not fit the packed node")
    right_global = right + base
    inner_ok = (right_global > index) & (right_global < next_root)
    if not bool(inner_ok[~is_leaf].all()):
        raise ValueError("right child must lie after its parent, inside the same tree")
    if not bool((next_root > index).all()) or (n_nodes and int(next_root[-1]) != n_nodes):
        raise ValueError("next-root chain must increase and end at n_nodes")
    probs = forest["leaf_proba"].cpu()
    # pure leaf: exactly one class carries the whole mass
    pmax, pcls = probs.max(dim=1)
    leaf_pure = torch.zeros_like(is_leaf)
    leaf_cls = torch.zeros_like(feat)
    valid = leaf_index >= 0
    if n_classes * 10 <= 64 and n_trees <= 1023:  # else the vote fields overflow
        leaf_pure[valid] = pmax[leaf_index[valid]] >= 1.0
    leaf_cls[valid] = pcls[leaf_index[valid]].to(torch.int64)
    thr_bits = thr.view(torch.int32).to(torch.int64)
    w0 = torch.where(is_leaf, leaf_index, thr_bits).to(torch.int32)
    leaf_byte = torch.where(leaf_pure, 0xF0 | leaf_cls, torch.tensor(0xFF, dtype=torch.int64))
    w1 = torch.where(is_leaf, leaf_byte, (right_global << 8) | feat).to(torch.int32)
    nodes = torch.stack([w0, w1], dim=1).contiguous()

    tested = (((tree & 7) == 7) & (2 * tree + 2 >= n_trees)) | (tree == n_trees - 1)
    shift = torch.where(leaf_pure, 10 * leaf_cls, torch.tensor(61, dtype=torch.int64))
    s_byte = 0x80 | (tested.to(torch.int64) << 6) | shift
    zero = torch.zeros_like(leaf_index)
    s0 = torch.where(is_leaf, torch.where(leaf_pure, zero, leaf_index + 1), thr_bits)
    s1 = torch.where(is_leaf, (next_root << 8) | s_byte, (right_global << 8) | feat)
    end = torch.tensor([[0, (n_nodes << 8) | 0x80 | 0x40 | 60]], dtype=torch.int64)
    park = torch.tensor([[0, ((n_nodes + 1) << 8) | 12]], dtype=torch.int64)
    snodes = torch.cat([torch.stack([s0, s1], dim=1), end, park]).to(torch.int32).contiguous()
    return {
        "nodes": nodes.to(device),
        "snodes": snodes.to(device),
        "roots": offsets[:-1].to(torch.int32).to(device),
        "leaf_proba": forest["leaf_proba"].to(torch.float32).to(device).contiguous(),
        "n_leaves": int(forest["leaf_proba"].shape[0]),
        "n_classes": n_classes,
    }


def _rf_packed(X: torch.Tensor, forest: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The forest's packed tables on X's device, cached in the forest dict."""
    packed = forest.get("_packed")
    if packed is None or packed["nodes"].device != X.device:
        packed = rf_pack(forest, X.device)
        forest["_packed"] = packed
    return packed


def rf_argmax(X: torch.Tensor, forest: Dict[str, torch.Tensor]) -> torch.Tensor:
    packed = _rf_packed(X, forest)
    return _ext.rf_predict(
        _f32(X),
        packed["nodes"],
        packed["snodes"],
        packed["roots"],
        packed["leaf_proba"],
        packed["n_leaves"],
        packed["n_classes"],
    )


def rf_predict_scores(
    X: torch.Tensor, forest: Dict[str, torch.Tensor], want_proba: bool = True
) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """(proba[n,C] f32 | None, labels[n] int32, conf[n] f32) from the scores
    kernels (csrc/rf_proba_kernels.hip): every tree counts, labels are the
    first-maximum argmax of the class sums and conf is the top probability.
    ``want_proba=False`` skips the proba store (the serve path)."""
    if X.shape[1] != 12:
        return _cpu.rf_predict_scores(X, forest, want_proba)
    packed = _rf_packed(X, forest)
    if not 2 <= packed["n_classes"] <= 8:  # the kernels' class range
        return _cpu.rf_predict_scores(X, forest, want_proba)
    proba, labels, conf = _ext.rf_predict_scores(
        _f32(X),
        packed["nodes"],
        packed["roots"],
        packed["leaf_proba"],
        packed["n_leaves"],
        packed["n_classes"],
        want_proba,
    )
    return (proba if want_proba else None), labels, conf


def rf_predict_proba(X: torch.Tensor, forest: Dict[str, torch.Tensor]) -> torch.Tensor:
    return rf_predict_scores(X, forest)[0]


# ----------------------------------------------------------------------
# forest feature contributions (csrc/rf_explain_kernels.hip)
# ----------------------------------------------------------------------

rf_explain_flatten = _cpu.rf_explain_flatten
rf_explain_check = _cpu.rf_explain_check


def _rf_explain_delta(X: torch.Tensor, tables: Dict[str, object]) -> torch.Tensor:
    """The delta table on X's device, cached in the tables dict."""
    delta = tables.get("_delta")
    if delta is None or delta.device != X.device:
        delta = tables["_delta"] = tables["delta"].to(X.device).contiguous()
    return delta


def rf_explain(
    X: torch.Tensor,
    forest: Dict[str, torch.Tensor],
    tables: Dict[str, object],
    labels: torch.Tensor,
    want_matrix: bool = True,
    want_sums: bool = False,
) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    # no cast and no copy: the captured serve pass hands its own buffers over
    T, C = _cpu.rf_explain_check(X, forest, tables, labels)
    if X.shape[1] != 12 or not 2 <= C <= 8:  # the kernels' schema and class range
        return _cpu.rf_explain(X, forest, tables, labels, want_matrix, want_sums)
    if T > _cpu.RF_EXPLAIN_MAX_TREES:
        raise ValueError(f"the forest explain kernels take at most 4096 trees, got {T}")
    packed = _rf_packed(X, forest)
    contrib, why, why_value, sums = _ext.explain.rf_explain(
        X, packed["nodes"], packed["roots"], _rf_explain_delta(X, tables), labels,
        bool(want_matrix), bool(want_sums),
    )
    return (contrib if want_matrix else None), why, why_value, (sums if want_sums else None)


# ----------------------------------------------------------------------
# isolation forest novelty score (csrc/iforest_kernels.hip)
# ----------------------------------------------------------------------

iforest_c = _cpu.iforest_c
iforest_flatten = _cpu.iforest_flatten
iforest_pack = _cpu.iforest_pack
iforest_consts = _cpu.iforest_consts
iforest_depth_cut = _cpu.iforest_depth_cut
iforest_score_check = _cpu.iforest_score_check
iforest_leaves = _cpu.iforest_leaves  # cold: the parity tests' per-tree leaves


def _iforest_packed(X: torch.Tensor, forest: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The isolation forest's packed tables on X's device, cached in the
    forest dict."""
    packed = forest.get("_packed")
    if packed is None or packed["nodes"].device != X.device:
        packed = iforest_pack(forest, X.device)
        forest["_packed"] = packed
    return packed


def iforest_score(
    X: torch.Tensor,
    forest: Dict[str, torch.Tensor],
    threshold: Optional[float] = None,
    labels: Optional[torch.Tensor] = None,
    want_sum: bool = False,
) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    # no cast and no copy: the captured serve pass hands its own buffers over
    depth_cut = _cpu.iforest_score_check(X, forest, threshold, labels)
    if not X.is_cuda:
        raise ValueError("the isolation forest kernels take GPU tensors, got a CPU tensor")
    packed = _iforest_packed(X, forest)
    score, flags, labels_out, psum = _ext.novelty.iforest_score(
        X, packed["nodes"], packed["roots"], labels, packed["inv_denom"], depth_cut,
        bool(want_sum),
    )
    return score, flags, (labels_out if labels is not None else None), (psum if want_sum else None)


# ----------------------------------------------------------------------
# class probabilities and the soft vote (csrc/ensemble_kernels.hip)
# ----------------------------------------------------------------------

ensemble_weights = _cpu.ensemble_weights
ensemble_check = _cpu.ensemble_check

# entry = (theta, var, prior, theta64, inv_var64, const64)
_gnb_proba_cache: Dict[Tuple[int, int, int], Tuple[torch.Tensor, ...]] = {}


def gnb_proba(
    X: torch.Tensor, theta: torch.Tensor, var: torch.Tensor, class_prior: torch.Tensor
) -> torch.Tensor:
    if X.shape[1] != 12:
        return _cpu.gnb_proba(X, theta, var, class_prior)
    key = (theta.data_ptr(), var.data_ptr(), class_prior.data_ptr())
    ent = _cached(
        _gnb_proba_cache, 32, key, (theta, var, class_prior),
        lambda: (_f64(theta), *_gnb_consts(var, class_prior)),
    )
    return _ext.gnb_proba(_f32(X), *ent[3:])


def linear_proba(X: torch.Tensor, coef: torch.Tensor, intercept: torch.Tensor) -> torch.Tensor:
    if X.shape[1] != 12:
        return _cpu.linear_proba(X, coef, intercept)
    return _ext.linear_proba(_f32(X), _f32_cached(coef), _f32_cached(intercept))


# entry = (y, y8)
_knn_y8_cache: Dict[Tuple[int, int, torch.dtype], Tuple[torch.Tensor, torch.Tensor]] = {}


def knn_vote_proba(idx: torch.Tensor, y: torch.Tensor, n_classes: int) -> torch.Tensor:
    y8 = y
    if y.dtype != torch.uint8 or not y.is_contiguous():
        key = (y.data_ptr(), y.numel(), y.dtype)
        y8 = _cached(_knn_y8_cache, 16, key, (y,), lambda: (y.to(torch.uint8).contiguous(),))[1]
    return _ext.knn_vote_proba(idx.to(torch.int32).contiguous(), y8, int(n_classes))


def ensemble_vote(
    probas, colmaps, weights, n_classes: int, want_proba: bool = True
) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    w32 = _cpu.ensemble_check(probas, colmaps, weights, n_classes)
    avg, labels, conf = _ext.ensemble_vote(
        [_f32(p) for p in probas], [[int(c) for c in m] for m in colmaps], w32,
        int(n_classes), bool(want_proba),
    )
    return (avg if want_proba else None), labels, conf


proba_smooth_check = _cpu.proba_smooth_check


def proba_smooth(
    proba: torch.Tensor,
    state: torch.Tensor,
    held: torch.Tensor,
    alpha: float,
    margin: float = 0.0,
    n_live: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    # no cast and no copy here: state and held are updated in place, so a
    # wrong dtype or layout is an error, not something to convert
    a, _, m = _cpu.proba_smooth_check(proba, state, held, alpha, margin, n_live)
    labels, conf = _ext.proba_smooth(proba, state, held, n_live, a, m)
    return labels, conf


class_traffic_check = _cpu.class_traffic_check
TRAFFIC_COLUMNS = _cpu.TRAFFIC_COLUMNS


def class_traffic(
    X: torch.Tensor,
    labels: torch.Tensor,
    n_classes: int,
    conf: Optional[torch.Tensor] = None,
    min_conf: float = 0.0,
    n_live: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    # no cast and no copy: the captured serve pass hands its own buffers over
    C, mc = _cpu.class_traffic_check(X, labels, n_classes, conf, min_conf, n_live)
    return _ext.class_traffic(X, labels, C, conf, mc, n_live)


class_top_flows_check = _cpu.class_top_flows_check
top_flow_columns_check = _cpu.top_flow_columns_check
top_flows_k_check = _cpu.top_flows_k_check
TOP_FLOW_COLUMNS = _cpu.TOP_FLOW_COLUMNS


def class_top_flows(
    X: torch.Tensor,
    labels: torch.Tensor,
    n_classes: int,
    k: int,
    columns=TOP_FLOW_COLUMNS,
    conf: Optional[torch.Tensor] = None,
    min_conf: float = 0.0,
    n_live: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    # no cast and no copy, as in class_traffic
    C, k, _, mask, mc = _cpu.class_top_flows_check(
        X, labels, n_classes, k, columns, conf, min_conf, n_live
    )
    rows, keys = _ext.selection.class_top_flows(X, labels, C, k, mask, conf, mc, n_live)
    return rows, keys


# ----------------------------------------------------------------------
# fit ops
# ----------------------------------------------------------------------


def gnb_fit_stats(
    X: torch.Tensor, y: torch.Tensor, n_classes: int
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    if X.shape[1] != 12:
        return _cpu.gnb_fit_stats(X, y, n_classes)
    count, s, sq = _ext.gnb_fit_stats(_f64(X), y.to(torch.int64).contiguous(), n_classes)
    return count.to(X.dtype), s.to(X.dtype), sq.to(X.dtype)


def logistic_loss_grad(
    X: torch.Tensor,
    y: torch.Tensor,
    coef: torch.Tensor,
    intercept: torch.Tensor,
    l2: float = 1.0,
    sample_range=None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    if X.shape[1] != 12:  # e.g. the PCA-projection fit in analysis.py
        return _cpu.logistic_loss_grad(X, y, coef, intercept, l2=l2)
    grad, loss = _ext.logistic_grad(
        _f64(X), y.to(torch.int64).contiguous(), _f64(coef), _f64(intercept)
    )
    loss = loss[0] + 0.5 * l2 * (coef.double() * coef.double()).sum()
    g_coef = grad[:, :12] + l2 * coef.double()
    g_b = grad[:, 12]
    return loss.to(X.dtype), g_coef.to(X.dtype), g_b.to(X.dtype)


def flow_features(cur: torch.Tensor, prev: torch.Tensor, times: torch.Tensor) -> torch.Tensor:
    return _ext.flow_features(_f64(cur), _f64(prev), _f64(times))


def kmeans_labels(X: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    if X.shape[1] != 12:
        return _cpu.kmeans_labels(X, centers)
    labels, _, _, _ = _ext.kmeans_assign(_f32(X), _f32_cached(centers), False)
    return labels
