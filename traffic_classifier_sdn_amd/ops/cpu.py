"""CPU reference implementations of every compute op.

These are the numerics oracles for the CDNA4 HIP kernels (tests compare the
GPU path against these on identical inputs) and the execution path when no
GPU is present.  Everything is plain PyTorch/numpy; semantics mirror the
sklearn 1.0.1 native kernels the reference's compute ran on (SURVEY.md §2.2
N1-N6), e.g. tie-breaking is always "first maximum".
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ..utils.schema import FEATURE_NAMES as _FEATURE_NAMES


# ----------------------------------------------------------------------
# Linear / logistic (N1)
# ----------------------------------------------------------------------


def linear_logits(X: torch.Tensor, coef: torch.Tensor, intercept: torch.Tensor) -> torch.Tensor:
    """logits[n,c] = X @ coef^T + intercept  (reference sklearn
    LogisticRegression.decision_function)."""
    return X @ coef.T.to(X.dtype) + intercept.to(X.dtype)


def linear_argmax(X: torch.Tensor, coef: torch.Tensor, intercept: torch.Tensor) -> torch.Tensor:
    return torch.argmax(linear_logits(X, coef, intercept), dim=1).to(torch.int32)


def logistic_loss_grad(
    X: torch.Tensor,
    y: torch.Tensor,
    coef: torch.Tensor,
    intercept: torch.Tensor,
    l2: float = 1.0,
    sample_range: Optional[Tuple[int, int]] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Full-batch multinomial logistic loss + gradients (sklearn's lbfgs
    objective: mean CE * n + 0.5*l2*||coef||^2, gradient in the same scale).

    Returns (loss_scalar, grad_coef[C,F], grad_intercept[C]).
    """
    logits = linear_logits(X, coef, intercept)
    logp = torch.log_softmax(logits, dim=1)
    n = X.shape[0]
    nll = -logp[torch.arange(n, device=X.device), y].sum()
    loss = nll + 0.5 * l2 * (coef * coef).sum()
    p = torch.exp(logp)
    p[torch.arange(n, device=X.device), y] -= 1.0
    grad_coef = p.T @ X + l2 * coef
    grad_intercept = p.sum(dim=0)
    return loss, grad_coef, grad_intercept


# ----------------------------------------------------------------------
# Gaussian NB (N5)
# ----------------------------------------------------------------------


def gnb_joint_loglik(
    X: torch.Tensor, theta: torch.Tensor, var: torch.Tensor, class_prior: torch.Tensor
) -> torch.Tensor:
    """Per-class joint log-likelihood (sklearn GaussianNB._joint_log_likelihood)."""
    theta = theta.to(X.dtype)
    var = var.to(X.dtype)
    class_prior = class_prior.to(X.dtype)
    # const[c] = log prior[c] - 0.5 * sum_j log(2*pi*var[c,j])
    const = torch.log(class_prior) - 0.5 * torch.log(2.0 * torch.pi * var).sum(dim=1)
    # quad[n,c] = -0.5 * sum_j (x[n,j]-theta[c,j])^2 / var[c,j]
    diff = X.unsqueeze(1) - theta.unsqueeze(0)  # (n, C, F)
    quad = -0.5 * (diff * diff / var.unsqueeze(0)).sum(dim=2)
    return quad + const


def gnb_argmax(
    X: torch.Tensor, theta: torch.Tensor, var: torch.Tensor, class_prior: torch.Tensor
) -> torch.Tensor:
    return torch.argmax(gnb_joint_loglik(X, theta, var, class_prior), dim=1).to(torch.int32)


def gnb_fit_stats(
    X: torch.Tensor, y: torch.Tensor, n_classes: int
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per-class sufficient statistics (count, sum, sum-of-squares)."""
    F = X.shape[1]
    count = torch.zeros(n_classes, dtype=X.dtype, device=X.device)
    s = torch.zeros(n_classes, F, dtype=X.dtype, device=X.device)
    sq = torch.zeros(n_classes, F, dtype=X.dtype, device=X.device)
    count.index_add_(0, y, torch.ones_like(y, dtype=X.dtype))
    s.index_add_(0, y, X)
    sq.index_add_(0, y, X * X)
    return count, s, sq


# ----------------------------------------------------------------------
# KMeans (N6)
# ----------------------------------------------------------------------


def pairwise_sqdist(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """||a-b||^2 via the expanded form (the GEMM-shaped formulation the MFMA
    kernel uses); clamped at 0 for numerical safety."""
    an = (A * A).sum(dim=1, keepdim=True)
    bn = (B * B).sum(dim=1, keepdim=True).T
    d = an + bn - 2.0 * (A @ B.T)
    return torch.clamp(d, min=0.0)


def kmeans_assign(
    X: torch.Tensor, centers: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Lloyd assignment step. Returns (labels, counts[K], sums[K,F], inertia)."""
    centers = centers.to(X.dtype)
    d = pairwise_sqdist(X, centers)
    dmin, labels = torch.min(d, dim=1)
    K, F = centers.shape
    counts = torch.zeros(K, dtype=X.dtype, device=X.device)
    sums = torch.zeros(K, F, dtype=X.dtype, device=X.device)
    counts.index_add_(0, labels, torch.ones_like(dmin))
    sums.index_add_(0, labels, X)
    return labels.to(torch.int32), counts, sums, dmin.sum()


# ----------------------------------------------------------------------
# KNN (N3)
# ----------------------------------------------------------------------


def knn_topk(Q: torch.Tensor, R: torch.Tensor, k: int, approx: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    # approx is a GPU-path option (bf16 coarse pass); the CPU oracle is exact
    """Brute-force k smallest squared distances. Returns (dist[nq,k], idx[nq,k]),
    sorted ascending (ties by lower index, matching sklearn's ordering)."""
    d = pairwise_sqdist(Q, R)
    dist, idx = torch.topk(d, k, dim=1, largest=False, sorted=True)
    return dist, idx


def knn_classify(
    Q: torch.Tensor, R: torch.Tensor, y: torch.Tensor, k: int, n_classes: int, idx_base: int = 0
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Fused top-k + uniform vote (CPU oracle for the fused GPU kernel)."""
    dist, idx = knn_topk(Q, R, k)
    lab = knn_vote(idx, y.long(), n_classes)
    return dist, idx + idx_base, lab


def knn_vote(idx: torch.Tensor, y: torch.Tensor, n_classes: int) -> torch.Tensor:
    """Uniform-weight majority vote; ties -> lowest class index (sklearn mode)."""
    labels = y[idx]  # (nq, k)
    counts = torch.zeros(idx.shape[0], n_classes, dtype=torch.int32, device=idx.device)
    counts.scatter_add_(1, labels.long(), torch.ones_like(labels, dtype=torch.int32))
    return torch.argmax(counts, dim=1).to(torch.int32)


def rf_hist(bins: torch.Tensor, y: torch.Tensor, nid: torch.Tensor, n_nodes: int, n_classes: int) -> torch.Tensor:
    """Per-node per-feature class histograms for the level-synchronous tree
    builder: hist[node, f, bin, class] = #rows of that class with that bin.
    Rows with nid < 0 (finalised) are skipped.  CPU oracle of the HIP
    scatter kernel (csrc rf_hist_kernel)."""
    F = bins.shape[1]
    mask = nid >= 0
    b = bins[mask].long()
    yv = y[mask].long()
    nd = nid[mask].long()
    feats = torch.arange(F, dtype=torch.long, device=bins.device)
    codes = ((nd.unsqueeze(1) * F + feats) * 256 + b) * n_classes + yv.unsqueeze(1)
    hist = torch.bincount(codes.reshape(-1), minlength=n_nodes * F * 256 * n_classes)
    return hist.reshape(n_nodes, F, 256, n_classes).to(torch.int32)


# ----------------------------------------------------------------------
# SVC RBF OVO (N2)
# ----------------------------------------------------------------------


def rbf_kernel(X: torch.Tensor, SV: torch.Tensor, gamma: float) -> torch.Tensor:
    return torch.exp(-gamma * pairwise_sqdist(X, SV))


def svc_ovo_decision(
    K: torch.Tensor,
    dual_coef: torch.Tensor,
    intercept: torch.Tensor,
    n_support: torch.Tensor,
) -> torch.Tensor:
    """libsvm one-vs-one decision values from a kernel matrix.

    ``dual_coef`` is (C-1, n_SV) in libsvm layout; SVs are grouped by class
    (sizes ``n_support``).  Pair p=(i,j), i<j:
      dec[p] = sum_{sv in class i} dual_coef[j-1, sv] * K[:, sv]
             + sum_{sv in class j} dual_coef[i,   sv] * K[:, sv] + intercept[p]
    """
    C = int(n_support.numel())
    starts = torch.zeros(C + 1, dtype=torch.long)
    starts[1:] = torch.cumsum(n_support.cpu(), dim=0)
    # acc[n, c, o] = sum over SVs of class c of dual_coef[o', sv] * K[n, sv]
    # with o' = o for o < c else o-1  (the 30-accumulator form the HIP kernel
    # uses)
    n = K.shape[0]
    decs = []
    p = 0
    for i in range(C):
        for j in range(i + 1, C):
            si, ei = int(starts[i]), int(starts[i + 1])
            sj, ej = int(starts[j]), int(starts[j + 1])
            d = (
                K[:, si:ei] @ dual_coef[j - 1, si:ei]
                + K[:, sj:ej] @ dual_coef[i, sj:ej]
                + intercept[p]
            )
            decs.append(d)
            p += 1
    return torch.stack(decs, dim=1)  # (n, C*(C-1)/2)


def svc_vote(dec: torch.Tensor, n_classes: int) -> torch.Tensor:
    """libsvm majority vote over OVO decisions; ties -> first max."""
    n = dec.shape[0]
    votes = torch.zeros(n, n_classes, dtype=torch.int32, device=dec.device)
    p = 0
    for i in range(n_classes):
        for j in range(i + 1, n_classes):
            win_i = dec[:, p] > 0
            votes[:, i] += win_i.to(torch.int32)
            votes[:, j] += (~win_i).to(torch.int32)
            p += 1
    return torch.argmax(votes, dim=1).to(torch.int32)


def svc_predict(
    X: torch.Tensor,
    SV: torch.Tensor,
    dual_coef: torch.Tensor,
    intercept: torch.Tensor,
    n_support: torch.Tensor,
    gamma: float,
    svclass: torch.Tensor = None,
) -> torch.Tensor:
    K = rbf_kernel(X, SV.to(X.dtype), gamma)
    dec = svc_ovo_decision(K, dual_coef.to(X.dtype), intercept.to(X.dtype), n_support)
    return svc_vote(dec, int(n_support.numel()))


def svc_decision(
    X: torch.Tensor,
    SV: torch.Tensor,
    dual_coef: torch.Tensor,
    intercept: torch.Tensor,
    n_support: torch.Tensor,
    gamma: float,
    svclass: torch.Tensor = None,
) -> torch.Tensor:
    """f64 [n, C(C-1)/2] one-vs-one decision values, pair order as
    ``svc_ovo_decision``.  Everything is cast up, so f64 rows give the f64
    decision function."""
    Xd = X.double()
    K = rbf_kernel(Xd, SV.double(), gamma)
    return svc_ovo_decision(K, dual_coef.double(), intercept.double(), n_support)


def svc_couple(
    dec: torch.Tensor,
    probA: torch.Tensor,
    probB: torch.Tensor,
    n_classes: int,
    with_margin: bool = False,
):
    """Class probabilities from one-vs-one decision values: a Platt sigmoid
    per pair, coupled by the method of Wu, Lin and Weng.  A transcription of
    libsvm (sigmoid_predict, svm_predict_probability, multiclass_probability)
    in f64 and in its operation order, rows side by side; every row leaves
    the iteration at its own sweep, as it would alone.

    Returns (proba f64[n,C], idx int32[n], conf f64[n]): ``idx`` is
    ``svc_vote`` of the same decisions and ``conf`` the coupled probability
    of that voted class, which need not be the row's largest.  With
    ``with_margin`` a fourth value: per row, the smallest |max_error - eps|
    over the stopping tests it went through, i.e. how far the row stayed from
    stopping one sweep earlier or later."""
    k = int(n_classes)
    dec = dec.double()
    n = dec.shape[0]
    A = probA.double().to(dec.device)
    B = probB.double().to(dec.device)
    # sigmoid_predict, both branches: exp(-|fApB|) is the argument of each
    fApB = dec * A + B
    e = torch.exp(-fApB.abs())
    s = torch.where(fApB >= 0, e / (1.0 + e), 1.0 / (1 + e))
    s = torch.clamp(s, 1e-7, 1 - 1e-7)
    r = [[None] * k for _ in range(k)]
    p = 0
    for i in range(k):
        for j in range(i + 1, k):
            r[i][j] = s[:, p]
            r[j][i] = 1 - s[:, p]
            p += 1
    zero = torch.zeros(n, dtype=torch.float64, device=dec.device)
    Q = [[None] * k for _ in range(k)]
    for t in range(k):
        q = zero.clone()
        for j in range(t):
            q = q + r[j][t] * r[j][t]
            Q[t][j] = Q[j][t]
        for j in range(t + 1, k):
            q = q + r[j][t] * r[j][t]
            Q[t][j] = -r[j][t] * r[t][j]
        Q[t][t] = q
    pr = [torch.full((n,), 1.0 / k, dtype=torch.float64, device=dec.device) for _ in range(k)]
    eps = 0.005 / k
    active = torch.ones(n, dtype=torch.bool, device=dec.device)
    margin = torch.full((n,), float("inf"), dtype=torch.float64, device=dec.device)
    for _ in range(max(100, k)):
        Qp = []
        pQp = zero.clone()
        for t in range(k):
            a = zero.clone()
            for j in range(k):
                a = a + Q[t][j] * pr[j]
            Qp.append(a)
            pQp = pQp + pr[t] * a
        max_error = zero.clone()
        for t in range(k):
            max_error = torch.maximum(max_error, (Qp[t] - pQp).abs())
        margin = torch.where(active, torch.minimum(margin, (max_error - eps).abs()), margin)
        active = active & ~(max_error < eps)
        if not bool(active.any()):
            break
        new = list(pr)
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t][t]
            new[t] = new[t] + diff
            pQp = (pQp + diff * (diff * Q[t][t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            for j in range(k):
                Qp[j] = (Qp[j] + diff * Q[t][j]) / (1 + diff)
                new[j] = new[j] / (1 + diff)
        pr = [torch.where(active, new[t], pr[t]) for t in range(k)]
    proba = torch.stack(pr, dim=1)
    idx = svc_vote(dec, k)
    conf = torch.gather(proba, 1, idx.long().unsqueeze(1)).squeeze(1)
    if with_margin:
        return proba, idx, conf, margin
    return proba, idx, conf


def platt_fit(dec: torch.Tensor, is_first: torch.Tensor) -> Tuple[float, float]:
    """(A, B) of the sigmoid P(first class | dec) = 1 / (1 + exp(A*dec + B))
    for one class pair: libsvm's sigmoid_train.  ``is_first`` marks the rows
    of the pair's first class, the one a positive decision votes for.
    Prior-smoothed targets, Newton with a backtracking line search
    (max_iter 100, min_step 1e-10, sigma 1e-12, eps 1e-5).  Runs on the host
    in f64: a fit-time step over one pair's rows."""
    d = dec.detach().double().cpu().ravel()
    first = is_first.detach().cpu().ravel().to(torch.bool)
    prior1 = float(first.sum())
    prior0 = float(first.numel()) - prior1
    max_iter, min_step, sigma, eps = 100, 1e-10, 1e-12, 1e-5
    hi = (prior1 + 1.0) / (prior1 + 2.0)
    lo = 1.0 / (prior0 + 2.0)
    t = torch.where(first, torch.tensor(hi, dtype=torch.float64), torch.tensor(lo, dtype=torch.float64))

    def objective(a: float, b: float) -> float:
        f = d * a + b
        lg = torch.log1p(torch.exp(-f.abs()))  # log(1+exp(-|f|)), both branches
        return float(torch.where(f >= 0, t * f + lg, (t - 1) * f + lg).sum())

    A, B = 0.0, float(np.log((prior0 + 1.0) / (prior1 + 1.0)))
    fval = objective(A, B)
    for _ in range(max_iter):
        f = d * A + B
        e = torch.exp(-f.abs())
        p = torch.where(f >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
        q = torch.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        d2 = p * q
        h11 = sigma + float((d * d * d2).sum())
        h22 = sigma + float(d2.sum())
        h21 = float((d * d2).sum())
        d1 = t - p
        g1 = float((d * d1).sum())
        g2 = float(d1.sum())
        if abs(g1) < eps and abs(g2) < eps:
            break
        det = h11 * h22 - h21 * h21
        dA = -(h22 * g1 - h21 * g2) / det
        dB = -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        step = 1.0
        while step >= min_step:
            newA, newB = A + step * dA, B + step * dB
            newf = objective(newA, newB)
            if newf < fval + 0.0001 * step * gd:
                A, B, fval = newA, newB, newf
                break
            step /= 2.0
        if step < min_step:  # line search fails: keep the last iterate
            break
    return A, B


# ----------------------------------------------------------------------
# Random forest predict (N4)
# ----------------------------------------------------------------------


def rf_flatten(trees, n_classes: int) -> Dict[str, torch.Tensor]:
    """Pack per-tree arrays into the SoA layout shared by CPU and HIP
    traversal kernels.

    Layout (per node, 8 bytes in the packed form):
      - non-leaf: threshold f32, right-child u16 (tree-local), feature u8
      - leaf:     payload u32 = row index into ``leaf_proba`` (f32[,(C)])
    sklearn's depth-first builder guarantees left_child == node_index + 1,
    which the packed form relies on (checked here).
    """
    all_thr = []
    all_right = []
    all_feat = []
    all_leafidx = []
    leaf_probs = []
    offsets = [0]
    n_leaves = 0
    for t in trees:
        left = np.asarray(t["left"], dtype=np.int64)
        right = np.asarray(t["right"], dtype=np.int64)
        feat = np.asarray(t["feature"], dtype=np.int64)
        thr = np.asarray(t["threshold"], dtype=np.float64)
        values = np.asarray(t["values"], dtype=np.float64)  # (nodes, C)
        n = left.shape[0]
        is_leaf = left == -1
        # depth-first invariant: left child immediately follows its parent
        inner = ~is_leaf
        if not np.all(left[inner] == np.nonzero(inner)[0] + 1):
            raise ValueError("tree violates left_child == index+1 invariant")
        # normalized per-leaf class distribution (sklearn predict_proba)
        probs = values / np.clip(values.sum(axis=1, keepdims=True), 1e-30, None)
        leaf_idx = np.full(n, -1, dtype=np.int64)
        leaf_idx[is_leaf] = n_leaves + np.arange(int(is_leaf.sum()))
        n_leaves += int(is_leaf.sum())
        leaf_probs.append(probs[is_leaf])
        all_thr.append(np.where(is_leaf, 0.0, thr).astype(np.float32))
        all_right.append(np.where(is_leaf, 0, right).astype(np.int32))
        all_feat.append(np.where(is_leaf, -1, feat).astype(np.int32))
        all_leafidx.append(leaf_idx.astype(np.int32))
        offsets.append(offsets[-1] + n)
    return {
        "threshold": torch.from_numpy(np.concatenate(all_thr)),
        "right": torch.from_numpy(np.concatenate(all_right)),
        "feature": torch.from_numpy(np.concatenate(all_feat)),
        "leaf_index": torch.from_numpy(np.concatenate(all_leafidx)),
        "leaf_proba": torch.from_numpy(np.concatenate(leaf_probs).astype(np.float32)),
        "tree_offset": torch.tensor(offsets, dtype=torch.int32),
        "n_classes": torch.tensor(n_classes, dtype=torch.int32),
    }


def rf_predict_proba(X: torch.Tensor, forest: Dict[str, torch.Tensor]) -> torch.Tensor:
    """Vectorised level-synchronous traversal: all rows advance one level per
    iteration (CPU oracle for the HIP per-lane traversal kernel)."""
    n = X.shape[0]
    device = X.device
    thr = forest["threshold"].to(device)
    right = forest["right"].to(device)
    feat = forest["feature"].to(device)
    leaf_index = forest["leaf_index"].to(device)
    leaf_proba = forest["leaf_proba"].to(device)
    offsets = forest["tree_offset"].to(device)
    C = int(forest["n_classes"])
    n_trees = offsets.numel() - 1
    acc = torch.zeros(n, C, dtype=torch.float32, device=device)
    rows = torch.arange(n, device=device)
    for t in range(n_trees):
        base = int(offsets[t])
        idx = torch.zeros(n, dtype=torch.long, device=device)
        active = torch.ones(n, dtype=torch.bool, device=device)
        while bool(active.any()):
            g = base + idx
            f = feat[g]
            leaf = f < 0
            done = active & leaf
            if bool(done.any()):
                acc[rows[done]] += leaf_proba[leaf_index[g[done]].long()]
                active = active & ~leaf
            still = active
            if bool(still.any()):
                gs = g[still]
                go_left = X[still, f[still].long()] <= thr[gs]
                nxt = torch.where(go_left, idx[still] + 1, right[gs].long())
                idx = idx.clone()
                idx[still] = nxt
    return acc / n_trees


def rf_argmax(X: torch.Tensor, forest: Dict[str, torch.Tensor]) -> torch.Tensor:
    return torch.argmax(rf_predict_proba(X, forest), dim=1).to(torch.int32)


def rf_predict_scores(
    X: torch.Tensor, forest: Dict[str, torch.Tensor], want_proba: bool = True
) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """(proba[n,C] f32, labels[n] int32, conf[n] f32): the class
    probabilities, their first-maximum argmax and the top probability (CPU
    oracle of the HIP scores kernels).  ``want_proba=False`` returns None in
    place of proba."""
    proba = rf_predict_proba(X, forest)
    labels = torch.argmax(proba, dim=1).to(torch.int32)
    conf = proba.max(dim=1).values
    return (proba if want_proba else None), labels, conf


# ----------------------------------------------------------------------
# Forest feature contributions (CPU oracle of csrc/rf_explain_kernels.hip)
# ----------------------------------------------------------------------

# a step of a class probability is stored as rint(step * 2^30) in an int32
RF_EXPLAIN_SCALE = float(1 << 30)
# T * max_depth below this keeps |S| under 2^22 * 2^30 = 2^52, exact in f64
RF_EXPLAIN_MAX_TERMS = 1 << 22
RF_EXPLAIN_MAX_TREES = 4096


def rf_explain_flatten(trees, n_classes: int) -> Dict[str, object]:
    """The tables of rf_explain next to rf_flatten's, in its node order:
    ``{"delta": int32 [n_nodes, C], "bias": f64 [C], "max_depth": int}``.

    With p_v = values[v] / sum(values[v]) in f64 (rf_flatten's leaf
    normalisation, here for every node), row w of ``delta`` holds
    rint((p_w - p_parent(w)) * 2^30), half to even, and zeros for a root;
    ``bias`` is the mean over the trees of p_root and ``max_depth`` the
    longest path in edges.  ValueError when T * max_depth >= 2^22 (the sums of
    rf_explain would leave the exact range), and for a tree that is not in
    depth-first order.
    """
    C = int(n_classes)
    deltas, roots = [], []
    max_depth = 0
    for t in trees:
        left = np.asarray(t["left"], dtype=np.int64)
        right = np.asarray(t["right"], dtype=np.int64)
        values = np.asarray(t["values"], dtype=np.float64).reshape(left.shape[0], -1)
        n = left.shape[0]
        if values.shape[1] != C:
            raise ValueError(f"a tree holds {values.shape[1]} classes per node, not {C}")
        inner = np.nonzero(left != -1)[0]
        if n < 1 or not (
            np.all(left[inner] == inner + 1)
            and np.all(right[inner] > inner + 1)
            and np.all(right[inner] < n)
        ):
            raise ValueError("tree violates left_child == index+1 invariant")
        p = values / np.clip(values.sum(axis=1, keepdims=True), 1e-30, None)
        parent = np.zeros(n, dtype=np.int64)  # a root is its own parent: zeros
        parent[left[inner]] = parent[right[inner]] = inner
        # depth = number of ancestors, by pointer doubling: log2(depth) rounds
        depth = (np.arange(n) > 0).astype(np.int64)
        jump = parent
        while jump.any():
            depth = depth + depth[jump]
            jump = jump[jump]
        deltas.append(np.rint((p - p[parent]) * RF_EXPLAIN_SCALE).astype(np.int32))
        roots.append(p[0])
        max_depth = max(max_depth, int(depth.max()))
    if not deltas:
        raise ValueError("a forest needs at least one tree")
    if len(deltas) * max_depth >= RF_EXPLAIN_MAX_TERMS:
        raise ValueError(
            f"{len(deltas)} trees of depth {max_depth} have 2^22 or more path edges: "
            "the contribution sums would not stay exact"
        )
    return {
        "delta": torch.from_numpy(np.ascontiguousarray(np.concatenate(deltas))),
        "bias": torch.from_numpy(np.stack(roots).sum(axis=0) / len(roots)),
        "max_depth": max_depth,
    }


def rf_explain_check(X, forest, tables, labels) -> Tuple[int, int]:
    """Argument rules of rf_explain, shared by the CPU and GPU bindings: no
    cast and no copy is made for the caller, so a wrong dtype or layout is an
    error.  Returns (T, C)."""
    for name, t in (("X", X), ("labels", labels)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"rf_explain takes tensors, got {type(t).__name__} for {name}")
    if X.dim() != 2 or X.dtype != torch.float32 or not X.is_contiguous():
        raise ValueError(
            f"rf_explain takes contiguous f32 (n, features) rows, got {X.dtype} {tuple(X.shape)}"
        )
    n = X.shape[0]
    if (
        labels.dtype != torch.int32
        or tuple(labels.shape) != (n,)
        or not labels.is_contiguous()
        or labels.device != X.device
    ):
        raise ValueError(f"labels must be a contiguous int32 ({n},) tensor on X's device")
    T = forest["tree_offset"].numel() - 1
    n_nodes = forest["feature"].numel()
    delta = tables["delta"]
    if (
        not isinstance(delta, torch.Tensor)
        or delta.dtype != torch.int32
        or delta.dim() != 2
        or delta.shape[0] != n_nodes
        or delta.shape[1] < 1
    ):
        raise ValueError(f"tables['delta'] must be int32 ({n_nodes}, C): one row per node")
    C = delta.shape[1]  # (the forest's own count may live on a device)
    if T < 1 or T * int(tables["max_depth"]) >= RF_EXPLAIN_MAX_TERMS:
        raise ValueError(
            f"rf_explain takes a forest of 1 or more trees with T * max_depth < 2^22, got "
            f"T = {T}, max_depth = {tables['max_depth']}"
        )
    top = forest.get("_max_feature")
    if top is None:  # read back once, not in every (possibly captured) pass
        top = forest["_max_feature"] = int(forest["feature"].max())
    if top >= X.shape[1]:
        raise ValueError(f"the forest splits on feature {top}, X has {X.shape[1]} columns")
    return T, C


def rf_explain(
    X: torch.Tensor,
    forest: Dict[str, torch.Tensor],
    tables: Dict[str, object],
    labels: torch.Tensor,
    want_matrix: bool = True,
    want_sums: bool = False,
) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Why the forest gives each row the class ``labels`` names: (contrib f32
    [n, F] | None, why int32 [n], why_value f32 [n], sums int64 [n, F] |
    None), the Saabas decomposition over rf_explain_flatten's ``tables``.

    A row walks every tree by rf_predict_proba's rule (``x[f] <= threshold``
    goes left, to the next entry; a NaN goes right).  sums[f] adds
    delta[w, label] over all trees and all edges v -> w of the paths with
    feature(v) = f: integers, so the sum is exact in any order.  contrib[f] =
    (float)((double)sums[f] / (2^30 T)), and tables["bias"][label] +
    sum(contrib) is the forest's probability of that class up to max_depth *
    2^-31.  why is the first-maximum argmax of sums if that maximum is > 0,
    else -1, and why_value = contrib[why], or 0.  A label outside [0, C) gives
    zeros, -1 and 0.
    """
    T, C = rf_explain_check(X, forest, tables, labels)
    dev = X.device
    n, F = X.shape
    offsets, right_global, _ = _iforest_layout(forest)
    feat = forest["feature"].to(dev).long()
    thr = forest["threshold"].to(dev)
    right_global = right_global.to(dev)
    delta = tables["delta"].to(dev).reshape(-1).long()
    lab = labels.long()
    known = (lab >= 0) & (lab < C)
    col = torch.where(known, lab, torch.zeros_like(lab)).unsqueeze(1)
    sums = torch.zeros(n, F, dtype=torch.int64, device=dev)
    for lo in range(0, n, 32768):  # bounds the [rows, T] index matrices
        x = X[lo : lo + 32768]
        idx = offsets[:-1].to(dev).unsqueeze(0).expand(x.shape[0], -1).contiguous()
        part = sums[lo : lo + 32768]
        while True:
            f = feat[idx]
            leaf = f < 0
            if bool(leaf.all()):
                break
            f = f.clamp(min=0)
            nxt = torch.where(x.gather(1, f) <= thr[idx], idx + 1, right_global[idx])
            nxt = torch.where(leaf, idx, nxt)
            step = delta[nxt * C + col[lo : lo + 32768]]
            part.scatter_add_(1, f, torch.where(leaf, torch.zeros_like(step), step))
            idx = nxt
    sums = torch.where(known.unsqueeze(1), sums, torch.zeros_like(sums))
    contrib = (sums.double() / (RF_EXPLAIN_SCALE * T)).to(torch.float32)
    if F:
        best = sums.max(dim=1).values
        # the first column that reaches the maximum (see ensemble_vote)
        first = torch.argmax((sums == best.unsqueeze(1)).to(torch.uint8), dim=1)
        why = torch.where(best > 0, first, torch.full_like(first, -1))
        why_value = torch.where(
            best > 0, contrib.gather(1, first.unsqueeze(1)).squeeze(1), torch.zeros_like(contrib[:, 0])
        )
    else:
        why = torch.full((n,), -1, dtype=torch.int64, device=dev)
        why_value = torch.zeros(n, dtype=torch.float32, device=dev)
    return (
        (contrib if want_matrix else None),
        why.to(torch.int32),
        why_value,
        (sums if want_sums else None),
    )


# ----------------------------------------------------------------------
# Isolation forest novelty score (CPU oracle of csrc/iforest_kernels.hip)
# ----------------------------------------------------------------------

_EULER_GAMMA = 0.5772156649015329

# what the packed node and the exact f64 sum hold (see iforest_pack)
IFOREST_MAX_TREES = 4096
IFOREST_MAX_H = 64.0
IFOREST_MAX_NODES = (1 << 24) - 1


def iforest_c(n) -> np.ndarray:
    """Average path length of an unsuccessful search in a binary search tree
    of n rows, f64: 0 for n <= 1, 1 for n == 2, else
    2 (ln(n - 1) + gamma) - 2 (n - 1) / n."""
    n = np.asarray(n, dtype=np.float64)
    big = np.maximum(n, 3.0)
    c = 2.0 * (np.log(big - 1.0) + _EULER_GAMMA) - 2.0 * (big - 1.0) / big
    return np.where(n <= 1.0, 0.0, np.where(n <= 2.0, 1.0, c))


def _f32_round_down(v: np.ndarray) -> np.ndarray:
    """The largest f32 <= each f64 value: the only f32 threshold t with
    (x <= t) == (x <= v) for EVERY f32 x.  A plain cast rounds to nearest and
    may land above v, which sends the f32 just above v to the wrong child."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore"):
        t = v.astype(np.float32)
    above = t.astype(np.float64) > v
    t[above] = np.nextafter(t[above], np.float32(-np.inf))
    return t


def iforest_flatten(trees, max_samples: int) -> Dict[str, torch.Tensor]:
    """Isolation trees -> the SoA layout of rf_flatten, with a leaf value in
    place of a class distribution.

    Each tree is a dict of per-node arrays ``left``, ``right``, ``feature``,
    ``threshold`` (f64) and ``n_node_samples``, a leaf having ``left == -1``,
    in depth-first order with ``left == index + 1`` (checked here).
    ``max_samples`` is psi, the rows each tree was grown on.

    ``threshold`` is the largest f32 <= the f64 threshold (_f32_round_down).
    ``leaf_h`` holds, per leaf, h = depth + c(n_node_samples), computed in f64
    and rounded once to f32; 0 for an inner node.
    """
    all_thr, all_right, all_feat, all_h = [], [], [], []
    offsets = [0]
    for t in trees:
        left = np.asarray(t["left"], dtype=np.int64)
        right = np.asarray(t["right"], dtype=np.int64)
        feat = np.asarray(t["feature"], dtype=np.int64)
        thr = np.asarray(t["threshold"], dtype=np.float64)
        nns = np.asarray(t["n_node_samples"], dtype=np.float64)
        n = left.shape[0]
        is_leaf = left == -1
        inner = np.nonzero(~is_leaf)[0]
        if n < 1 or not (
            np.all(left[inner] == inner + 1)
            and np.all(right[inner] > inner + 1)
            and np.all(right[inner] < n)
        ):
            raise ValueError("isolation tree is not in depth-first order (left == index + 1)")
        depth = np.zeros(n, dtype=np.int64)
        for i in inner:  # children follow their parent
            depth[left[i]] = depth[i] + 1
            depth[right[i]] = depth[i] + 1
        h = depth.astype(np.float64) + iforest_c(nns)
        all_thr.append(np.where(is_leaf, np.float32(0.0), _f32_round_down(thr)))
        all_right.append(np.where(is_leaf, 0, right).astype(np.int32))
        all_feat.append(np.where(is_leaf, -1, feat).astype(np.int32))
        all_h.append(np.where(is_leaf, h, 0.0).astype(np.float32))
        offsets.append(offsets[-1] + n)
    if not all_thr:
        raise ValueError("an isolation forest needs at least one tree")
    return {
        "threshold": torch.from_numpy(np.concatenate(all_thr).astype(np.float32)),
        "right": torch.from_numpy(np.concatenate(all_right)),
        "feature": torch.from_numpy(np.concatenate(all_feat)),
        "leaf_h": torch.from_numpy(np.concatenate(all_h)),
        "tree_offset": torch.tensor(offsets, dtype=torch.int32),
        "max_samples": torch.tensor(int(max_samples), dtype=torch.int32),
    }


def _iforest_layout(forest: Dict[str, torch.Tensor]):
    """(offsets i64 [T+1], right_global i64 [n_nodes], next_root i64
    [n_nodes]) of a flattened forest, on the host."""
    offsets = forest["tree_offset"].cpu().to(torch.int64)
    counts = offsets[1:] - offsets[:-1]
    n_nodes = forest["feature"].numel()
    if (
        offsets.numel() < 2 or int(offsets[0]) != 0 or int(offsets[-1]) != n_nodes
        or bool((counts < 1).any())
    ):
        raise ValueError("tree_offset must rise from 0 to n_nodes, one or more nodes per tree")
    base = torch.repeat_interleave(offsets[:-1], counts)
    next_root = torch.repeat_interleave(offsets[1:], counts)
    return offsets, forest["right"].cpu().to(torch.int64) + base, next_root


def iforest_consts(forest: Dict[str, torch.Tensor]) -> Tuple[int, float, float]:
    """(T, c(psi), inv_denom = 1 / (T c(psi))), the last two as f64; cached in
    the forest dict, so that a forest on a device is read back once and not
    in every (possibly captured) pass."""
    consts = forest.get("_consts")
    if consts is None:
        T = forest["tree_offset"].numel() - 1
        psi = int(forest["max_samples"])
        if psi < 2:
            raise ValueError(f"an isolation forest needs max_samples >= 2, got {psi}")
        c_psi = float(iforest_c(psi))
        consts = forest["_consts"] = (T, c_psi, 1.0 / (T * c_psi))
    return consts


def iforest_depth_cut(threshold, T: int, c_psi: float) -> float:
    """The f64 path-length sum below which a row is novel:
    score > threshold  <=>  psum < -log2(threshold) T c(psi).  ``None`` gives
    -inf: nothing is flagged.  ValueError unless 0 < threshold < 1."""
    if threshold is None:
        return float("-inf")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.floating)):
        raise ValueError(f"threshold must be None or a float in (0, 1), got {threshold!r}")
    thr = float(threshold)
    if not 0.0 < thr < 1.0:
        raise ValueError(f"threshold must be inside (0, 1), got {threshold!r}")
    return -float(np.log2(thr)) * T * c_psi


def iforest_pack(forest: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    """Pack a flattened isolation forest into the kernels' uint2 node table.

    ``nodes``, n_nodes entries in rf_pack's layout:
      inner: word0 = f32 threshold bits, word1 = (right_child_GLOBAL << 8) | feature
      leaf:  word0 = f32 bits of h = depth + c(n_node_samples), word1 = 0xff
    ``roots`` are the T root indices.

    ValueError for what the kernels or the exact sum cannot hold: a right
    child that does not lie after its parent's left child inside the same
    tree (a tree not in depth-first order), a feature outside 0..11, more
    than 4096 trees, a leaf value that is not 0 or in [1, 64) (with 4096
    trees the f64 sum of such values stays an exact multiple of 2^-23 below
    2^18), more than 2^24 - 1 nodes (the child link has 24 bits).
    """
    n_nodes = forest["feature"].numel()
    n_trees = forest["tree_offset"].numel() - 1
    if n_trees > IFOREST_MAX_TREES:
        raise ValueError(f"the isolation forest kernels take at most 4096 trees, got {n_trees}")
    if n_nodes > IFOREST_MAX_NODES:
        raise ValueError(f"packed node format holds at most 2^24 - 1 nodes, got {n_nodes}")
    offsets, right_global, next_root = _iforest_layout(forest)
    feat = forest["feature"].cpu().to(torch.int64)
    thr = forest["threshold"].cpu().to(torch.float32)
    leaf_h = forest["leaf_h"].cpu().to(torch.float32)
    index = torch.arange(n_nodes, dtype=torch.int64)
    is_leaf = feat < 0
    if bool((feat[~is_leaf] > 11).any()):
        raise ValueError("an isolation tree splits on a feature outside 0..11")
    ok = (right_global > index + 1) & (right_global < next_root)
    if not bool(ok[~is_leaf].all()):
        raise ValueError(
            "isolation tree is not in depth-first order: a right child must lie after "
            "its parent's left child, inside the same tree"
        )
    # (every link so stays inside its tree and points forward: a walk ends)
    h = leaf_h[is_leaf]
    if not bool(((h == 0) | ((h >= 1) & (h < IFOREST_MAX_H))).all()):
        raise ValueError("a leaf value h = depth + c(n) must be 0 or in [1, 64)")
    consts = iforest_consts(forest)
    w0 = torch.where(is_leaf, leaf_h, thr).view(torch.int32)
    w1 = torch.where(is_leaf, torch.tensor(0xFF, dtype=torch.int64), (right_global << 8) | feat)
    # bits 31 of word1 are set from 2^23 nodes on: keep the bit pattern
    w1 = torch.where(w1 >= 1 << 31, w1 - (1 << 32), w1).to(torch.int32)
    nodes = torch.stack([w0, w1], dim=1).contiguous()
    return {
        "nodes": nodes.to(device),
        "roots": offsets[:-1].to(torch.int32).to(device),
        "n_trees": consts[0],
        "c_psi": consts[1],
        "inv_denom": consts[2],
    }


def iforest_score_check(X, forest, threshold, labels) -> float:
    """Argument rules of iforest_score, shared by the CPU and GPU bindings:
    no cast and no copy is made for the caller, so a wrong dtype or layout is
    an error.  Returns depth_cut (iforest_depth_cut)."""
    if not isinstance(X, torch.Tensor):
        raise ValueError(f"iforest_score takes a tensor, got {type(X).__name__}")
    if X.dim() != 2 or X.shape[1] != len(_FEATURE_NAMES):
        raise ValueError(f"iforest_score takes (n, 12) features, got {tuple(X.shape)}")
    if X.dtype != torch.float32:
        raise ValueError(f"iforest_score takes f32 features, got {X.dtype}")
    if not X.is_contiguous():
        raise ValueError("X must be contiguous")
    n = X.shape[0]
    if labels is not None:
        if (
            not isinstance(labels, torch.Tensor)
            or labels.dtype != torch.int32
            or tuple(labels.shape) != (n,)
            or not labels.is_contiguous()
            or labels.device != X.device
        ):
            raise ValueError(f"labels must be None or a contiguous int32 ({n},) tensor on X's device")
    T, c_psi, _ = iforest_consts(forest)
    if not 1 <= T <= IFOREST_MAX_TREES:
        raise ValueError(f"iforest_score takes 1..4096 trees, got {T}")
    return iforest_depth_cut(threshold, T, c_psi)


def iforest_leaves(X: torch.Tensor, forest: Dict[str, torch.Tensor]) -> torch.Tensor:
    """int64 [n, T]: the GLOBAL index of the leaf each row reaches in each
    tree.  Level-synchronous: all rows advance one level in all trees per
    iteration.  ``x <= thr`` is false for a NaN, which so goes right."""
    dev = X.device
    offsets, right_global, _ = _iforest_layout(forest)
    feat = forest["feature"].to(dev).long()
    thr = forest["threshold"].to(dev)
    right_global = right_global.to(dev)
    n = X.shape[0]
    idx = offsets[:-1].to(dev).unsqueeze(0).expand(n, -1).contiguous()
    while True:
        f = feat[idx]
        leaf = f < 0
        if bool(leaf.all()):
            return idx
        xv = X.gather(1, f.clamp(min=0))
        nxt = torch.where(xv <= thr[idx], idx + 1, right_global[idx])
        idx = torch.where(leaf, idx, nxt)


def iforest_score(
    X: torch.Tensor,
    forest: Dict[str, torch.Tensor],
    threshold: Optional[float] = None,
    labels: Optional[torch.Tensor] = None,
    want_sum: bool = False,
) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(score f32 [n], flags u8 [n], labels_out int32 [n] | None, psum f64 [n]
    | None) of a flattened isolation forest (iforest_flatten).

    psum is the sum over the trees of the leaf value h = depth + c(n_leaf) a
    row reaches; every h is a multiple of 2^-23 below 64, so the f64 sum is
    exact in any order.  score = 2^(-psum / (T c(psi))) in (0, 1], higher
    meaning more anomalous (sklearn's -score_samples).  A row is flagged when
    psum < depth_cut = -log2(threshold) T c(psi), which is score > threshold
    decided on the exact sum; ``threshold=None`` flags nothing.  With
    ``labels``, labels_out is -1 for a flagged row and its label otherwise,
    so that class_traffic counts flagged rows as unknown.
    """
    depth_cut = iforest_score_check(X, forest, threshold, labels)
    inv_denom = iforest_consts(forest)[2]
    leaf_h = forest["leaf_h"].to(X.device)
    n = X.shape[0]
    psum = torch.empty(n, dtype=torch.float64, device=X.device)
    for lo in range(0, n, 32768):  # bounds the [rows, T] index matrices
        leaves = iforest_leaves(X[lo : lo + 32768], forest)
        psum[lo : lo + 32768] = leaf_h[leaves].double().sum(dim=1)
    score = torch.exp2(-psum * inv_denom).to(torch.float32)
    novel = psum < depth_cut
    labels_out = None
    if labels is not None:
        labels_out = torch.where(novel, torch.full_like(labels, -1), labels)
    return score, novel.to(torch.uint8), labels_out, (psum if want_sum else None)


# ----------------------------------------------------------------------
# Class probabilities as f32 tensors, and the soft vote over them (CPU
# oracles of csrc/ensemble_kernels.hip)
# ----------------------------------------------------------------------


def gnb_proba(
    X: torch.Tensor, theta: torch.Tensor, var: torch.Tensor, class_prior: torch.Tensor
) -> torch.Tensor:
    """softmax of the joint log-likelihoods, computed in f64, as f32 [n,C]."""
    ll = gnb_joint_loglik(X.double(), theta.double(), var.double(), class_prior.double())
    return torch.softmax(ll, dim=1).to(torch.float32)


def linear_proba(X: torch.Tensor, coef: torch.Tensor, intercept: torch.Tensor) -> torch.Tensor:
    """softmax of the logits, computed in f64 from the parameters as they
    are stored, as f32 [n,C]."""
    logits = linear_logits(X.double(), coef.double(), intercept.double())
    return torch.softmax(logits, dim=1).to(torch.float32)


def knn_vote_proba(idx: torch.Tensor, y: torch.Tensor, n_classes: int) -> torch.Tensor:
    """Neighbour vote fractions: proba[c] = count[c] / k_valid as an f32
    division.  An entry with idx < 0 is padding and is not counted; k_valid
    is the number of counted entries (the contract is k_valid >= 1)."""
    if not 2 <= int(n_classes) <= 8:
        raise ValueError(f"knn_vote_proba supports 2..8 classes, got {n_classes}")
    idx = idx.long()
    valid = idx >= 0
    lab = y.long()[idx.clamp(min=0)]
    classes = torch.arange(n_classes, device=idx.device)
    hit = (lab.unsqueeze(2) == classes) & valid.unsqueeze(2)  # (n, k, C)
    count = hit.sum(dim=1).to(torch.float32)
    return count / valid.sum(dim=1, keepdim=True).to(torch.float32)


def ensemble_weights(weights, n_members: int):
    """Member weights as the vote uses them: divided by their f64 sum, then
    rounded to f32 (returned as Python floats).  ``None`` means equal
    weights.  ValueError for a wrong count, and for a weight that is not
    finite, not positive, or whose total is zero."""
    if weights is None:
        weights = [1.0] * n_members
    w = np.asarray([float(v) for v in weights], dtype=np.float64)
    if w.shape != (n_members,):
        raise ValueError(f"{w.size} weights for {n_members} ensemble members")
    if not bool(np.isfinite(w).all()) or bool((w <= 0.0).any()):
        raise ValueError("ensemble weights must be finite and positive")
    total = float(w.sum())
    if not np.isfinite(total) or total <= 0.0:
        raise ValueError("ensemble weights must have a finite, positive total")
    w32 = (w / total).astype(np.float32)
    if bool((w32 <= 0.0).any()):
        raise ValueError("an ensemble weight vanishes next to the others")
    return [float(v) for v in w32]


def ensemble_check(probas, colmaps, weights, n_classes: int):
    """Argument rules of ensemble_vote, shared by the CPU and GPU bindings:
    1..8 members of 2..8 classes with one row count, one map entry below
    ``n_classes`` per member column, ``n_classes`` in 2..8.  Returns the
    normalised f32 weights."""
    M = len(probas)
    if not 1 <= M <= 8:
        raise ValueError(f"ensemble_vote takes 1..8 members, got {M}")
    if not 2 <= int(n_classes) <= 8:
        raise ValueError(f"ensemble_vote supports 2..8 classes, got {n_classes}")
    if len(colmaps) != M:
        raise ValueError(f"{len(colmaps)} column maps for {M} ensemble members")
    n = probas[0].shape[0]
    for p, cmap in zip(probas, colmaps):
        if p.dim() != 2 or not 2 <= p.shape[1] <= 8:
            raise ValueError(f"member probabilities must be (n, 2..8), got {tuple(p.shape)}")
        if p.shape[0] != n:
            raise ValueError(f"members differ in their row count: {p.shape[0]} and {n}")
        if len(cmap) != p.shape[1]:
            raise ValueError(f"{len(cmap)} map entries for {p.shape[1]} member classes")
        if any(not 0 <= int(c) < n_classes for c in cmap):
            raise ValueError(f"column map {list(cmap)} points outside {n_classes} classes")
    return ensemble_weights(weights, M)


def ensemble_vote(
    probas, colmaps, weights, n_classes: int, want_proba: bool = True
) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """Soft vote: (avg[n,C] f32 | None, label[n] int32, conf[n] f32).

    ``probas[m]`` is member m's [n, C_m] f32 probabilities, ``colmaps[m][j]``
    the ensemble column of its column j and ``weights[m]`` its weight
    (normalised here, see ensemble_weights).  Per row avg starts at zero and
    takes, in member order, avg[col] = fma(w_m, p_m[j], avg[col]) in f32; a
    class a member lacks gets nothing from it.  label is the first-maximum
    argmax of avg and conf its maximum.

    The fused step is formed in f64, where the product of two f32 values is
    exact, and rounded to f32: the kernel's fmaf up to the double rounding
    of the sum.
    """
    w32 = ensemble_check(probas, colmaps, weights, n_classes)
    n = probas[0].shape[0]
    avg = torch.zeros(n, n_classes, dtype=torch.float32, device=probas[0].device)
    for p, cmap, w in zip(probas, colmaps, w32):
        p64 = p.to(torch.float32).double()
        for j, col in enumerate(cmap):
            avg[:, col] = (avg[:, col].double() + w * p64[:, j]).to(torch.float32)
    conf, label = avg.max(dim=1)
    # torch.max returns the first maximum on CPU and leaves the choice open
    # on other devices: take the first column that reaches it
    label = torch.argmax((avg == conf.unsqueeze(1)).to(torch.uint8), dim=1)
    return (avg if want_proba else None), label.to(torch.int32), conf


def proba_smooth_check(proba, state, held, alpha, margin, n_live):
    """Argument rules of proba_smooth, shared by the CPU and GPU bindings.
    Returns (a, b, margin) as Python floats holding the f32 values the op
    works with: a = f32(alpha), b = 1 - a in f32, f32(margin)."""
    if proba.dim() != 2 or not 2 <= proba.shape[1] <= 8:
        raise ValueError(f"proba_smooth takes (n, 2..8) probabilities, got {tuple(proba.shape)}")
    n, C = proba.shape
    if state.dim() != 2 or state.shape[1] != C or held.dim() != 1:
        raise ValueError(
            f"proba_smooth takes state (cap, {C}) and held (cap), got "
            f"{tuple(state.shape)} and {tuple(held.shape)}"
        )
    if state.shape[0] < n or held.shape[0] < n:
        raise ValueError(
            f"{n} rows do not fit a state of {state.shape[0]} and a held of {held.shape[0]} rows"
        )
    if proba.dtype != torch.float32 or state.dtype != torch.float32 or held.dtype != torch.int32:
        raise ValueError("proba_smooth takes f32 proba, f32 state and int32 held")
    if not (proba.is_contiguous() and state.is_contiguous() and held.is_contiguous()):
        raise ValueError("proba, state and held must be contiguous")
    if state.device != proba.device or held.device != proba.device:
        raise ValueError("proba, state and held must be on one device")
    p0, s0 = proba.data_ptr(), state.data_ptr()
    if proba.numel() and p0 < s0 + state.numel() * 4 and s0 < p0 + proba.numel() * 4:
        raise ValueError("proba must not alias state")
    if n_live is not None:
        if (
            not isinstance(n_live, torch.Tensor)
            or n_live.dtype != torch.int32
            or tuple(n_live.shape) != (1,)
            or n_live.device != proba.device
        ):
            raise ValueError("n_live must be None or an int32 [1] tensor on proba's device")
    a = np.float32(alpha)
    if not (np.float32(0.0) < a <= np.float32(1.0)) or not 0.0 < float(alpha) <= 1.0:
        raise ValueError(f"alpha must be in (0, 1], got {alpha}")
    m = np.float32(margin)
    if not bool(np.isfinite(m)) or not m >= 0 or not np.isfinite(float(margin)):
        raise ValueError(f"margin must be finite and >= 0, got {margin}")
    return float(a), float(np.float32(1.0) - a), float(m)


def proba_smooth(
    proba: torch.Tensor,
    state: torch.Tensor,
    held: torch.Tensor,
    alpha: float,
    margin: float = 0.0,
    n_live: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-flow smoothing across polls: (label[n] int32, conf[n] f32).

    ``state`` [cap, C] f32 and ``held`` [cap] int32 (-1: never seen) belong
    to the flow slots and are updated in place, rows < n only.  With a =
    f32(alpha) and b = 1 - a in f32, per row r:

    * r >= n_live[0]: state[r] = 0, held[r] = -1; label is the
      first-maximum argmax of proba[r] and conf that maximum;
    * held[r] < 0: s = proba[r] bit for bit;
    * otherwise s[c] = fma(a, proba[r,c], b * state[r,c]), the product
      rounded to f32 once and the fused add once;

    then top = first-maximum argmax of s, and label = held[r] unless
    s[top] - s[held[r]] > margin (an exact tie keeps the held label).
    state[r] = s, held[r] = label, conf = s[label].

    The fused step is formed in f64, where a * proba is exact, and rounded
    to f32: the kernel's fmaf up to the double rounding of the sum.  Nothing
    here reads a value back to the host, so the same formulation runs on
    device tensors.
    """
    a, b, m = proba_smooth_check(proba, state, held, alpha, margin, n_live)
    n = proba.shape[0]
    dev = proba.device
    if n == 0:
        return (torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.float32, device=dev))
    old = state[:n]
    h = held[:n].long()
    if n_live is None:
        live = torch.ones(n, dtype=torch.bool, device=dev)
    else:
        live = torch.arange(n, device=dev) < n_live.long()
    seen = live & (h >= 0)
    ema = (a * proba.double() + (b * old).double()).to(torch.float32)
    s = torch.where(seen.unsqueeze(1), ema, proba)
    best = s.max(dim=1).values
    # the first column that reaches the maximum (see ensemble_vote)
    top = torch.argmax((s == best.unsqueeze(1)).to(torch.uint8), dim=1)
    hc = h.clamp(min=0)
    sh = s.gather(1, hc.unsqueeze(1)).squeeze(1)
    keep = seen & ~((best - sh) > m)
    label = torch.where(keep, hc, top)
    conf = s.gather(1, label.unsqueeze(1)).squeeze(1)
    state[:n] = torch.where(live.unsqueeze(1), s, torch.zeros_like(s))
    held[:n] = torch.where(live, label, torch.full_like(label, -1)).to(torch.int32)
    return label.to(torch.int32), conf


# ----------------------------------------------------------------------
# Per-class traffic accounting
# ----------------------------------------------------------------------

# the columns of class_traffic's totals
TRAFFIC_COLUMNS = ("flows",) + _FEATURE_NAMES


def class_traffic_check(X, labels, n_classes, conf, min_conf, n_live):
    """Argument rules of class_traffic, shared by the CPU and GPU bindings.
    Returns (C, min_conf) with min_conf a Python float holding f32(min_conf),
    the value a confidence is compared with."""
    for name, t in (("X", X), ("labels", labels)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"class_traffic takes tensors, got {type(t).__name__} for {name}")
    if isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer)):
        raise ValueError(f"n_classes must be an int, got {n_classes!r}")
    C = int(n_classes)
    if not 2 <= C <= 8:
        raise ValueError(f"class_traffic supports 2..8 classes, got {C}")
    if X.dim() != 2 or X.shape[1] != len(_FEATURE_NAMES):
        raise ValueError(f"class_traffic takes (n, 12) features, got {tuple(X.shape)}")
    n = X.shape[0]
    if tuple(labels.shape) != (n,):
        raise ValueError(f"class_traffic takes labels ({n},), got {tuple(labels.shape)}")
    if X.dtype != torch.float32 or labels.dtype != torch.int32:
        raise ValueError("class_traffic takes f32 X and int32 labels")
    if not (X.is_contiguous() and labels.is_contiguous()):
        raise ValueError("X and labels must be contiguous")
    if labels.device != X.device:
        raise ValueError("X and labels must be on one device")
    if conf is not None:
        if (
            not isinstance(conf, torch.Tensor)
            or conf.dtype != torch.float32
            or tuple(conf.shape) != (n,)
            or not conf.is_contiguous()
            or conf.device != X.device
        ):
            raise ValueError(f"conf must be None or a contiguous f32 ({n},) tensor on X's device")
    if n_live is not None:
        if (
            not isinstance(n_live, torch.Tensor)
            or n_live.dtype != torch.int32
            or tuple(n_live.shape) != (1,)
            or n_live.device != X.device
        ):
            raise ValueError("n_live must be None or an int32 [1] tensor on X's device")
    with np.errstate(over="ignore"):
        m = np.float32(min_conf)
    if not np.isfinite(float(min_conf)) or not bool(np.isfinite(m)):
        raise ValueError(f"min_conf must be finite, got {min_conf}")
    return C, float(m)


def class_traffic(
    X: torch.Tensor,
    labels: torch.Tensor,
    n_classes: int,
    conf: Optional[torch.Tensor] = None,
    min_conf: float = 0.0,
    n_live: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Per-class flow count and feature sums: totals [C + 1, 13] f64, the
    columns TRAFFIC_COLUMNS.

    Row r < min(n, n_live[0]) belongs to group labels[r], or to group C
    ("unknown") when its label is outside 0..C-1 or ``conf`` is given and
    conf[r] < f32(min_conf) (false for a NaN confidence).  totals[g, 0]
    counts the group's rows and totals[g, 1 + j] sums (double)X[r, j] over
    them.  Rows at or past n_live[0] contribute nothing; every cell is
    written, zeros included.

    A plain index_add_: a NaN or infinity reaches the one cell of its row's
    group and column.  Dead rows go to a spare group that is cut off, not
    through a 0/1 factor.  Nothing here reads a value back to the host, so
    the same formulation runs on device tensors.
    """
    C, mc = class_traffic_check(X, labels, n_classes, conf, min_conf, n_live)
    n = X.shape[0]
    dev = X.device
    totals = torch.zeros(C + 2, len(TRAFFIC_COLUMNS), dtype=torch.float64, device=dev)
    if n == 0:
        return totals[: C + 1]
    lab = labels.long()
    known = (lab >= 0) & (lab < C)
    if conf is not None:
        known &= ~(conf < mc)
    g = torch.where(known, lab, torch.full_like(lab, C))
    if n_live is not None:
        live = torch.arange(n, device=dev) < n_live.long()
        g = torch.where(live, g, torch.full_like(g, C + 1))
    vals = torch.cat(
        [torch.ones(n, 1, dtype=torch.float64, device=dev), X.double()], dim=1
    )
    totals.index_add_(0, g, vals)
    return totals[: C + 1]


# ----------------------------------------------------------------------
# Top talkers: the k largest flows of every class
# ----------------------------------------------------------------------

# the default key of class_top_flows: forward plus reverse instantaneous bytes
# per second, what the summary's "Bytes share" is made of
TOP_FLOW_COLUMNS = (
    _FEATURE_NAMES.index("Forward Instantaneous Bytes per Second"),
    _FEATURE_NAMES.index("Reverse Instantaneous Bytes per Second"),
)
TOP_FLOWS_MAX_K = 64


def top_flow_columns_check(columns):
    """The columns of a key: a non-empty tuple of distinct ints in 0..11, in
    any order (they are added in ascending order).  Returns them sorted."""
    if isinstance(columns, (str, bytes)) or not isinstance(columns, (tuple, list)):
        raise ValueError(f"columns must be a tuple of ints, got {columns!r}")
    cols = []
    for c in columns:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
            raise ValueError(f"columns must be ints, got {c!r}")
        if not 0 <= int(c) < len(_FEATURE_NAMES):
            raise ValueError(f"columns must be in 0..11, got {c}")
        cols.append(int(c))
    if not cols:
        raise ValueError("columns must name at least one column")
    if len(set(cols)) != len(cols):
        raise ValueError(f"columns names a column twice: {tuple(columns)}")
    return tuple(sorted(cols))


def top_flows_k_check(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"k must be an int, got {k!r}")
    if not 1 <= int(k) <= TOP_FLOWS_MAX_K:
        raise ValueError(f"class_top_flows lists 1..{TOP_FLOWS_MAX_K} flows per class, got {k}")
    return int(k)


def class_top_flows_check(X, labels, n_classes, k, columns, conf, min_conf, n_live):
    """Argument rules of class_top_flows, shared by the CPU and GPU bindings:
    class_traffic's for everything the two ops share.  Returns
    (C, k, columns sorted, column bit mask, f32(min_conf) as a float)."""
    try:
        C, mc = class_traffic_check(X, labels, n_classes, conf, min_conf, n_live)
    except ValueError as e:
        raise ValueError(str(e).replace("class_traffic", "class_top_flows")) from None
    k = top_flows_k_check(k)
    cols = top_flow_columns_check(columns)
    if X.shape[0] >= 2**31:
        raise ValueError(f"class_top_flows indexes rows with 32 bits, got {X.shape[0]} rows")
    return C, k, cols, sum(1 << c for c in cols), mc


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
    """Per class and for "unknown", the k live rows with the largest key:
    (rows int32 [C + 1, k], keys f32 [C + 1, k]).

    The group of a row is class_traffic's.  Its key is the f32 sum of
    X[r, c] over ``columns``, added one at a time in ascending column order.
    Within a group the larger key comes first and equal keys go by the lower
    row; +0 and -0 are equal; a NaN key ranks above every number and NaNs tie
    with each other.  Where a group has fewer than k rows the remaining cells
    hold -1 and 0.0.
    """
    C, k, cols, _, mc = class_top_flows_check(
        X, labels, n_classes, k, columns, conf, min_conf, n_live
    )
    n = X.shape[0]
    dev = X.device
    rows = torch.full((C + 1, k), -1, dtype=torch.int32, device=dev)
    keys = torch.zeros(C + 1, k, dtype=torch.float32, device=dev)
    if n_live is not None:
        n = min(n, max(int(n_live[0]), 0))
    if n == 0:
        return rows, keys
    key = X[:n, cols[0]].clone()
    for c in cols[1:]:
        key = key + X[:n, c]
    lab = labels[:n].long()
    known = (lab >= 0) & (lab < C)
    if conf is not None:
        known &= ~(conf[:n] < mc)
    group = torch.where(known, lab, torch.full_like(lab, C))
    nan = torch.isnan(key)
    # what the order compares: -0 becomes +0, a NaN stands above +inf through
    # the second sort; both sorts are stable, so ties keep the lower row first
    value = torch.where(nan, torch.full_like(key, float("inf")), key + 0.0)
    for g in range(C + 1):
        idx = torch.nonzero(group == g).squeeze(1)
        idx = idx[torch.argsort(value[idx], descending=True, stable=True)]
        idx = idx[torch.argsort(nan[idx].to(torch.int8), descending=True, stable=True)]
        idx = idx[:k]
        rows[g, : idx.numel()] = idx.to(torch.int32)
        keys[g, : idx.numel()] = key[idx]
    return rows, keys


# ----------------------------------------------------------------------
# Serve-path feature extraction (CPU oracle of the GPU kernel; mirrors the
# reference Flow update math, traffic_classifier.py:63-96)
# ----------------------------------------------------------------------


def flow_features(cur: torch.Tensor, prev: torch.Tensor, times: torch.Tensor) -> torch.Tensor:
    """counters -> 12-feature rows (mirrors Flow update math,
    traffic_classifier.py:63-96).

    cur/prev: (n,4) cumulative [fwd_pkts, fwd_bytes, rev_pkts, rev_bytes] at
    the latest / previous update of each direction;
    times: (n,6) [tf_cur, tf_prev, tr_cur, tr_prev, t_start, pad].
    Division guards: a zero time delta leaves the rate at 0 (the reference
    skips the update; with prev==cur at creation the result matches).
    """
    d = cur - prev
    df = times[:, 0] - times[:, 1]
    dr = times[:, 2] - times[:, 3]
    lf = times[:, 0] - times[:, 4]
    lr = times[:, 2] - times[:, 4]

    def safe(num, den):
        out = torch.zeros_like(num)
        nz = den != 0
        out[nz] = num[nz] / den[nz]
        return out

    cols = [
        d[:, 0],
        d[:, 1],
        safe(d[:, 0], df),
        safe(cur[:, 0], lf),
        safe(d[:, 1], df),
        safe(cur[:, 1], lf),
        d[:, 2],
        d[:, 3],
        safe(d[:, 2], dr),
        safe(cur[:, 2], lr),
        safe(d[:, 3], dr),
        safe(cur[:, 3], lr),
    ]
    return torch.stack(cols, dim=1).to(torch.float32)


def kmeans_labels(X: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    """Assignment only (predict path; no partial-sum update)."""
    return kmeans_assign(X, centers)[0]
