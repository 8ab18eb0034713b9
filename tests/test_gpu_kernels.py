"""HIP kernel numerics vs CPU torch oracles (ops.cpu) on identical inputs.
All tests require an MI355X (pytest -m gpu)."""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on CPU boxes
    pytest.skip("no GPU", allow_module_level=True)

from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.ops import gpu as og
from traffic_classifier_sdn_amd.utils.datasets import load_reference_dataset, synthetic_flow_rows

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def X_real():
    X, y = load_reference_dataset()
    return torch.from_numpy(X.astype(np.float32))


@pytest.fixture(scope="module")
def X_syn():
    return torch.from_numpy(synthetic_flow_rows(200_000, seed=3))


def agree(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.cpu() == b.cpu()).float().mean())


def test_gnb_kernel(X_real, X_syn):
    C = 6
    rng = np.random.default_rng(0)
    theta = torch.from_numpy(rng.normal(size=(C, 12)).astype(np.float32)) * 100
    var = torch.from_numpy(rng.uniform(0.5, 100, size=(C, 12)).astype(np.float32))
    prior = torch.full((C,), 1.0 / C)
    for X in (X_real, X_syn):
        ref = oc.gnb_argmax(X, theta, var, prior)
        got = og.gnb_argmax(X.cuda(), theta.cuda(), var.cuda(), prior.cuda())
        assert agree(ref, got) > 0.999


def test_linear_kernel(X_real, X_syn):
    rng = np.random.default_rng(1)
    W = torch.from_numpy(rng.normal(size=(6, 12)).astype(np.float32))
    b = torch.from_numpy(rng.normal(size=(6,)).astype(np.float32))
    for X in (X_real, X_syn):
        ref = oc.linear_argmax(X, W, b)
        got = og.linear_argmax(X.cuda(), W.cuda(), b.cuda())
        assert agree(ref, got) > 0.999


def test_kmeans_kernel(X_syn):
    rng = np.random.default_rng(2)
    K = 6
    centers = torch.from_numpy(
        synthetic_flow_rows(K, seed=5).astype(np.float32)
    )
    ref_l, ref_c, ref_s, ref_i = oc.kmeans_assign(X_syn, centers)
    got_l, got_c, got_s, got_i = og.kmeans_assign(X_syn.cuda(), centers.cuda())
    assert agree(ref_l, got_l) > 0.999
    np.testing.assert_allclose(got_c.cpu().numpy(), ref_c.numpy(), rtol=1e-3)
    np.testing.assert_allclose(got_s.cpu().numpy(), ref_s.numpy(), rtol=1e-3)
    assert float(got_i) == pytest.approx(float(ref_i), rel=1e-3)
    lab2 = og.kmeans_labels(X_syn.cuda(), centers.cuda())
    assert agree(got_l, lab2) == 1.0


def test_rf_kernel_shipped_forest(X_real, X_syn):
    from traffic_classifier_sdn_amd.models import load_model

    m = load_model(os.path.join(REPO, "data", "ref_models", "RandomForestClassifier.npz"), device="cpu")
    forest = m.forest
    for X in (X_real, X_syn):
        ref = oc.rf_argmax(X, forest)
        got = og.rf_argmax(X.cuda(), {k: v for k, v in forest.items()})
        assert agree(ref, got) == 1.0


def test_svc_kernel_shipped_model(X_real):
    from traffic_classifier_sdn_amd.models import load_model

    m = load_model(os.path.join(REPO, "data", "ref_models", "SVC.npz"), device="cpu")
    X = X_real
    ref = oc.svc_predict(
        X, m.support_vectors_.float(), m.dual_coef_.float(), m.intercept_.float(),
        m.n_support_, m.gamma_,
    )
    got = og.svc_predict(
        X.cuda(), m.support_vectors_.float().cuda(), m.dual_coef_.float().cuda(),
        m.intercept_.float().cuda(), m.n_support_.cuda(), m.gamma_,
    )
    assert agree(ref, got) > 0.999


def test_knn_kernel(X_real):
    # oracle: exact f64 direct-difference distances.  The flow dataset has
    # many duplicate rows (ties at distance ~0) and feature magnitudes where
    # the CPU expanded-form f32 GEMM loses ~1e5 absolute precision, so index
    # lists are validated against the f64 k-th-distance boundary rather than
    # element-wise.
    from traffic_classifier_sdn_amd.models import load_model

    m = load_model(os.path.join(REPO, "data", "ref_models", "KNeighbors.npz"), device="cpu")
    Q = X_real[:2000]
    R = m.fit_X_.float()
    y = m.y_
    k = 5
    d64 = torch.cdist(Q.double(), R.double()).pow(2)
    ref_d, ref_i = torch.topk(d64, k, dim=1, largest=False)
    got_d, got_i = og.knn_topk(Q.cuda(), R.cuda(), k)
    got_d = got_d.cpu().double()
    got_i = got_i.cpu().long()
    # every selected neighbour must lie within the true k-th distance bound
    tol = 1e-3 * (1.0 + ref_d[:, -1])
    sel_d64 = torch.gather(d64, 1, got_i)
    assert bool((sel_d64 <= (ref_d[:, -1:] + tol.unsqueeze(1))).all())
    # reported distances match the true distances of the selected indices
    np.testing.assert_allclose(
        got_d.numpy(), sel_d64.numpy(), rtol=1e-3, atol=1.0
    )
    # sorted ascending
    assert bool((got_d[:, 1:] >= got_d[:, :-1] - 1e-3).all())
    # fused vote agrees with the f64-oracle vote almost everywhere
    _, _, got_lab = og.knn_classify(Q.cuda(), R.cuda(), y.cuda(), k, 6)
    ref_lab = oc.knn_vote(ref_i, y, 6)
    assert agree(ref_lab, got_lab.cpu()) > 0.99


def test_gnb_fit_stats_kernel(X_syn):
    y = torch.from_numpy(np.random.default_rng(4).integers(0, 6, X_syn.shape[0]))
    Xd = X_syn.double()
    ref = oc.gnb_fit_stats(Xd, y.long(), 6)
    got = og.gnb_fit_stats(Xd.cuda(), y.cuda(), 6)
    for r, g in zip(ref, got):
        np.testing.assert_allclose(g.cpu().numpy(), r.numpy(), rtol=1e-10)


def test_logistic_grad_kernel(X_syn):
    rng = np.random.default_rng(5)
    X = X_syn[:50_000].double()
    X = (X - X.mean(0)) / (X.std(0) + 1)
    y = torch.from_numpy(rng.integers(0, 6, X.shape[0]))
    W = torch.from_numpy(rng.normal(size=(6, 12)))
    b = torch.from_numpy(rng.normal(size=(6,)))
    ref = oc.logistic_loss_grad(X, y.long(), W, b, l2=1.0)
    got = og.logistic_loss_grad(X.cuda(), y.cuda(), W.cuda(), b.cuda(), l2=1.0)
    assert float(got[0]) == pytest.approx(float(ref[0]), rel=1e-10)
    np.testing.assert_allclose(got[1].cpu().numpy(), ref[1].numpy(), rtol=1e-8)
    np.testing.assert_allclose(got[2].cpu().numpy(), ref[2].numpy(), rtol=1e-8)
    # RAW-scale features + grown weights: the per-row margin exceeds the f64
    # exp underflow range, which a log(exp(t)) formulation turns into -inf
    # (regression: GPU LR fit collapsed to 15% accuracy on real flow rows)
    Xr = X_syn[:50_000].double()
    Wr = torch.from_numpy(rng.normal(size=(6, 12)) * 1e-2)
    ref = oc.logistic_loss_grad(Xr, y.long(), Wr, b, l2=1.0)
    got = og.logistic_loss_grad(Xr.cuda(), y.cuda(), Wr.cuda(), b.cuda(), l2=1.0)
    assert np.isfinite(float(got[0]))
    assert float(got[0]) == pytest.approx(float(ref[0]), rel=1e-9)
    np.testing.assert_allclose(got[1].cpu().numpy(), ref[1].numpy(), rtol=1e-7)


@pytest.mark.gpu
def test_logistic_gpu_fit_accuracy():
    from traffic_classifier_sdn_amd.models import LogisticRegression
    from traffic_classifier_sdn_amd.utils.datasets import load_reference_dataset, train_test_split_ref
    from traffic_classifier_sdn_amd.utils.metrics import accuracy

    X, y = load_reference_dataset()
    Xtr, Xte, ytr, yte = train_test_split_ref(X, y)
    m = LogisticRegression(device="cuda").fit(Xtr, ytr)
    acc = accuracy(yte, m.predict(Xte))
    assert acc > 0.95, acc  # published: 96.47% (CPU path: 99.6%)


def test_flow_features_kernel():
    rng = np.random.default_rng(6)
    n = 10_000
    prev = torch.from_numpy(rng.integers(0, 10_000, (n, 4)).astype(np.float64))
    cur = prev + torch.from_numpy(rng.integers(0, 1000, (n, 4)).astype(np.float64))
    t0 = torch.full((n, 1), 100.0, dtype=torch.float64)
    # [tf_cur, tf_prev, tr_cur, tr_prev, t_start, pad]
    times = torch.cat([t0 + 10, t0 + 9, t0 + 10, t0 + 8, t0, t0 * 0], dim=1)
    # some rows with zero time deltas (division guards)
    times[:100, 1] = times[:100, 0]
    ref = oc.flow_features(cur, prev, times)
    got = og.flow_features(cur.cuda(), prev.cuda(), times.cuda())
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=1e-6)


def test_end_to_end_models_on_gpu(X_real):
    """Every converted reference checkpoint predicts on GPU and agrees with
    the CPU path."""
    from traffic_classifier_sdn_amd.models import load_model

    names = ["LogisticRegression", "GaussianNB", "KMeans_Clustering", "SVC",
             "KNeighbors", "RandomForestClassifier"]
    X = X_real.numpy()
    for name in names:
        path = os.path.join(REPO, "data", "ref_models", name + ".npz")
        cpu_m = load_model(path, device="cpu")
        gpu_m = load_model(path, device="cuda")
        a = cpu_m.predict(X)
        b = gpu_m.predict(X)
        assert (a == b).mean() > 0.999, name


def test_smo_kernels_match_cpu():
    from traffic_classifier_sdn_amd.models.svc_fit import smo_fit_pair

    rng = np.random.default_rng(9)
    X = rng.normal(size=(3000, 12)).astype(np.float32) * 2
    y = np.where(X[:, 0] + 0.5 * X[:, 3] + rng.normal(size=3000) * 0.5 > 0, 1.0, -1.0)
    Xc = torch.from_numpy(X)
    yc = torch.from_numpy(y.astype(np.float32))
    a_cpu, b_cpu, it_cpu = smo_fit_pair(Xc, yc, C=1.0, gamma=0.05, tol=1e-3, max_iter=20000)
    a_gpu, b_gpu, it_gpu = smo_fit_pair(Xc.cuda(), yc.cuda(), C=1.0, gamma=0.05, tol=1e-3, max_iter=20000)
    # same optimisation problem: objective value and intercept agree
    assert b_gpu == pytest.approx(b_cpu, abs=5e-2)
    # decision agreement on the training rows
    def dec(alpha, X_t, b):
        av = (alpha * yc.double().to(alpha.device)).float()
        K = torch.exp(-0.05 * torch.cdist(X_t, X_t) ** 2)
        return K @ av.to(X_t.device) + b
    d_cpu = dec(a_cpu, Xc, b_cpu)
    d_gpu = dec(a_gpu.cpu(), Xc, b_gpu)
    agree_frac = ((d_cpu > 0) == (d_gpu > 0)).float().mean()
    assert float(agree_frac) > 0.995


def test_svc_gpu_fit_accuracy(X_real):
    from traffic_classifier_sdn_amd.models import SVC
    from traffic_classifier_sdn_amd.utils.datasets import load_reference_dataset, train_test_split_ref
    from traffic_classifier_sdn_amd.utils.metrics import accuracy

    X, y = load_reference_dataset()
    Xtr, Xte, ytr, yte = train_test_split_ref(X, y)
    m = SVC(device="cuda").fit(Xtr, ytr)
    acc = accuracy(yte, m.predict(Xte))
    assert acc > 0.80  # published RBF-SVC: 85.01% (6-class; 5 classes here)


@pytest.mark.gpu
def test_knn_mfma_matches_scalar_kernel():
    """MFMA distance-GEMM path (csrc/knn_mfma.hip) vs the scalar kernel on a
    reference set large enough to engage sharding; distances must agree to
    f32 roundoff and selected neighbours must lie inside the scalar k-th
    distance boundary (ties between duplicate rows may reorder)."""
    from traffic_classifier_sdn_amd.ops.gpu import _ext, _knn_cmean
    from traffic_classifier_sdn_amd.utils.datasets import synthetic_flow_rows

    Rn = synthetic_flow_rows(400_000, seed=3)
    Qn = synthetic_flow_rows(4096, seed=4)
    R = torch.from_numpy(Rn).float().cuda().contiguous()
    Q = torch.from_numpy(Qn).float().cuda().contiguous()
    k = 5
    d1, i1 = _ext.knn_topk(Q, R, None, k, 0, 0)
    d2, i2 = _ext.knn_topk_mfma(Q, R, _knn_cmean(R), None, k, 0, 0, 8)
    d1, i1, d2, i2 = d1.cpu(), i1.cpu().long(), d2.cpu(), i2.cpu().long()
    # refined distances are the exact diff-form values: k-th boundary parity
    bound = d1[:, -1] * (1 + 1e-4) + 1e-3
    assert bool((d2 <= bound.unsqueeze(1)).all())
    # and vice versa (the MFMA path found nothing worse than the scalar one)
    bound2 = d2[:, -1] * (1 + 1e-4) + 1e-3
    assert bool((d1 <= bound2.unsqueeze(1)).all())
    # index agreement away from ties
    agree_idx = (i1 == i2).float().mean().item()
    assert agree_idx > 0.99, agree_idx

    # fused vote + idx_base (sharded merge contract)
    y = torch.from_numpy(np.random.default_rng(0).integers(0, 6, size=400_000)).cuda()
    y8 = y.to(torch.uint8).contiguous()
    _, im, labm = _ext.knn_topk_mfma(Q, R, _knn_cmean(R), y8, k, 6, 1000, 8)
    _, is_, labs = _ext.knn_topk(Q, R, y8, k, 6, 1000)
    assert bool((im.min() >= 1000).item())
    assert (labm.cpu() == labs.cpu()).float().mean().item() > 0.99


@pytest.mark.gpu
def test_rf_hist_kernel_matches_cpu():
    from traffic_classifier_sdn_amd.ops import cpu as oc2
    from traffic_classifier_sdn_amd.ops import gpu as og2

    rng = np.random.default_rng(12)
    n, nodes, C = 200_000, 37, 6
    bins = torch.from_numpy(rng.integers(0, 256, (n, 12)).astype(np.uint8))
    y = torch.from_numpy(rng.integers(0, C, n).astype(np.uint8))
    nid = torch.from_numpy(rng.integers(-1, nodes, n).astype(np.int32))
    ref = oc2.rf_hist(bins, y, nid, nodes, C)
    got = og2.rf_hist(bins.cuda(), y.cuda(), nid.cuda(), nodes, C)
    assert torch.equal(got.cpu(), ref)


@pytest.mark.gpu
def test_rf_gpu_hist_fit_accuracy():
    """GPU level-synchronous histogram fit (HIP rf_hist kernel) reaches the
    published RF accuracy."""
    from traffic_classifier_sdn_amd.models import RandomForestClassifier
    from traffic_classifier_sdn_amd.utils.datasets import load_reference_dataset, train_test_split_ref
    from traffic_classifier_sdn_amd.utils.metrics import accuracy

    X, y = load_reference_dataset()
    Xtr, Xte, ytr, yte = train_test_split_ref(X, y)
    m = RandomForestClassifier(n_estimators=100, seed=0, device="cuda").fit(Xtr, ytr)
    acc = accuracy(yte, m.predict(Xte))
    assert acc > 0.995, acc  # published: 0.9987


@pytest.mark.gpu
def test_knn_mfma_edge_shapes():
    """Partial query blocks, ragged tiles, k=8, single shard."""
    from traffic_classifier_sdn_amd.ops.gpu import _ext, _knn_cmean
    from traffic_classifier_sdn_amd.utils.datasets import synthetic_flow_rows

    R = torch.from_numpy(synthetic_flow_rows(150_000 + 37, seed=5)).float().cuda().contiguous()
    Q = torch.from_numpy(synthetic_flow_rows(77, seed=6)).float().cuda().contiguous()
    for k in (1, 5, 8):
        d1, i1 = _ext.knn_topk(Q, R, None, k, 0, 0)
        d2, i2 = _ext.knn_topk_mfma(Q, R, _knn_cmean(R), None, k, 0, 0, 3)
        bound = d1[:, -1] * (1 + 1e-4) + 1e-3
        assert bool((d2 <= bound.unsqueeze(1)).all()), k
        assert (i1.cpu() == i2.cpu()).float().mean().item() > 0.98, k


@pytest.mark.gpu
def test_analysis_runs_on_gpu():
    """PCA / LR-on-2PC / KMeans analysis end-to-end on cuda (C10): the
    non-12-feature LR fit must route to the torch fallback."""
    from traffic_classifier_sdn_amd.analysis import run_analysis

    res = run_analysis(device="cuda")
    assert res["device"].startswith("cuda")
    assert res["lr_accuracy_on_2pc"] > 0.8
    assert len(res["kmeans_mode_assignment"]) == 6


@pytest.mark.gpu
def test_svc_full_ovo_fit_6class_gpu():
    """Full 6-class one-vs-one SVC fit (all 15 pairs, device-fused SMO) on
    stratified synthetic rows — the svc-fit-full bench path (config #3)."""
    from traffic_classifier_sdn_amd.models import SVC
    from traffic_classifier_sdn_amd.utils.datasets import load_six_class_dataset

    X6, y6 = load_six_class_dataset(quake_rows=400, seed=2)
    rng = np.random.default_rng(0)
    idx = rng.permutation(len(X6))
    tr, te = idx[:6000], idx[6000:7500]
    m = SVC(tol=1e-3, max_iter=4000, device="cuda").fit(X6[tr], y6[tr])
    assert len(m.n_iter_) == 15  # all OVO pairs ran
    assert int(m.n_support_.sum()) > 0
    acc = (m.predict(X6[te]).astype(str) == y6[te].astype(str)).mean()
    assert acc > 0.85, acc  # published 6-class SVC reference accuracy: 85.01


@pytest.mark.gpu
def test_svc_predict_large_nsv_accumulation():
    """Regression: the tiled svc_predict kernel accumulated tens of
    thousands of SIGNED near-unit dual terms in one sequential f32 chain —
    at 35K SVs (non-separable pair, alphas at the C bound) rounding
    swallowed the O(1) decision values and flipped 24% of votes at
    n>32768 rows (the tiled-kernel regime).  Now per-tile f32 partials fold
    into f64 accumulators.  Oracle: f64 torch decision."""
    from traffic_classifier_sdn_amd.ops.gpu import _ext

    rng = np.random.default_rng(11)
    C, nsv_per, n = 6, 6000, 150_000  # n > 131072 -> tiled kernel
    nsv = C * nsv_per
    SV = torch.from_numpy(rng.normal(size=(nsv, 12))).float()
    # bounded-alpha-style duals: mostly +-1 (the pathological regime)
    dual = torch.from_numpy(
        rng.choice([-1.0, 1.0], size=(C - 1, nsv)) * rng.uniform(0.5, 1.0, size=(C - 1, nsv))
    ).float()
    n_support = torch.full((C,), nsv_per, dtype=torch.int64)
    svclass = torch.repeat_interleave(torch.arange(C), nsv_per).to(torch.uint8)
    intercept = torch.from_numpy(rng.normal(size=15)).float()
    X = torch.from_numpy(rng.normal(size=(n, 12))).float()
    got = _ext.svc_predict(
        X.cuda(), SV.cuda(), dual.cuda(), svclass.cuda(), intercept.cuda(), 0.05
    ).cpu()
    want = oc.svc_predict(
        X.double(), SV.double(), dual.double(), intercept.double(), n_support, 0.05
    )
    agree = (got == want).float().mean().item()
    assert agree > 0.999, agree


@pytest.mark.gpu
def test_knn_bf16_coarse_pass_recall():
    """Opt-in bf16 coarse-pass KNN (approx=1): candidate pool ranked by the
    bf16 key, every pooled candidate refined with the exact f32 distance.
    Recall vs the exact kernel must be >= 0.999 @ k=5 and the returned
    distances must be the exact f32 values of the returned neighbours."""
    from traffic_classifier_sdn_amd.ops.gpu import _ext, _knn_cmean
    from traffic_classifier_sdn_amd.utils.datasets import synthetic_flow_rows

    R = torch.from_numpy(synthetic_flow_rows(400_000, seed=3)).float().cuda().contiguous()
    Q = torch.from_numpy(synthetic_flow_rows(4096, seed=4)).float().cuda().contiguous()
    k = 5
    d_ex, i_ex = _ext.knn_topk_mfma(Q, R, _knn_cmean(R), None, k, 0, 0, 8, 0)
    d_ap, i_ap = _ext.knn_topk_mfma(Q, R, _knn_cmean(R), None, k, 0, 0, 8, 1)
    ex = i_ex.cpu().numpy()
    ap = i_ap.cpu().numpy()
    recall = np.mean([len(set(ex[i]) & set(ap[i])) / k for i in range(ex.shape[0])])
    assert recall >= 0.999, recall
    # distances of the approx result are the EXACT f32 values (refined)
    Qc, Rc = Q.cpu(), R.cpu()
    sub = np.random.default_rng(0).choice(4096, 200, replace=False)
    for qi in sub:
        for j in range(k):
            ri = int(ap[qi, j])
            want = float(((Qc[qi] - Rc[ri]) ** 2).sum())
            got = float(d_ap[qi, j])
            assert abs(got - want) <= 1e-4 * max(1.0, want), (qi, j)

    # fused vote agreement with the exact path
    y = torch.from_numpy(np.random.default_rng(0).integers(0, 6, size=400_000)).cuda()
    y8 = y.to(torch.uint8).contiguous()
    _, _, lab_ex = _ext.knn_topk_mfma(Q, R, _knn_cmean(R), y8, k, 6, 0, 8, 0)
    _, _, lab_ap = _ext.knn_topk_mfma(Q, R, _knn_cmean(R), y8, k, 6, 0, 8, 1)
    assert (lab_ex.cpu() == lab_ap.cpu()).float().mean().item() > 0.995


@pytest.mark.gpu
def test_smo_wss2_converges():
    """The WSS-2 fused pipeline (measured off by default — see
    profiles/svc_wss2_r02.md) reaches the same optimum as WSS-1."""
    from traffic_classifier_sdn_amd.models.svc_fit import (
        _smo_fused_gpu,
        _smo_intercept,
    )

    rng = np.random.default_rng(9)
    Xn = (rng.normal(size=(3000, 12)) * 2).astype(np.float32)
    yn = np.where(Xn[:, 0] + 0.5 * Xn[:, 3] + rng.normal(size=3000) * 0.5 > 0, 1.0, -1.0)
    X = torch.from_numpy(Xn).cuda()
    yv = torch.from_numpy(yn.astype(np.float32)).cuda()
    res = {}
    for wss2 in (False, True):
        alpha = torch.zeros(3000, dtype=torch.float64, device="cuda")
        grad = -torch.ones(3000, dtype=torch.float64, device="cuda")
        it = _smo_fused_gpu(X, yv, alpha, grad, 1.0, 0.05, 1e-3, 20000, wss2=wss2)
        b = _smo_intercept(yv, alpha, grad, 1.0, "cuda")
        res[wss2] = (alpha.clone(), b, it)
    a1, b1, _ = res[False]
    a2, b2, _ = res[True]
    assert b2 == pytest.approx(b1, abs=5e-2)
    # same optimum: decision agreement on the training rows
    K = torch.exp(-0.05 * torch.cdist(X, X) ** 2).double()
    d1 = K @ (a1 * yv.double()) + b1
    d2 = K @ (a2 * yv.double()) + b2
    assert float(((d1 > 0) == (d2 > 0)).float().mean()) > 0.995


@pytest.mark.gpu
def test_predict_parity_wave_tiled_band(X_real):
    """The RF/SVC wave-per-row kernels now serve up to 131072 rows (cutover
    re-tuned in round 2); pin prediction parity in the 32K-131K band the
    old threshold never exercised, and across the boundary."""
    from traffic_classifier_sdn_amd.models import load_model
    from traffic_classifier_sdn_amd.utils.datasets import synthetic_flow_rows

    for n in (65_536, 140_000):  # wave side / tiled side of the cutover
        X = torch.from_numpy(synthetic_flow_rows(n, seed=21)).float()
        rf = load_model(os.path.join(REPO, "data", "ref_models", "RandomForestClassifier.npz"), device="cuda")
        got = rf.predict_index(X.cuda()).cpu()
        rf_cpu = load_model(os.path.join(REPO, "data", "ref_models", "RandomForestClassifier.npz"), device="cpu")
        want = rf_cpu.predict_index(X)
        assert (got == want).float().mean().item() > 0.9995, n

        svc = load_model(os.path.join(REPO, "data", "ref_models", "SVC.npz"), device="cuda")
        got_s = svc.predict_index(X.cuda()).cpu()
        svc_cpu = load_model(os.path.join(REPO, "data", "ref_models", "SVC.npz"), device="cpu")
        want_s = svc_cpu.predict_index(X)
        assert (got_s == want_s).float().mean().item() > 0.999, n


@pytest.mark.gpu
def test_rf_hist_fsel_mask_planes():
    """rf_hist's mtry mask: selected feature planes match the full scatter,
    unselected planes stay zero (API kept alongside the compact level pass)."""
    rng = np.random.default_rng(3)
    n, nodes, C = 100_000, 17, 6
    bins = torch.from_numpy(rng.integers(0, 256, (n, 12)).astype(np.uint8)).cuda()
    y = torch.from_numpy(rng.integers(0, C, n).astype(np.uint8)).cuda()
    nid = torch.from_numpy(rng.integers(-1, nodes, n).astype(np.int32)).cuda()
    fsel = torch.from_numpy((rng.random((nodes, 12)) < 0.3).astype(np.uint8)).cuda()
    full = og.rf_hist(bins, y, nid, nodes, C)
    masked = og.rf_hist(bins, y, nid, nodes, C, fsel=fsel)
    sel = fsel.bool().cpu()[:, :, None, None]
    assert torch.equal(masked.cpu().masked_select(sel), full.cpu().masked_select(sel))
    assert int(masked.cpu().masked_select(~sel).abs().sum()) == 0


@pytest.mark.gpu
def test_knn_gpu_tolerates_absurd_magnitudes():
    """The HIP brute-force kernels (scalar + MFMA + bf16) must return valid
    labels for hostile feature magnitudes (the ingestion clamp keeps f32
    squared distances finite)."""
    from traffic_classifier_sdn_amd.models import KNeighborsClassifier
    from traffic_classifier_sdn_amd.utils.datasets import synthetic_flow_rows

    rng = np.random.default_rng(0)
    for n_ref, approx in ((50_000, False), (200_000, False), (200_000, True)):
        X = synthetic_flow_rows(n_ref, seed=1)
        y = rng.integers(0, 6, size=n_ref)
        m = KNeighborsClassifier(n_neighbors=5, device="cuda", approx=approx).fit(X, y)
        Q = np.zeros((8, 12))
        Q[0] = 1e38
        Q[1, 3] = np.inf
        Q[2] = -1e38
        Q[3] = np.nan
        pred = m.predict_index(Q).cpu()
        assert int(pred.min()) >= 0 and int(pred.max()) < 6, (n_ref, approx)


@pytest.mark.gpu
def test_knn_topk_rejects_a_k_without_kernel():
    """k = 9 passes the binding's k <= 32 check but has no instantiation:
    an error, not a tensor that no kernel wrote."""
    from traffic_classifier_sdn_amd.ops.gpu import _ext

    Q = torch.zeros(4, 12, device="cuda")
    R = torch.zeros(16, 12, device="cuda")
    with pytest.raises(RuntimeError, match="no kernel for k = 9"):
        _ext.knn_topk(Q, R, None, 9, 0, 0)
