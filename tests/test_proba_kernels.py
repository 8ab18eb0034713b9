"""Class-probability kernels (csrc/ensemble_kernels.hip: gnb_proba,
linear_proba, knn_vote_proba) against the CPU oracles in ops/cpu.py.

Tolerance of the two softmax kernels, atol = 2^-23 on a probability:

Kernel and oracle both work in f64 from the same parameters and the same f32
rows, but not in the same order (the kernel multiplies by a host-derived
1/var where the oracle divides, fuses its multiply-adds, and sums in feature
order where torch reduces in its own).  A logit or log-likelihood is a sum
of 12 products plus a constant: about 14 f64 roundings, each relative to a
partial sum that is at most S in magnitude, so the two sides differ by at
most about 14 * 2^-53 * S.  A probability is exp(s_c - max) / sum, so an
absolute score error e changes it by a relative 2e at most (numerator and
denominator), and probabilities are <= 1: 28 * 2^-53 * S absolute.  The f32
store adds half an ulp of a value <= 1, 2^-24, on each side's own rounding
of a value that differs by the above.  With S <= 2^24 the f64 part is
28 * 2^-29 < 2^-24, so the total stays below 2^-23.

S per model:
  logistic  max over rows and classes of sum_j |x_j w_cj| + |b_c|
  NB        max over rows of |ll_max| + 745: a class whose log-likelihood
            lies more than 745 below the row's best has exp() == 0 on both
            sides whatever its error, so only scores within 745 of the best
            matter
Each test computes S from the f64 oracle and asserts S <= 2^24 on its inputs
(shipped models on dataset rows: about 1.0e5 for logistic, 134 + 745 for NB).

The KNN vote is count / k in f32 on both sides: bit for bit.
"""

import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd.ops import cpu as oc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

ROWS = (1, 255, 256, 257, 1500)  # 256 rows per block: partial, full, second block
CLASSES = (2, 4, 6, 8)
ATOL = 2.0 ** -23
S_MAX = 2.0 ** 24


def _og():
    from traffic_classifier_sdn_amd.ops import gpu as og

    return og


def _caps(monkeypatch):
    """Runs the body with the default grid, then with two blocks: several
    passes of the grid-stride loop and a partial last tile."""
    for cap in (None, 2):
        if cap is None:
            monkeypatch.delenv("TCSDN_PROBA_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("TCSDN_PROBA_BLOCKS", str(cap))
        yield cap


def _rows(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).normal(size=(n, 12)).astype(np.float32))


def _gnb_params(C, seed):
    rng = np.random.default_rng(seed)
    theta = torch.from_numpy(rng.normal(size=(C, 12)))
    var = torch.from_numpy(rng.uniform(0.5, 2.0, size=(C, 12)))
    prior = rng.uniform(0.5, 1.5, size=C)
    return theta, var, torch.from_numpy(prior / prior.sum())


def _linear_params(C, seed):
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.normal(size=(C, 12)).astype(np.float32)),
            torch.from_numpy(rng.normal(size=C).astype(np.float32)))


def _gnb_scale(X, theta, var, prior):
    ll = oc.gnb_joint_loglik(X.double(), theta.double(), var.double(), prior.double())
    return float(ll.max(dim=1).values.abs().max()) + 745.0


def _linear_scale(X, W, b):
    return float(((X.double().abs() @ W.double().abs().T) + b.double().abs()).max())


def _check_proba(got, ref, tag):
    C = ref.shape[1]
    assert got.dtype == torch.float32 and got.shape == ref.shape, tag
    got = got.cpu()
    err = float((got.double() - ref.double()).abs().max())
    row_err = float((got.double().sum(dim=1) - 1.0).abs().max())
    print(f"{tag}: max err {err:.3e} (atol {ATOL:.3e}), row-sum err {row_err:.3e}")
    assert err <= ATOL, tag
    assert row_err <= C * ATOL, tag


# ----------------------------------------------------------------------
# softmax kernels, synthetic parameters
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
def test_gnb_proba(monkeypatch, C):
    og = _og()
    theta, var, prior = _gnb_params(C, 10 + C)
    X = _rows(max(ROWS), 20 + C)
    S = _gnb_scale(X, theta, var, prior)
    assert S <= S_MAX
    ref = oc.gnb_proba(X, theta, var, prior)
    assert ref.dtype == torch.float32
    dev = [t.cuda() for t in (theta, var, prior)]
    Xd = X.cuda()
    for cap in _caps(monkeypatch):
        for n in ROWS:
            _check_proba(og.gnb_proba(Xd[:n], *dev), ref[:n], f"gnb C {C} S {S:.0f} cap {cap} n {n}")


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
def test_linear_proba(monkeypatch, C):
    og = _og()
    W, b = _linear_params(C, 30 + C)
    X = _rows(max(ROWS), 40 + C)
    S = _linear_scale(X, W, b)
    assert S <= S_MAX
    ref = oc.linear_proba(X, W, b)
    assert ref.dtype == torch.float32
    Wd, bd, Xd = W.cuda(), b.cuda(), X.cuda()
    for cap in _caps(monkeypatch):
        for n in ROWS:
            _check_proba(og.linear_proba(Xd[:n], Wd, bd), ref[:n],
                         f"linear C {C} S {S:.1f} cap {cap} n {n}")


@needs_gpu
@pytest.mark.gpu
def test_nine_classes_raise():
    og = _og()
    X = _rows(8, 50).cuda()
    theta, var, prior = (t.cuda() for t in _gnb_params(9, 51))
    with pytest.raises(RuntimeError):
        og.gnb_proba(X, theta, var, prior)
    W, b = (t.cuda() for t in _linear_params(9, 52))
    with pytest.raises(RuntimeError):
        og.linear_proba(X, W, b)
    idx = torch.zeros(8, 3, dtype=torch.int32).cuda()
    y = torch.zeros(16, dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError):
        og.knn_vote_proba(idx, y, 9)
    with pytest.raises(RuntimeError):
        og.knn_vote_proba(idx, y, 1)


# ----------------------------------------------------------------------
# softmax kernels, shipped checkpoints on dataset rows
# ----------------------------------------------------------------------


def _load(name, device):
    from traffic_classifier_sdn_amd.models import load_model

    return load_model(os.path.join(MODELS, name + ".npz"), device=device)


def _shipped_reference(name, X):
    """(f32 oracle, f64 probabilities, S) of a shipped model on CPU."""
    m = _load(name, "cpu")
    Xt = torch.from_numpy(X)
    if name == "GaussianNB":
        args = (m.theta_, m.var_, m.class_prior_)
        ref = oc.gnb_proba(Xt, *args)
        p64 = torch.softmax(oc.gnb_joint_loglik(Xt.double(), *args), dim=1)
        S = _gnb_scale(Xt, *args)
    else:
        args = (m.coef_, m.intercept_)
        ref = oc.linear_proba(Xt, *args)
        p64 = torch.softmax(oc.linear_logits(Xt.double(), args[0].double(), args[1].double()), dim=1)
        S = _linear_scale(Xt, *args)
    return ref, p64, S


@pytest.mark.parametrize("name", ["GaussianNB", "LogisticRegression"])
def test_shipped_oracle_scale_and_gaps(dataset, name):
    """What the GPU comparison below rests on: S within the tolerance's
    range, and no row whose two best classes are closer than 2^-20, so the
    argmax check there leaves no row out."""
    X = np.asarray(dataset[0][::16], dtype=np.float32)
    ref, p64, S = _shipped_reference(name, X)
    top2 = torch.topk(p64, 2, dim=1).values
    gap = float((top2[:, 0] - top2[:, 1]).min())
    print(f"{name}: S {S:.4g}, smallest top-two gap {gap:.4f}")
    assert S <= S_MAX
    assert gap > 2.0 ** -20
    m = _load(name, "cpu")
    got = m.predict_proba_device(X)
    assert got.dtype == torch.float32 and torch.equal(got, ref)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["GaussianNB", "LogisticRegression"])
def test_shipped_proba(monkeypatch, dataset, name):
    X = np.asarray(dataset[0][::16], dtype=np.float32)
    ref, p64, S = _shipped_reference(name, X)
    assert S <= S_MAX
    m = _load(name, "cuda")
    top2 = torch.topk(p64, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2.0 ** -20
    assert bool(clear.all())
    for cap in _caps(monkeypatch):
        got = m.predict_proba_device(X)
        assert got.is_cuda
        _check_proba(got, ref, f"{name} S {S:.4g} cap {cap}")
        labels = m.predict_index(X).cpu()
        assert torch.equal(torch.argmax(got, dim=1).cpu()[clear].to(torch.int32), labels[clear])


# ----------------------------------------------------------------------
# KNN vote fractions
# ----------------------------------------------------------------------


def _knn_case(n, k, C, seed, nr=300):
    rng = np.random.default_rng(seed)
    idx = torch.from_numpy(rng.integers(0, nr, size=(n, k)).astype(np.int32))
    # trailing padding, as the top-k kernels leave it: 0..k-1 entries of a
    # row, never all of them
    pad = rng.integers(0, k, size=n)
    idx[torch.arange(k).unsqueeze(0) >= torch.from_numpy(k - pad).unsqueeze(1)] = -1
    y = torch.from_numpy(rng.integers(0, C, size=nr).astype(np.uint8))
    return idx, y


def test_knn_vote_proba_oracle():
    idx = torch.tensor([[0, 1, 2], [2, -1, -1], [3, 3, -1]], dtype=torch.int32)
    y = torch.tensor([0, 1, 1, 2], dtype=torch.uint8)
    got = oc.knn_vote_proba(idx, y, 3)
    third = np.float32(1) / np.float32(3)
    want = torch.tensor([[third, np.float32(2) / np.float32(3), 0], [0, 1, 0], [0, 0, 1]],
                        dtype=torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    with pytest.raises(ValueError):
        oc.knn_vote_proba(idx, y, 9)


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 6, 8])
@pytest.mark.parametrize("k", [1, 3, 5, 8])
def test_knn_vote_proba(monkeypatch, k, C):
    og = _og()
    for cap in _caps(monkeypatch):
        for n in (1, 257):
            idx, y = _knn_case(n, k, C, 100 * k + C + n)
            assert k == 1 or n == 1 or bool((idx < 0).any())
            ref = oc.knn_vote_proba(idx, y, C)
            got = og.knn_vote_proba(idx.cuda(), y.cuda(), C)
            assert got.dtype == torch.float32 and got.shape == (n, C)
            assert torch.equal(got.cpu(), ref), f"k {k} C {C} cap {cap} n {n}"
            # labels held as int64, as the models keep them
            got64 = og.knn_vote_proba(idx.cuda(), y.long().cuda(), C)
            assert torch.equal(got64.cpu(), ref)


def test_knn_shipped_proba_cpu(dataset):
    X = np.asarray(dataset[0][::64], dtype=np.float32)
    m = _load("KNeighbors", "cpu")
    got = m.predict_proba_device(X)
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy(), m.predict_proba(X).astype(np.float32))


@needs_gpu
@pytest.mark.gpu
def test_knn_shipped_proba(dataset):
    X = np.asarray(dataset[0][::64], dtype=np.float32)
    m = _load("KNeighbors", "cuda")
    got = m.predict_proba_device(X)
    assert got.is_cuda and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), m.predict_proba(X).astype(np.float32))
    assert torch.equal(torch.argmax(got, dim=1).to(torch.int32), m.predict_index(X))


def test_sharded_knn_has_no_device_proba(dataset):
    m = _load("KNeighbors", "cpu")
    m.sharded_ = True
    with pytest.raises(NotImplementedError):
        m.predict_proba_device(np.asarray(dataset[0][:4], dtype=np.float32))
