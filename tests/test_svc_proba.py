"""SVC class probabilities on the CPU: the Platt/coupling oracles of
ops/cpu.py against sklearn, SVC.calibrate and SVC(probability=True).fit, the
checkpoint round trips, and a calibrated SVC through the ensemble, the serve
engine and the CLI.  The kernels are in test_svc_proba_kernels.py."""

import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import cli
from traffic_classifier_sdn_amd.flow.parser import replay
from traffic_classifier_sdn_amd.flow.replay import TelemetryReplaySource
from traffic_classifier_sdn_amd.models import (
    SVC,
    CalibratedSVC,
    SoftVoteEnsemble,
    load_model,
)
from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine
from traffic_classifier_sdn_amd.utils import checkpoint as ckpt
from traffic_classifier_sdn_amd.utils.datasets import load_six_class_dataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")


@pytest.fixture(scope="module")
def six():
    """(X, y, perm): the six-class rows and one seeded permutation of them.
    perm[:1500] fits, perm[1500:2100] tests, perm[2100:5100] calibrates."""
    X, y = load_six_class_dataset()
    return X, y, np.random.RandomState(0).permutation(len(X))


def _from_sklearn(sk):
    return SVC.from_params(
        {
            "kind": "svc",
            "classes": sk.classes_,
            "support_vectors": sk.support_vectors_,
            "dual_coef": sk._dual_coef_,  # libsvm's own signs, also for two classes
            "intercept": sk._intercept_,
            "n_support": sk._n_support,
            "gamma": sk._gamma,
            "probA": sk.probA_,
            "probB": sk.probB_,
        },
        device="cpu",
    )


def _decision_bounds(sk):
    """Per pair: 2 * (m + 1) * 2^-53 * (Sd + |b|), the distance two f64
    summations of that pair's decision value can be apart (see
    test_couple_oracle_matches_sklearn)."""
    dual, ns = np.abs(sk._dual_coef_), sk._n_support
    start = np.concatenate([[0], np.cumsum(ns)])
    C = len(ns)
    out, p = [], 0
    for i in range(C):
        for j in range(i + 1, C):
            sd = dual[j - 1, start[i]:start[i + 1]].sum() + dual[i, start[j]:start[j + 1]].sum()
            m = int(ns[i] + ns[j])
            out.append(2 * (m + 1) * 2.0 ** -53 * (sd + abs(sk._intercept_[p])))
            p += 1
    return np.asarray(out)


@pytest.fixture(scope="module")
def sk_fits(six):
    """{n_classes: (sklearn estimator, our model, test rows)} for 6 and 2."""
    svm = pytest.importorskip("sklearn.svm")
    X, y, perm = six
    tr, te = perm[:1500], perm[1500:2100]
    out = {}
    for C in (6, 2):
        keep = np.unique(y)[:C]
        mtr, mte = np.isin(y[tr], keep), np.isin(y[te], keep)
        sk = svm.SVC(probability=True, random_state=0, decision_function_shape="ovo")
        sk.fit(X[tr][mtr], y[tr][mtr])
        out[C] = (sk, _from_sklearn(sk), X[te][mte])
    return out


@pytest.fixture(scope="module")
def shipped():
    return load_model(os.path.join(MODELS, "SVC.npz"), device="cpu")


@pytest.fixture(scope="module")
def calibrated(shipped, six):
    X, y, perm = six
    rows = perm[2100:5100]
    return shipped.calibrate(X[rows], y[rows])


# ----------------------------------------------------------------------
# oracles against sklearn
# ----------------------------------------------------------------------


@pytest.mark.parametrize("C", [6, 2])
def test_couple_oracle_matches_sklearn(sk_fits, C):
    """ops.cpu.svc_couple on sklearn's OWN decision values against sklearn's
    predict_proba at 1e-12 (measured 4.4e-16): same libsvm arithmetic, only
    exp() may differ in its last bit.

    The model's full path is held to 1e-9 instead, and this is why: its f64
    decision values differ from sklearn's, measured 3.4e-13 here, because
    torch sums the dual * kernel terms of a pair in another order than
    libsvm's serial loop.  A sum of m f64 terms is good to m * 2^-53 *
    sum|term| in whatever order; a kernel value is <= 1, so for a pair with
    m support vectors each side is within (m + 1) * 2^-53 * (Sd + |b|) of
    the exact sum, Sd = sum |dual| over the pair's SVs (_decision_bounds;
    up to 4e-11 here).  A sigmoid's slope is at most |A|/4, which turns
    that into a bound on each pairwise probability; the test asserts both
    from the inputs, and that the second stays below 1e-9.  The coupled
    probabilities are a smooth function of the pairwise ones with
    sensitivity of order one (they are their weighted means at the fixed
    point), so 1e-9 on them asks no less.
    For two classes sklearn's public decision_function is the negative of
    libsvm's, which the sigmoid applies to."""
    sk, model, Xe = sk_fits[C]
    assert isinstance(model, CalibratedSVC) and len(Xe) >= 150
    ref = sk.predict_proba(Xe)
    dec_sk = sk.decision_function(Xe)
    dec_sk = -dec_sk[:, None] if C == 2 else dec_sk
    A, B = torch.from_numpy(sk.probA_), torch.from_numpy(sk.probB_)
    proba, idx, conf = oc.svc_couple(torch.from_numpy(dec_sk), A, B, C)
    err = float(np.abs(proba.numpy() - ref).max())
    print(f"C={C}: couple on sklearn's decisions, max err {err:.3e}")
    assert err <= 1e-12

    dec = model.decision_function(Xe).numpy()
    dec_bound = _decision_bounds(sk)
    dec_err = np.abs(dec - dec_sk).max(axis=0)
    r_bound = float((np.abs(sk.probA_) / 4 * dec_bound).max())
    print(f"C={C}: decisions, max err {dec_err.max():.3e} (bounds up to {dec_bound.max():.3e}); "
          f"pairwise probability bound {r_bound:.3e}")
    assert bool((dec_err <= dec_bound).all())
    assert r_bound <= 1e-9
    got = model.predict_proba(Xe)
    err = float(np.abs(got - ref).max())
    print(f"C={C}: model predict_proba, max err {err:.3e}")
    assert got.dtype == np.float64 and err <= 1e-9
    assert float(np.abs(got.sum(axis=1) - 1.0).max()) <= 1e-12

    p32, idx, conf = model.predict_scores(Xe)
    assert p32.dtype == torch.float32 and conf.dtype == torch.float32 and idx.dtype == torch.int32
    assert torch.equal(idx, model.predict_index(Xe))
    assert torch.equal(conf, p32[torch.arange(len(Xe)), idx.long()])
    assert np.array_equal(model.predict(Xe), sk.predict(Xe))
    labels, c = model.predict_with_confidence(Xe)
    assert np.array_equal(labels, model.predict(Xe)) and np.array_equal(c, conf.numpy())


def test_vote_and_argmax_differ(sk_fits):
    """The confidence is the voted class's probability, not the row maximum:
    the two rules disagree on some rows, here as in sklearn."""
    sk, model, Xe = sk_fits[6]
    proba, idx, conf = model.predict_scores(Xe)
    differ = proba.argmax(dim=1) != idx.long()
    assert bool(differ.any())
    assert bool((conf[differ] < proba.max(dim=1).values[differ]).all())
    assert np.array_equal(sk.predict(Xe) != sk.classes_[sk.predict_proba(Xe).argmax(axis=1)],
                          differ.numpy())


def test_platt_fit_matches_sklearn(shipped, six):
    """platt_fit (libsvm's Newton iteration) against sklearn's
    _sigmoid_calibration (L-BFGS on the same objective and targets) on the
    shipped model's 15 pairs: rtol 1e-4 with denominator max(1, |value|),
    about 100x the 1.3e-6 measured between the two optimisers when this was
    written (this run's figure is printed)."""
    cal = pytest.importorskip("sklearn.calibration")
    if not hasattr(cal, "_sigmoid_calibration"):
        pytest.skip("sklearn.calibration has no _sigmoid_calibration")
    X, y, perm = six
    rows = perm[2100:5100]
    dec = oc.svc_decision(
        torch.from_numpy(X[rows]), shipped.support_vectors_, shipped.dual_coef_,
        shipped.intercept_, shipped.n_support_, shipped.gamma_)
    y_idx = np.searchsorted(np.asarray(shipped.classes_, dtype=str), y[rows].astype(str))
    worst, p = 0.0, 0
    for i in range(6):
        for j in range(i + 1, 6):
            m = (y_idx == i) | (y_idx == j)
            a, b = oc.platt_fit(dec[m, p], torch.from_numpy(y_idx[m] == i))
            ra, rb = cal._sigmoid_calibration(dec[m, p].numpy(), (y_idx[m] == i).astype(float))
            for got, ref in ((a, ra), (b, rb)):
                worst = max(worst, abs(got - ref) / max(1.0, abs(ref)))
            p += 1
    print(f"platt_fit vs _sigmoid_calibration: worst relative difference {worst:.3e}")
    assert worst <= 1e-4


# ----------------------------------------------------------------------
# calibrate on the shipped checkpoint
# ----------------------------------------------------------------------


def test_calibrate_shipped(shipped, calibrated, six, tmp_path):
    X, y, perm = six
    assert type(shipped) is SVC and not hasattr(shipped, "predict_proba")
    assert isinstance(calibrated, CalibratedSVC) and calibrated.kind == "svc"
    assert calibrated.support_vectors_ is shipped.support_vectors_  # shared, not copied
    assert calibrated.probA_.shape == (15,) and bool((calibrated.probA_ < 0).all())
    Xe = X[perm[5100:5900]]
    assert np.array_equal(calibrated.predict(Xe), shipped.predict(Xe))
    path = str(tmp_path / "SVC.npz")
    calibrated.save(path)
    back = load_model(path, device="cpu")
    assert isinstance(back, CalibratedSVC)
    assert torch.equal(back.probA_, calibrated.probA_) and torch.equal(back.probB_, calibrated.probB_)
    assert np.array_equal(back.predict_proba(Xe), calibrated.predict_proba(Xe))
    # the shipped checkpoint itself stays what it was
    assert type(load_model(os.path.join(MODELS, "SVC.npz"), device="cpu")) is SVC
    with pytest.raises(ValueError, match="CalibratedSVC|probA"):
        CalibratedSVC.from_params(shipped.to_params(), device="cpu")


def test_calibrate_needs_both_classes_of_a_pair(shipped, six):
    X, y, perm = six
    rows = perm[2100:5100]
    rows = rows[y[rows] != "quake"]
    with pytest.raises(ValueError, match="quake"):
        shipped.calibrate(X[rows], y[rows])
    with pytest.raises(ValueError, match="not classes"):
        shipped.calibrate(X[rows[:10]], np.asarray(["nope"] * 10, dtype=object))


def test_calibrated_in_ensemble_engine_and_cli(shipped, calibrated, tmp_path, capsys):
    rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device="cpu")
    with pytest.raises(ValueError, match="no class probabilities"):
        SoftVoteEnsemble({"rf": rf, "svc": shipped})
    ens = SoftVoteEnsemble({"rf": rf, "svc": calibrated})
    table = replay(TelemetryReplaySource(seed=7).stream(6))
    assert len(table) > 2
    X = table.feature_matrix(dtype=np.float32)
    assert ens.predict_index(X).shape == (len(table),)

    models = {"rf": rf, "svc": calibrated}
    eng = GpuServeEngine(models, capacity=64, device="cpu", use_graph=False,
                         confidence=True, ensemble=["rf", "svc"])
    plain = GpuServeEngine({"rf": rf, "svc": shipped}, capacity=64, device="cpu", use_graph=False)
    out, ref = eng.classify(table), plain.classify(table)
    np.testing.assert_array_equal(out["svc"], ref["svc"])
    np.testing.assert_array_equal(out["rf"], ref["rf"])
    assert list(eng.confidence) == ["rf", "svc", "ensemble"]
    conf = eng.confidence["svc"]
    assert conf.dtype == np.float32 and conf.shape == (len(table),)
    _, expect = calibrated.predict_with_confidence(X)
    np.testing.assert_array_equal(conf, expect)
    np.testing.assert_array_equal(out["ensemble"], ens.predict_index(X).numpy())

    calibrated.save(str(tmp_path / "SVC.npz"))
    argv = ["svm", "--confidence", "--models-dir", str(tmp_path), "--device", "cpu",
            "--source", "replay", "--replay-polls", "4"]
    assert cli.main(argv) == 0
    assert "Confidence" in capsys.readouterr().out
    argv = ["ensemble", "--members", "Randomforest,svm", "--models-dir", str(tmp_path),
            "--device", "cpu", "--source", "replay", "--replay-polls", "4"]
    assert cli.main(argv) == 0
    capsys.readouterr()


# ----------------------------------------------------------------------
# fit(probability=True)
# ----------------------------------------------------------------------


@pytest.fixture(scope="module")
def small3(six):
    """150 seeded random rows of each of three classes, and 150 others."""
    X, y, _ = six
    rng = np.random.RandomState(0)
    picks = [rng.permutation(np.where(y == c)[0])[:300] for c in ("dns", "game", "ping")]
    tr = np.concatenate([p[:150] for p in picks])
    te = np.concatenate([p[150:] for p in picks])
    return X[tr], y[tr], X[te]


def test_fit_probability(small3):
    """Every A < 0: a sigmoid falls with the decision value whenever a pair's
    cross-validated decisions rank its two classes better than chance, which
    they do on a random sample of these classes (sklearn's fit of the same
    rows has the same signs)."""
    Xtr, ytr, Xte = small3
    a = SVC(device="cpu", probability=True, random_state=0).fit(Xtr, ytr)
    b = SVC(device="cpu", probability=True, random_state=0).fit(Xtr, ytr)
    assert isinstance(a, CalibratedSVC)
    assert a.probA_.shape == (3,) and a.probB_.shape == (3,)
    assert torch.equal(a.probA_, b.probA_) and torch.equal(a.probB_, b.probB_)
    assert bool((a.probA_ < 0).all())
    other = SVC(device="cpu", probability=True, random_state=1).fit(Xtr, ytr)
    assert not torch.equal(other.probA_, a.probA_)  # the seed does fold
    plain = SVC(device="cpu").fit(Xtr, ytr)
    assert type(plain) is SVC
    assert np.array_equal(plain.predict(Xte), a.predict(Xte))  # same SVs: no refit
    proba = a.predict_proba(Xte)
    assert proba.shape == (len(Xte), 3) and float(np.abs(proba.sum(axis=1) - 1).max()) <= 1e-12
    with pytest.raises(NotImplementedError, match="sharded"):
        SVC(device="cpu", probability=True).fit(Xtr, ytr, sharded=True)


def test_fit_fold_with_one_class():
    """A pair with a single row of one class: the folds that hold it out
    train on one class and give +-1 like libsvm, and the fit goes through."""
    rng = np.random.default_rng(5)
    X = np.concatenate([rng.normal(size=(40, 12)), rng.normal(size=(1, 12)) + 4.0])
    y = np.asarray(["a"] * 40 + ["b"], dtype=object)
    m = SVC(device="cpu", gamma=0.05, probability=True).fit(X, y)
    assert isinstance(m, CalibratedSVC)
    assert bool(torch.isfinite(m.probA_).all()) and bool(torch.isfinite(m.probB_).all())


def test_fit_cli_writes_calibrated_checkpoint(tmp_path, capsys):
    """fit --svc-probability writes a checkpoint that loads as a
    CalibratedSVC; without the flag it stays a plain SVC.  (The exit status
    is the accuracy gate's, which a 5 % training share need not meet.)"""
    from traffic_classifier_sdn_amd import fit

    common = ["--algos", "svm", "--device", "cpu", "--test-size", "0.95", "--json"]
    fit.main(common + ["--out", str(tmp_path / "cal"), "--svc-probability"])
    fit.main(common + ["--out", str(tmp_path / "plain")])
    capsys.readouterr()
    cal = load_model(str(tmp_path / "cal" / "SVC.npz"), device="cpu")
    plain = load_model(str(tmp_path / "plain" / "SVC.npz"), device="cpu")
    assert isinstance(cal, CalibratedSVC) and type(plain) is SVC
    assert cal.probA_.shape == (10,)  # five classes in the shipped rows
    assert torch.equal(cal.support_vectors_, plain.support_vectors_)


# ----------------------------------------------------------------------
# sklearn pickles
# ----------------------------------------------------------------------


def test_export_round_trip(calibrated, six, small3, tmp_path):
    """sklearn's predict_proba on the exported estimator against ours at
    1e-9 (the decision values differ by summation order, see above), for the
    calibrated shipped model, which stores no training-row indices, and for
    a two-class fit, where sklearn's public and private signs differ; then
    back through the pickle reader."""
    pytest.importorskip("sklearn.svm")
    X, y, perm = six
    Xe = X[perm[5100:5900]]
    Xtr, ytr, Xte = small3
    two = ytr != "ping"
    binary = SVC(device="cpu", probability=True).fit(Xtr[two], ytr[two])
    for name, model, rows in (("shipped", calibrated, Xe), ("binary", binary, Xte)):
        est = ckpt.params_to_sklearn(model.to_params())
        assert est.probability is True
        dec = est.decision_function(rows)
        assert not np.isnan(dec).any()
        assert np.array_equal(est.predict(rows), model.predict(rows)), name
        err = float(np.abs(est.predict_proba(rows) - model.predict_proba(rows)).max())
        print(f"{name}: exported predict_proba, max err {err:.3e}")
        assert err <= 1e-9, name
        path = str(tmp_path / name)
        model.save(path)  # no .npz: an sklearn pickle
        back = load_model(path, device="cpu")
        assert isinstance(back, CalibratedSVC), name
        assert np.array_equal(back.predict_proba(rows), model.predict_proba(rows)), name
