"""SoftVoteEnsemble through the model, the console table, the serve engine
and the CLI.

conf tolerance against the f64 oracle (the members' own predict_proba,
averaged in f64), 4 * 2^-23 + T * 2^-23: the vote's four fused steps plus
weight roundings (test_ensemble_vote_kernel.py), and the largest member
error, the forest's T * 2^-23 (test_rf_proba_kernel.py), weighted by at most
the whole; the three softmax/vote members are within 2^-23 each, far inside
it.
"""

import io
import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import cli
from traffic_classifier_sdn_amd.flow.parser import replay
from traffic_classifier_sdn_amd.flow.replay import TelemetryReplaySource
from traffic_classifier_sdn_amd.models import SoftVoteEnsemble, load_model
from traffic_classifier_sdn_amd.serve import RealtimeClassifier
from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
MEMBERS = {"rf": "RandomForestClassifier", "gnb": "GaussianNB",
           "lr": "LogisticRegression", "knn": "KNeighbors"}
UNION = ["dns", "game", "ping", "quake", "telnet", "voice"]

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def _load(name, device="cpu"):
    return load_model(os.path.join(MODELS, name + ".npz"), device=device)


def _members(device="cpu", names=MEMBERS):
    return {k: _load(MEMBERS[k], device) for k in names}


def _table(polls=6, seed=7):
    return replay(TelemetryReplaySource(seed=seed).stream(polls))


@pytest.fixture(scope="module")
def ens_cpu():
    return SoftVoteEnsemble(_members())


@pytest.fixture(scope="module")
def oracle(dataset, ens_cpu):
    """(X f32 rows [::3], f64 average of the members' predict_proba on the
    union of classes, number of trees), computed once on the CPU."""
    X = np.asarray(dataset[0][::3], dtype=np.float32)
    avg = np.zeros((X.shape[0], len(UNION)), dtype=np.float64)
    for m, cmap in zip(ens_cpu.members.values(), ens_cpu.colmaps):
        p = m.predict_proba(X)
        p = p.numpy() if isinstance(p, torch.Tensor) else p
        avg[:, cmap] += 0.25 * p.astype(np.float64)
    top2 = np.sort(avg, axis=1)[:, -2:]
    margin = float((top2[:, 1] - top2[:, 0]).min())
    print(f"oracle: smallest top-two margin {margin:.4f}")
    assert margin >= 0.05  # a condition on the input: the labels below are well defined
    return X, avg, len(ens_cpu.members["rf"].trees_)


def _check_against_oracle(ens, oracle):
    X, avg, T = oracle
    idx, conf = ens.predict_index_conf(X)
    assert idx.dtype == torch.int32 and conf.dtype == torch.float32
    assert np.array_equal(idx.cpu().numpy(), avg.argmax(axis=1))
    err = float(np.abs(conf.cpu().numpy().astype(np.float64) - avg.max(axis=1)).max())
    tol = 4 * 2.0 ** -23 + T * 2.0 ** -23
    print(f"conf max err {err:.3e} (tol {tol:.3e})")
    assert err <= tol
    return idx, conf


# ----------------------------------------------------------------------
# model, CPU
# ----------------------------------------------------------------------


def test_union_of_classes(ens_cpu):
    assert list(ens_cpu.classes_) == UNION
    assert len(ens_cpu.members["lr"].classes_) == 4
    assert ens_cpu.colmaps[2] == [0, 2, 4, 5]  # dns, ping, telnet, voice
    assert ens_cpu.weights == [0.25] * 4
    with pytest.raises(NotImplementedError):
        ens_cpu.to_params()


def test_dataset_vote_cpu(dataset, ens_cpu, oracle):
    idx, conf = _check_against_oracle(ens_cpu, oracle)
    X = oracle[0]
    proba = ens_cpu.predict_proba(X)
    assert proba.dtype == torch.float32 and proba.shape == (X.shape[0], 6)
    assert torch.equal(proba.max(dim=1).values, conf)
    assert torch.equal(torch.argmax(proba, dim=1).to(torch.int32), idx)
    y = np.asarray(dataset[1])[::3]
    acc = float((ens_cpu.classes_[idx.numpy()] == y).mean())
    print(f"soft vote accuracy on rows [::3]: {acc:.4f}")
    assert acc > 0.99  # far above its 68 % member


def test_predict_with_confidence_matches_predict(ens_cpu, oracle):
    X = oracle[0][::8]
    labels, conf = ens_cpu.predict_with_confidence(X)
    assert np.array_equal(labels, ens_cpu.predict(X))
    assert conf.dtype == np.float32 and conf.shape == (X.shape[0],)
    assert np.array_equal(conf, ens_cpu.predict_proba(X).max(dim=1).values.numpy())
    assert float(conf.min()) > 0.0 and float(conf.max()) <= 1.0


def test_weights_change_the_vote(oracle):
    X = oracle[0][::8]
    members = _members(names=("rf", "lr"))
    even = SoftVoteEnsemble(members)
    lr_heavy = SoftVoteEnsemble(members, weights=[1, 99])
    assert lr_heavy.weights == [float(np.float32(0.01)), float(np.float32(0.99))]
    a, b = even.predict_index(X), lr_heavy.predict_index(X)
    lr_idx = members["lr"].predict_index(X).long()
    lr_cols = torch.tensor(lr_heavy.colmaps[1])
    assert torch.equal(b.long(), lr_cols[lr_idx]) and not torch.equal(a, b)


@pytest.mark.parametrize("name", ["SVC", "KMeans_Clustering"])
def test_member_without_probabilities_raises(name):
    with pytest.raises(ValueError, match="odd_one"):
        SoftVoteEnsemble({"rf": _load("RandomForestClassifier"), "odd_one": _load(name)})


def test_bad_weights_raise():
    members = _members(names=("rf", "gnb"))
    for w in ([1.0], [1.0, 0.0], [1.0, -2.0], [1.0, float("nan")]):
        with pytest.raises(ValueError):
            SoftVoteEnsemble(members, weights=w)


# ----------------------------------------------------------------------
# console table
# ----------------------------------------------------------------------


def test_realtime_renders_confidence_column(ens_cpu):
    out = io.StringIO()
    rc = RealtimeClassifier(ens_cpu, predict_every=8, out=out, min_confidence=0.6)
    last = None
    for line in TelemetryReplaySource(seed=3).stream(4):
        before = out.tell()
        if rc.feed(line):
            last = (out.getvalue()[before:], rc.parser.table.feature_matrix(dtype=np.float32))
    assert last is not None
    text, X = last
    labels, conf = ens_cpu.predict_with_confidence(X)
    lines = text.splitlines()
    header = [c.strip() for c in lines[1].strip("|").split("|")]
    assert header[-1] == "Confidence" and header[3] == "Traffic Type"
    rows = [[c.strip() for c in l.strip("|").split("|")] for l in lines[3:-1]]
    assert len(rows) == len(labels) > 0
    for i, row in enumerate(rows):
        assert row[3] == (labels[i] if conf[i] >= 0.6 else "unknown")
        assert row[-1] == "%.2f" % conf[i]


# ----------------------------------------------------------------------
# serve engine, CPU
# ----------------------------------------------------------------------


@pytest.mark.parametrize("capacity", [64, 2])  # 2: the over-capacity path
def test_engine_cpu_ensemble(ens_cpu, capacity):
    models = dict(ens_cpu.members)
    models["svc"] = _load("SVC")
    table = _table()
    n = len(table)
    assert n > 2
    kw = dict(capacity=capacity, use_graph=False, device="cpu", confidence=True)
    eng = GpuServeEngine(models, ensemble=list(MEMBERS), **kw)
    off = GpuServeEngine(models, **kw)
    out, ref = eng.classify(table), off.classify(table)
    assert list(ref) == list(models) and list(off.confidence) == ["rf"]
    assert list(out) == list(models) + ["ensemble"]
    assert list(eng.confidence) == ["rf", "ensemble"]
    for name in models:
        np.testing.assert_array_equal(out[name], ref[name])
    np.testing.assert_array_equal(eng.confidence["rf"], off.confidence["rf"])
    X = table.feature_matrix(dtype=np.float32)
    idx, conf = ens_cpu.predict_index_conf(X)
    assert out["ensemble"].dtype == np.int32 and out["ensemble"].shape == (n,)
    assert eng.confidence["ensemble"].dtype == np.float32
    np.testing.assert_array_equal(out["ensemble"], idx.numpy())
    np.testing.assert_array_equal(eng.confidence["ensemble"], conf.numpy())
    assert list(eng.ensemble.classes_) == UNION
    out2 = eng.classify(table)  # static buffers: a second pass gives the same
    np.testing.assert_array_equal(out2["ensemble"], out["ensemble"])
    np.testing.assert_array_equal(eng.confidence["ensemble"], conf.numpy())


def test_engine_cpu_ensemble_without_confidence(ens_cpu):
    models = {k: ens_cpu.members[k] for k in ("rf", "gnb")}
    table = _table()
    eng = GpuServeEngine(models, capacity=64, use_graph=False, device="cpu",
                         ensemble=["gnb", "rf"], ensemble_weights=[1, 3])
    off = GpuServeEngine(models, capacity=64, use_graph=False, device="cpu")
    out, ref = eng.classify(table), off.classify(table)
    assert list(eng.confidence) == ["ensemble"] and off.confidence == {}
    for name in models:
        np.testing.assert_array_equal(out[name], ref[name])
    direct = SoftVoteEnsemble({"gnb": models["gnb"], "rf": models["rf"]}, [1, 3])
    idx, conf = direct.predict_index_conf(table.feature_matrix(dtype=np.float32))
    np.testing.assert_array_equal(out["ensemble"], idx.numpy())
    np.testing.assert_array_equal(eng.confidence["ensemble"], conf.numpy())


def test_engine_rejects_bad_ensembles(ens_cpu):
    models = dict(ens_cpu.members)
    models["svc"] = _load("SVC")
    kw = dict(capacity=8, use_graph=False, device="cpu")
    with pytest.raises(ValueError, match="nobody"):
        GpuServeEngine(models, ensemble=["rf", "nobody"], **kw)
    with pytest.raises(ValueError, match="svc"):
        GpuServeEngine(models, ensemble=["rf", "svc"], **kw)
    with pytest.raises(ValueError):
        GpuServeEngine(models, ensemble=["rf", "gnb"], ensemble_weights=[1.0], **kw)


# ----------------------------------------------------------------------
# CLI
# ----------------------------------------------------------------------


def test_cli_ensemble(capsys):
    rc = cli.main(["ensemble", "--source", "replay", "--replay-polls", "4",
                   "--min-confidence", "0.6", "--device", "cpu"])
    assert rc == 0
    assert "Confidence" in capsys.readouterr().out


def test_cli_ensemble_members_weights_and_stats(capsys):
    rc = cli.main(["ensemble", "--members", "Randomforest,gaussiannb", "--weights", "2,1",
                   "--source", "replay", "--replay-polls", "4", "--confidence", "--stats",
                   "--device", "cpu"])
    assert rc == 0
    cap = capsys.readouterr()
    assert "Confidence" in cap.out and '"mean_confidence"' in cap.err


@pytest.mark.parametrize("extra", [
    ["--members", "Randomforest,svm"],
    ["--members", "Randomforest,kmeans"],
    ["--members", "Randomforest,nosuchmodel"],
    ["--weights", "1,2"],
    ["--weights", "1,1,1,0"],
    ["--weights", "1,1,1,x"],
])
def test_cli_ensemble_rejects(capsys, extra):
    rc = cli.main(["ensemble", "--source", "replay", "--replay-polls", "4", "--device", "cpu"] + extra)
    assert rc == 2
    cap = capsys.readouterr()
    assert cap.out == "" and len(cap.err.strip().splitlines()) == 1


# ----------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
def test_dataset_vote_gpu(oracle):
    ens = SoftVoteEnsemble(_members("cuda"))
    idx, conf = _check_against_oracle(ens, oracle)
    assert idx.is_cuda and conf.is_cuda
    proba = ens.predict_proba(oracle[0])
    assert proba.is_cuda and torch.equal(proba.max(dim=1).values, conf)


@needs_gpu
@pytest.mark.gpu
def test_engine_gpu_graph_ensemble():
    from traffic_classifier_sdn_amd.ops import gpu as og

    shipped = ("RandomForestClassifier", "GaussianNB", "LogisticRegression", "SVC", "KMeans_Clustering")
    models = {n: _load(n, "cuda") for n in shipped}
    names = ["RandomForestClassifier", "GaussianNB", "LogisticRegression"]
    kw = dict(capacity=4096, confidence=True)
    eng = GpuServeEngine(models, use_graph=True, ensemble=names, **kw)
    eager = GpuServeEngine(models, use_graph=False, ensemble=names, **kw)
    off = GpuServeEngine(models, use_graph=True, **kw)
    direct = SoftVoteEnsemble({n: models[n] for n in names})
    for seed in (7, 11):  # the second table replays the captured graph
        table = _table(polls=8, seed=seed)
        n = len(table)
        out, plain, ref = eng.classify(table), eager.classify(table), off.classify(table)
        assert list(out) == list(shipped) + ["ensemble"]
        assert list(eng.confidence) == ["RandomForestClassifier", "ensemble"]
        assert list(ref) == list(shipped) and list(off.confidence) == ["RandomForestClassifier"]
        for name in shipped:
            np.testing.assert_array_equal(out[name], ref[name])
            np.testing.assert_array_equal(plain[name], ref[name])
        np.testing.assert_array_equal(eng.confidence["RandomForestClassifier"],
                                      off.confidence["RandomForestClassifier"])
        assert out["ensemble"].shape == (n,) and eng.confidence["ensemble"].dtype == np.float32
        np.testing.assert_array_equal(out["ensemble"], plain["ensemble"])
        np.testing.assert_array_equal(eng.confidence["ensemble"], eager.confidence["ensemble"])
        X = og.flow_features(*(torch.from_numpy(a).cuda() for a in table.counters_snapshot()))
        idx, conf = direct.predict_index_conf(X)
        np.testing.assert_array_equal(out["ensemble"], idx.cpu().numpy())
        np.testing.assert_array_equal(eng.confidence["ensemble"], conf.cpu().numpy())
    assert eng._graph is not None


@needs_gpu
@pytest.mark.gpu
def test_engine_gpu_knn_member_is_eager_only():
    from traffic_classifier_sdn_amd.ops import gpu as og

    models = _members("cuda", names=("rf", "knn"))
    table = _table()
    eng = GpuServeEngine(models, capacity=256, use_graph=False, ensemble=["rf", "knn"])
    off = GpuServeEngine(models, capacity=256, use_graph=False)
    out, ref = eng.classify(table), off.classify(table)
    for name in models:
        np.testing.assert_array_equal(out[name], ref[name])
    assert list(eng.confidence) == ["ensemble"]
    X = og.flow_features(*(torch.from_numpy(a).cuda() for a in table.counters_snapshot()))
    idx, conf = SoftVoteEnsemble(models).predict_index_conf(X)
    np.testing.assert_array_equal(out["ensemble"], idx.cpu().numpy())
    np.testing.assert_array_equal(eng.confidence["ensemble"], conf.cpu().numpy())
    with pytest.raises(ValueError, match="knn"):
        GpuServeEngine(models, capacity=256, use_graph=True, ensemble=["rf", "knn"])
