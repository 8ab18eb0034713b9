"""Per-flow confidence through the models, the serve engine, the console
table and the CLI."""

import io
import json
import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import cli
from traffic_classifier_sdn_amd.flow.parser import replay
from traffic_classifier_sdn_amd.flow.replay import TelemetryReplaySource
from traffic_classifier_sdn_amd.models import load_model
from traffic_classifier_sdn_amd.serve import RealtimeClassifier
from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine
from traffic_classifier_sdn_amd.utils.table import Table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
SHIPPED = ("RandomForestClassifier", "GaussianNB", "LogisticRegression", "SVC", "KMeans_Clustering")


def _load(name, device="cpu"):
    return load_model(os.path.join(MODELS, name + ".npz"), device=device)


def _table(polls=6, seed=7):
    return replay(TelemetryReplaySource(seed=seed).stream(polls))


@pytest.fixture(scope="module")
def rf_cpu():
    return _load("RandomForestClassifier")


# ----------------------------------------------------------------------
# models
# ----------------------------------------------------------------------


@pytest.mark.parametrize(
    "name", ["RandomForestClassifier", "GaussianNB", "LogisticRegression", "KNeighbors"])
def test_predict_with_confidence(dataset, name):
    X = np.asarray(dataset[0][::16], dtype=np.float32)
    model = _load(name)
    labels, conf = model.predict_with_confidence(X)
    assert np.array_equal(labels, model.predict(X))
    proba = model.predict_proba(X)
    if isinstance(proba, torch.Tensor):
        proba = proba.numpy()
    assert conf.dtype == np.float32 and conf.shape == (X.shape[0],)
    assert np.array_equal(conf, proba.max(axis=1).astype(np.float32))
    assert float(conf.min()) > 0.0 and float(conf.max()) <= 1.0


def test_rf_index_conf_and_log_proba(dataset, rf_cpu):
    X = np.asarray(dataset[0][::16], dtype=np.float32)
    idx, conf = rf_cpu.predict_index_conf(X)
    assert idx.dtype == torch.int32 and conf.dtype == torch.float32
    assert torch.equal(idx, rf_cpu.predict_index(X))
    proba = rf_cpu.predict_proba(X)
    assert torch.equal(conf, proba.max(dim=1).values)
    logp = rf_cpu.predict_log_proba(X)
    assert torch.equal(logp, torch.log(proba)) and bool((logp <= 0).all())


def test_svc_has_no_confidence(dataset):
    with pytest.raises(NotImplementedError, match="SVC"):
        _load("SVC").predict_with_confidence(np.asarray(dataset[0][:4], dtype=np.float32))


# ----------------------------------------------------------------------
# console table and --stats
# ----------------------------------------------------------------------


def _render_today(table, labels):
    """The six-column table as it is rendered without the new options."""
    t = Table(["Flow ID", "Src MAC", "Dest MAC", "Traffic Type", "Forward Status", "Reverse Status"])
    for i, (meta, (fs, rs)) in enumerate(zip(table.metas(), table.statuses())):
        t.add_row([i, meta.ethsrc, meta.ethdst, labels[i], fs, rs])
    return str(t)


def _serve(model, **kw):
    """Feed a replay stream; returns (text of the last table, parsed last
    --stats line, the flow table, labels and confidence at that pass)."""
    out, err = io.StringIO(), io.StringIO()
    rc = RealtimeClassifier(model, predict_every=8, out=out, stats=True, stats_out=err, **kw)
    last = None
    for line in TelemetryReplaySource(seed=3).stream(4):
        before = out.tell()
        if rc.feed(line):
            X = rc.parser.table.feature_matrix(dtype=np.float32)
            last = (out.getvalue()[before:], X)
    assert last is not None
    text, X = last
    return text, json.loads(err.getvalue().splitlines()[-1]), rc.parser.table, X


STATS_KEYS = ["flows", "records", "predict_ms", "flows_per_sec", "device"]


def test_realtime_defaults_render_todays_table(rf_cpu):
    text, stats, table, X = _serve(rf_cpu, confidence=False, min_confidence=0.0)
    assert text == _render_today(table, rf_cpu.predict(X)) + "\n"
    assert "Confidence" not in text
    assert list(stats) == STATS_KEYS


def test_realtime_confidence_column(rf_cpu):
    text, stats, table, X = _serve(rf_cpu, confidence=True)
    labels, conf = rf_cpu.predict_with_confidence(X)
    lines = text.splitlines()
    header = [c.strip() for c in lines[1].strip("|").split("|")]
    assert header == ["Flow ID", "Src MAC", "Dest MAC", "Traffic Type", "Forward Status",
                      "Reverse Status", "Confidence"]
    rows = [[c.strip() for c in l.strip("|").split("|")] for l in lines[3:-1]]
    assert len(rows) == len(table) > 0
    for i, row in enumerate(rows):
        assert row[3] == labels[i]  # no threshold: labels untouched
        assert row[-1] == "%.2f" % conf[i]
    assert list(stats) == STATS_KEYS + ["mean_confidence", "unknown"]
    assert stats["mean_confidence"] == pytest.approx(float(conf.mean()))
    assert stats["unknown"] == 0


def test_realtime_min_confidence_marks_unknown(rf_cpu):
    text, stats, table, _ = _serve(rf_cpu, min_confidence=1.01)  # implies the column
    lines = text.splitlines()
    assert "Confidence" in lines[1]
    rows = [[c.strip() for c in l.strip("|").split("|")] for l in lines[3:-1]]
    assert len(rows) == len(table) > 0
    assert all(row[3] == "unknown" for row in rows)
    assert stats["unknown"] == len(table)


# ----------------------------------------------------------------------
# serve engine
# ----------------------------------------------------------------------


@pytest.mark.parametrize("capacity", [64, 2])  # 2: the over-capacity path
def test_engine_cpu_confidence(rf_cpu, capacity):
    models = {"rf": rf_cpu, "gnb": _load("GaussianNB")}
    table = _table()
    assert len(table) > 2
    eng = GpuServeEngine(models, capacity=capacity, use_graph=False, device="cpu", confidence=True)
    plain = GpuServeEngine(models, capacity=capacity, use_graph=False, device="cpu")
    out, ref = eng.classify(table), plain.classify(table)
    assert plain.confidence == {}
    for name in models:
        np.testing.assert_array_equal(out[name], ref[name])
    assert list(eng.confidence) == ["rf"]  # models with predict_index_conf
    conf = eng.confidence["rf"]
    assert conf.dtype == np.float32 and conf.shape == (len(table),)
    _, expect = rf_cpu.predict_with_confidence(table.feature_matrix(dtype=np.float32))
    np.testing.assert_array_equal(conf, expect)
    out2 = eng.classify(table)  # static buffers: a second pass gives the same
    np.testing.assert_array_equal(out2["rf"], out["rf"])
    np.testing.assert_array_equal(eng.confidence["rf"], conf)


# ----------------------------------------------------------------------
# CLI
# ----------------------------------------------------------------------


def test_cli_min_confidence(capsys):
    rc = cli.main(["Randomforest", "--source", "replay", "--replay-polls", "4",
                   "--min-confidence", "0.9", "--device", "cpu"])
    assert rc == 0
    assert "Confidence" in capsys.readouterr().out


def test_cli_rejects_confidence_for_svm(capsys):
    rc = cli.main(["svm", "--source", "replay", "--replay-polls", "4", "--confidence",
                   "--device", "cpu"])
    assert rc == 2
    cap = capsys.readouterr()
    assert cap.out == "" and len(cap.err.strip().splitlines()) == 1


# ----------------------------------------------------------------------
# GPU: captured graph
# ----------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
def test_engine_gpu_graph_confidence():
    from traffic_classifier_sdn_amd.ops import gpu as og

    models = {n: _load(n, device="cuda") for n in SHIPPED}
    rf = models["RandomForestClassifier"]
    T = len(rf.trees_)
    eng = GpuServeEngine(models, capacity=4096, use_graph=True, confidence=True)
    off = GpuServeEngine(models, capacity=4096, use_graph=True)
    eager = GpuServeEngine(models, capacity=4096, use_graph=False, confidence=True)
    for seed in (7, 11):  # the second call replays the captured graph
        table = _table(polls=8, seed=seed)
        n = len(table)
        out, ref, plain = eng.classify(table), off.classify(table), eager.classify(table)
        for name in SHIPPED:
            assert out[name].shape == (n,)
            np.testing.assert_array_equal(out[name], ref[name])
            np.testing.assert_array_equal(out[name], plain[name])
        assert list(eng.confidence) == ["RandomForestClassifier"]
        conf = eng.confidence["RandomForestClassifier"]
        assert conf.dtype == np.float32 and conf.shape == (n,)
        np.testing.assert_array_equal(conf, eager.confidence["RandomForestClassifier"])
        X = og.flow_features(*(torch.from_numpy(a).cuda() for a in table.counters_snapshot()))
        labels, expect = rf.predict_with_confidence(X)
        assert np.array_equal(labels, rf.classes_[out["RandomForestClassifier"]])
        assert float(np.abs(conf - expect).max()) <= T * 2.0 ** -23
    assert eng._graph is not None
