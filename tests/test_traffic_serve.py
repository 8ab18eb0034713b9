"""Per-class traffic accounting through the serve engine, the classify loop,
its --stats lines and the Prometheus gauges."""

import io
import json
import os
import socket

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import cli
from traffic_classifier_sdn_amd.flow.parser import PollStreamParser
from traffic_classifier_sdn_amd.flow.replay import SynthFlowSpec, TelemetryReplaySource
from traffic_classifier_sdn_amd.models import load_model
from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.serve import RealtimeClassifier
from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
VOTERS = ["RandomForestClassifier", "GaussianNB", "LogisticRegression"]

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def _load(name, device="cpu"):
    return load_model(os.path.join(MODELS, name + ".npz"), device=device)


@pytest.fixture(scope="module")
def voters_cpu():
    return {n: _load(n) for n in VOTERS}


@pytest.fixture(scope="module")
def rf_cpu(voters_cpu):
    return voters_cpu["RandomForestClassifier"]


LATE = [
    SynthFlowSpec("00:00:00:00:00:09", "00:00:00:00:00:0a", 40.0, 120.0, 35.0, 400.0),
    SynthFlowSpec("00:00:00:00:00:0b", "00:00:00:00:00:0c", 8.0, 70.0, 6.0, 600.0),
]


def _polls(polls=8, late_at=4, seed=0):
    """The flow table after each poll: four flows, six from poll ``late_at``."""
    first = TelemetryReplaySource(seed=seed)
    late = TelemetryReplaySource(specs=LATE, seed=seed + 100,
                                 t0=first.t + late_at * first.interval)
    parser = PollStreamParser()
    for k in range(polls):
        for line in first.poll() + (late.poll() if k >= late_at else []):
            parser.feed(line)
        yield parser.table


def _oracle(table, labels, C, conf=None, min_conf=0.0):
    X = torch.from_numpy(np.ascontiguousarray(table.feature_matrix(dtype=np.float32)))
    lab = torch.from_numpy(np.asarray(labels).astype(np.int32))
    if conf is not None:
        conf = torch.from_numpy(np.asarray(conf, dtype=np.float32))
    return oc.class_traffic(X, lab, C, conf, min_conf).numpy()


# ----------------------------------------------------------------------
# serve engine, CPU
# ----------------------------------------------------------------------


@pytest.mark.parametrize("capacity", [64, 4])  # 4: the fifth flow crosses it
@pytest.mark.parametrize("key", ["ensemble", "GaussianNB", "smoothed"])
def test_engine_cpu_totals_follow_the_oracle(voters_cpu, capacity, key):
    kw = dict(capacity=capacity, use_graph=False, device="cpu", ensemble=VOTERS)
    if key == "smoothed":
        kw.update(smooth=0.25)
    eng = GpuServeEngine(voters_cpu, traffic=key, **kw)
    plain = GpuServeEngine(voters_cpu, **kw)
    C = len(voters_cpu["GaussianNB"].classes_)
    assert eng.traffic is None
    assert eng.traffic_classes == [str(c) for c in voters_cpu["GaussianNB"].classes_] + ["unknown"]
    sizes = []
    for table in _polls():
        out, ref = eng.classify(table), plain.classify(table)
        sizes.append(len(table))
        assert list(out) == list(ref)
        for name in ref:  # nothing that was there changes
            np.testing.assert_array_equal(out[name], ref[name])
        assert list(eng.confidence) == list(plain.confidence)
        t = eng.traffic
        assert t.dtype == np.float64 and t.shape == (C + 1, 13)
        np.testing.assert_array_equal(t, _oracle(table, out[key], C))
        assert t[:, 0].sum() == len(table)
        np.testing.assert_array_equal(t[:C, 0], np.bincount(out[key], minlength=C))
    assert sizes == [4] * 4 + [6] * 4
    # a smaller table after a larger one: the rows past it are not counted
    small = next(_polls(polls=1, seed=3))
    out = eng.classify(small)
    np.testing.assert_array_equal(eng.traffic, _oracle(small, out[key], C))
    assert eng.traffic[:, 0].sum() == 4


@pytest.mark.parametrize("capacity", [64, 4])
def test_engine_cpu_min_confidence(voters_cpu, capacity):
    kw = dict(capacity=capacity, use_graph=False, device="cpu", ensemble=VOTERS)
    thr = 0.75
    eng = GpuServeEngine(voters_cpu, traffic="ensemble", traffic_min_confidence=thr, **kw)
    allu = GpuServeEngine(voters_cpu, traffic="ensemble", traffic_min_confidence=2.0, **kw)
    rf = GpuServeEngine(voters_cpu, confidence=True, traffic="RandomForestClassifier",
                        traffic_min_confidence=thr, **kw)
    C = len(eng.traffic_classes) - 1
    below = 0
    for table in _polls():
        out = eng.classify(table)
        conf = eng.confidence["ensemble"]
        np.testing.assert_array_equal(
            eng.traffic, _oracle(table, out["ensemble"], C, conf, thr))
        assert eng.traffic[C, 0] == (conf < np.float32(thr)).sum()
        below += int(eng.traffic[C, 0])
        allu.classify(table)
        assert allu.traffic[C, 0] == len(table) and not allu.traffic[:C].any()
        np.testing.assert_array_equal(allu.traffic[C], _oracle(table, out["ensemble"], C).sum(axis=0))
        out = rf.classify(table)
        np.testing.assert_array_equal(
            rf.traffic,
            _oracle(table, out["RandomForestClassifier"], C,
                    rf.confidence["RandomForestClassifier"], thr))
    assert below > 0  # the threshold did send flows to "unknown"


def test_engine_refusals(voters_cpu):
    kw = dict(use_graph=False, device="cpu")
    models = dict(voters_cpu)
    models["KMeans"] = _load("KMeans_Clustering")
    with pytest.raises(ValueError, match="KMeans"):
        GpuServeEngine(models, traffic="KMeans", **kw)
    with pytest.raises(ValueError, match="nobody"):
        GpuServeEngine(models, traffic="nobody", **kw)
    with pytest.raises(ValueError, match="ensemble="):
        GpuServeEngine(models, traffic="ensemble", **kw)
    with pytest.raises(ValueError, match="smooth="):
        GpuServeEngine(models, ensemble=VOTERS, traffic="smoothed", **kw)
    # a confidence threshold on a key that carries no confidence
    with pytest.raises(ValueError, match="confidence"):
        GpuServeEngine(models, traffic="GaussianNB", traffic_min_confidence=0.5, **kw)
    with pytest.raises(ValueError, match="confidence"):  # confidence=False
        GpuServeEngine(models, traffic="RandomForestClassifier", traffic_min_confidence=0.5, **kw)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            GpuServeEngine(models, ensemble=VOTERS, traffic="ensemble",
                           traffic_min_confidence=bad, **kw)
    GpuServeEngine(models, traffic="GaussianNB", **kw)
    GpuServeEngine(models, confidence=True, traffic="RandomForestClassifier",
                   traffic_min_confidence=0.5, **kw)


# the instance attributes of an engine without traffic=, as they were before
# the option existed (h_nlive .. _smooth_n only with smooth=)
TODAY = {
    "models", "capacity", "device", "use_graph", "h_cur", "h_prev", "h_times", "d_cur",
    "d_prev", "d_times", "d_labels", "h_labels", "_conf_models", "d_conf", "h_conf",
    "ensemble", "_ens_members", "smoother", "_vote_keys", "_conf_keys", "confidence",
    "_graph", "last_latency_s",
}
TODAY_SMOOTH = TODAY | {"h_nlive", "_h_nlive_np", "d_nlive", "_smooth_table", "_smooth_n"}


def test_without_traffic_the_engine_is_todays(voters_cpu):
    kw = dict(capacity=16, use_graph=False, device="cpu", confidence=True)
    plain = GpuServeEngine(voters_cpu, ensemble=VOTERS, **kw)
    smooth = GpuServeEngine(voters_cpu, ensemble=VOTERS, smooth=0.25, **kw)
    table = next(_polls(polls=1))
    out = plain.classify(table)
    assert list(out) == VOTERS + ["ensemble"]
    assert list(plain.confidence) == ["RandomForestClassifier", "ensemble"]
    assert list(smooth.classify(table)) == VOTERS + ["ensemble", "smoothed"]
    assert list(smooth.confidence) == ["RandomForestClassifier", "ensemble", "smoothed"]
    assert set(vars(plain)) == TODAY
    assert set(vars(smooth)) == TODAY_SMOOTH
    assert plain.traffic is None and plain.traffic_classes is None
    # with traffic= the live count is staged also without smooth=
    eng = GpuServeEngine(voters_cpu, ensemble=VOTERS, traffic="ensemble", **kw)
    assert {"h_nlive", "d_nlive"} <= set(vars(eng))


# ----------------------------------------------------------------------
# serve engine, GPU: the captured graph against the plain launches
# ----------------------------------------------------------------------


@pytest.fixture(scope="module")
def voters_gpu():
    return {n: _load(n, device="cuda") for n in VOTERS}


@needs_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("key, kw", [
    ("ensemble", dict(traffic_min_confidence=0.75)),
    ("GaussianNB", dict()),
    ("smoothed", dict(smooth=0.25)),
])
def test_engine_gpu_graph_equals_eager(voters_gpu, key, kw):
    kw = dict(capacity=256, ensemble=VOTERS, traffic=key, **kw)
    graph = GpuServeEngine(voters_gpu, use_graph=True, **kw)
    eager = GpuServeEngine(voters_gpu, use_graph=False, **kw)
    C = len(graph.traffic_classes) - 1
    thr = kw.get("traffic_min_confidence", 0.0)
    for k, table in enumerate(_polls()):  # one table object, growing
        if k not in (2, 6, 7):  # four flows, then six: 6 and 7 replay the capture
            continue
        n = len(table)
        assert n == (4 if k < 4 else 6)
        out, ref = graph.classify(table), eager.classify(table)
        for name in ref:
            np.testing.assert_array_equal(out[name], ref[name], err_msg=f"poll {k} {name}")
        assert graph.traffic.shape == (C + 1, 13) and graph.traffic.dtype == np.float64
        np.testing.assert_array_equal(graph.traffic, eager.traffic, err_msg=f"poll {k}")
        known = out[key][graph.confidence[key] >= np.float32(thr)] if thr else out[key]
        np.testing.assert_array_equal(graph.traffic[:C, 0], np.bincount(known, minlength=C))
        assert graph.traffic[:, 0].sum() == n
        # the device's own features, summed by the oracle on the host
        X = graph_features(graph, n)
        conf = torch.from_numpy(graph.confidence[key]) if thr else None
        want = oc.class_traffic(X, torch.from_numpy(out[key]), C, conf, thr).numpy()
        np.testing.assert_allclose(graph.traffic, want, rtol=n * 2.0 ** -52, atol=0.0)
    assert graph._graph is not None


def graph_features(engine, n):
    """The features of the engine's last pass, recomputed from its staged
    counters by the same kernel."""
    from traffic_classifier_sdn_amd import ops

    return ops.flow_features(engine.d_cur, engine.d_prev, engine.d_times)[:n].cpu().contiguous()


@needs_gpu
@pytest.mark.gpu
def test_engine_gpu_smaller_table_counts_only_live_rows(voters_gpu):
    """Rows past the live count hold the counters of the poll before."""
    eng = GpuServeEngine(voters_gpu, capacity=256, use_graph=True, traffic="GaussianNB")
    eng.classify(list(_polls())[-1])
    big = eng.traffic.copy()
    assert big[:, 0].sum() == 6
    small = next(_polls(polls=1, seed=3))
    out = eng.classify(small)
    C = len(eng.traffic_classes) - 1
    assert eng.traffic[:, 0].sum() == 4
    np.testing.assert_array_equal(eng.traffic[:C, 0], np.bincount(out["GaussianNB"], minlength=C))
    X = graph_features(eng, 4)
    want = oc.class_traffic(X, torch.from_numpy(out["GaussianNB"]), C).numpy()
    np.testing.assert_allclose(eng.traffic, want, rtol=4 * 2.0 ** -52, atol=0.0)


@needs_gpu
@pytest.mark.gpu
def test_engine_gpu_crosses_its_capacity(voters_gpu):
    kw = dict(capacity=4, ensemble=VOTERS, traffic="ensemble")
    graph = GpuServeEngine(voters_gpu, use_graph=True, **kw)
    eager = GpuServeEngine(voters_gpu, use_graph=False, **kw)
    C = len(graph.traffic_classes) - 1
    for k, table in enumerate(_polls()):
        out, ref = graph.classify(table), eager.classify(table)
        np.testing.assert_array_equal(out["ensemble"], ref["ensemble"])
        np.testing.assert_array_equal(graph.traffic, eager.traffic, err_msg=f"poll {k}")
        np.testing.assert_array_equal(
            graph.traffic[:C, 0], np.bincount(out["ensemble"], minlength=C))
        assert graph.traffic[:, 0].sum() == len(table)


# ----------------------------------------------------------------------
# RealtimeClassifier, --stats, the CLI
# ----------------------------------------------------------------------

HEAD = ["Traffic Type", "Flows", "Fwd pkt/s", "Fwd B/s", "Rev pkt/s", "Rev B/s", "Bytes share"]


def _rows(block):
    return [[c.strip() for c in l.strip("|").split("|")] for l in block if l.startswith("|")]


def _split(text):
    """(flow-table lines, summary-table lines) of one pass's output."""
    lines = text.splitlines()
    at = next(i for i, l in enumerate(lines) if "Bytes share" in l) - 1
    return lines[:at], lines[at:]


def _passes(model, polls=6, seed=0, **kw):
    out, stats = io.StringIO(), io.StringIO()
    rc = RealtimeClassifier(model, out=out, stats=True, stats_out=stats, **kw)
    passes = []
    for line in TelemetryReplaySource(seed=seed).stream(polls):
        before = out.tell()
        if rc.feed(line):
            passes.append((out.getvalue()[before:],
                           rc.parser.table.feature_matrix(dtype=np.float32)))
    assert len(passes) >= 4
    return rc, passes, out.getvalue(), [json.loads(l) for l in stats.getvalue().splitlines()]


@pytest.mark.parametrize("kw", [dict(), dict(min_confidence=0.75), dict(smooth=0.3)])
def test_summary_table_and_stats(rf_cpu, kw):
    rc, passes, text, stats = _passes(rf_cpu, summary=True, **kw)
    _, _, plain_text, plain_stats = _passes(rf_cpu, **kw)
    classes = [str(c) for c in rf_cpu.classes_] + ["unknown"]
    assert rc.traffic_classes == classes
    kept = []
    unknown = 0
    for (block, X), line in zip(passes, stats):
        flows, summary = _split(block)
        kept += flows
        rows = _rows(summary)
        assert rows[0] == HEAD
        assert [r[0] for r in rows[1:]] == classes  # one row per class and unknown
        shown = [r[3] for r in _rows(flows)[1:]]
        assert len(shown) == len(X)
        idx = torch.tensor([classes.index(s) for s in shown], dtype=torch.int32)
        want = oc.class_traffic(
            torch.from_numpy(np.ascontiguousarray(X)), idx, len(classes) - 1).numpy()
        total = want[:, 5].sum() + want[:, 11].sum()
        for g, r in enumerate(rows[1:]):
            assert int(r[1]) == shown.count(r[0])
            assert r[2:6] == ["%.1f" % want[g, c] for c in (3, 5, 9, 11)]
            share = (want[g, 5] + want[g, 11]) / total if total else 0.0
            assert r[6] == "%.1f%%" % (100.0 * share)
        unknown += shown.count("unknown")
        # the --stats line carries the same numbers
        assert list(line["traffic"]) == classes
        for g, name in enumerate(classes):
            assert line["traffic"][name] == {
                "flows": int(want[g, 0]), "fwd_pps": want[g, 3], "fwd_Bps": want[g, 5],
                "rev_pps": want[g, 9], "rev_Bps": want[g, 11],
            }
    assert (unknown > 0) == ("min_confidence" in kw)
    # everything else is what it is without the option
    assert "\n".join(kept) + "\n" == plain_text
    for line, plain in zip(stats, plain_stats):
        line.pop("traffic")
        for timing in ("predict_ms", "flows_per_sec"):
            line.pop(timing), plain.pop(timing)
        assert line == plain and "traffic" not in plain


def test_summary_off_is_byte_identical(rf_cpu, capsys):
    _, _, off, _ = _passes(rf_cpu, summary=False)
    _, _, absent, _ = _passes(rf_cpu)
    assert off == absent and "Bytes share" not in off
    args = ["Randomforest", "--source", "replay", "--replay-polls", "6", "--device", "cpu"]
    assert cli.main(args) == 0
    assert capsys.readouterr().out == off
    _, _, on, _ = _passes(rf_cpu, summary=True)
    assert cli.main(args + ["--summary"]) == 0
    assert capsys.readouterr().out == on


def test_summary_with_no_bytes_has_zero_shares():
    from traffic_classifier_sdn_amd.serve import render_traffic_summary

    totals = np.zeros((3, 13))
    totals[0, 0] = 2
    rows = _rows(render_traffic_summary(["a", "b", "unknown"], totals).splitlines())
    assert rows[1] == ["a", "2", "0.0", "0.0", "0.0", "0.0", "0.0%"]
    assert [r[6] for r in rows[1:]] == ["0.0%"] * 3


def test_summary_kmeans_uses_its_cluster_names():
    km = _load("KMeans_Clustering")
    rc, passes, _, stats = _passes(km, summary=True)
    names = getattr(km, "cluster_label_names_", None)
    if names is None:
        from traffic_classifier_sdn_amd.utils.schema import CLASS_NAMES as names
    want = list(dict.fromkeys(str(n) for n in names))
    assert rc.traffic_classes == [n for n in want if n != "unknown"] + ["unknown"]
    for (block, X), line in zip(passes, stats):
        flows, summary = _split(block)
        shown = [r[3] for r in _rows(flows)[1:]]
        for r in _rows(summary)[1:]:
            assert int(r[1]) == shown.count(r[0])


class _Named:
    """A model of ``names`` whose every flow is of class ``now``."""

    device = "cpu"

    def __init__(self, names):
        self.classes_ = np.asarray(names, dtype=object)
        self.now = names[0]

    def predict(self, X):
        return np.asarray([self.now] * len(X), dtype=object)


def test_summary_refuses_more_than_eight_classes():
    with pytest.raises(ValueError, match="2..8"):
        RealtimeClassifier(_Named([f"c{i}" for i in range(9)]), out=io.StringIO(), summary=True)
    RealtimeClassifier(_Named([f"c{i}" for i in range(9)]), out=io.StringIO())
    RealtimeClassifier(_Named([f"c{i}" for i in range(8)]), out=io.StringIO(), summary=True)


def test_prometheus_rate_gauges():
    prom = pytest.importorskip("prometheus_client")
    registry = prom.CollectorRegistry()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    model = _Named(["bulk", "voice"])
    rc = RealtimeClassifier(model, out=io.StringIO(), prometheus_port=port, summary=True,
                            prometheus_registry=registry)

    def value(metric, label, direction):
        return registry.get_sample_value(metric, {"label": label, "direction": direction})

    metrics = ("tcsdn_class_bytes_per_second", "tcsdn_class_packets_per_second")
    lines = TelemetryReplaySource(seed=1).stream(8)
    passes = 0
    for line in lines:
        if not rc.feed(line):
            continue
        passes += 1
        rates = rc.traffic
        for metric in metrics:  # every class and unknown, both directions
            for label in ("bulk", "voice", "unknown"):
                for direction in ("forward", "reverse"):
                    assert value(metric, label, direction) is not None
        here, gone = ("bulk", "voice") if model.now == "bulk" else ("voice", "bulk")
        g = rc.traffic_classes.index(here)
        assert value(metrics[0], here, "forward") == rates[g, 5]
        assert value(metrics[0], here, "reverse") == rates[g, 11]
        assert value(metrics[1], here, "forward") == rates[g, 3]
        assert value(metrics[1], here, "reverse") == rates[g, 9]
        if passes >= 2:
            assert rates[g, 5] > 0  # the class that is here does carry bytes
        for metric in metrics:  # the class that left reads 0, not its last value
            assert value(metric, gone, "forward") == 0.0 and value(metric, gone, "reverse") == 0.0
            assert value(metric, "unknown", "forward") == 0.0
        assert registry.get_sample_value("tcsdn_class_flows", {"label": here}) == len(rc.parser.table)
        model.now = "voice" if passes >= 2 else "bulk"
    assert passes >= 4 and model.now == "voice"


def test_prometheus_without_summary_has_no_rate_gauges():
    prom = pytest.importorskip("prometheus_client")
    from traffic_classifier_sdn_amd.utils.prom import PromServeMetrics

    registry = prom.CollectorRegistry()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    PromServeMetrics(port, addr="127.0.0.1", registry=registry)
    names = {m.name for m in registry.collect()}
    assert "tcsdn_class_flows" in names
    assert not any("per_second" in n for n in names)
