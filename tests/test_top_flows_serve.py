"""The K largest flows per class through the serve engine, the classify
loop, its --stats lines and the CLI."""

import io
import json
import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import cli
from traffic_classifier_sdn_amd.flow.parser import PollStreamParser
from traffic_classifier_sdn_amd.flow.replay import (
    SynthFlowSpec, TelemetryReplaySource, default_specs,
)
from traffic_classifier_sdn_amd.models import IsolationForest, load_model
from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.serve import RealtimeClassifier
from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine
from traffic_classifier_sdn_amd.utils.datasets import load_six_class_dataset

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
# a flow that none of the six classes describes (pps x bytes per packet)
BULK = SynthFlowSpec("00:00:00:00:01:01", "00:00:00:00:01:02", 8000.0, 1400.0, 4000.0, 64.0)


def _polls(polls=8, late_at=4, seed=0, first_specs=None):
    """The flow table after each poll: four flows, six from poll ``late_at``."""
    first = TelemetryReplaySource(specs=first_specs, seed=seed)
    late = TelemetryReplaySource(specs=LATE, seed=seed + 100,
                                 t0=first.t + late_at * first.interval)
    parser = PollStreamParser()
    for k in range(polls):
        for line in first.poll() + (late.poll() if k >= late_at else []):
            parser.feed(line)
        yield parser.table


def _features(table):
    return torch.from_numpy(np.ascontiguousarray(table.feature_matrix(dtype=np.float32)))


def _oracle(table, labels, C, k, conf=None, min_conf=0.0, columns=oc.TOP_FLOW_COLUMNS):
    lab = torch.from_numpy(np.asarray(labels).astype(np.int32))
    if conf is not None:
        conf = torch.from_numpy(np.asarray(conf, dtype=np.float32))
    rows, rates = oc.class_top_flows(_features(table), lab, C, k, columns, conf, min_conf)
    return rows.numpy(), rates.numpy()


def _check(eng, table, labels, C, k, **kw):
    rows, rates = _oracle(table, labels, C, k, **kw)
    assert eng.top_flows.dtype == np.int32 and eng.top_flows.shape == (C + 1, k)
    assert eng.top_flow_rates.dtype == np.float32 and eng.top_flow_rates.shape == (C + 1, k)
    np.testing.assert_array_equal(eng.top_flows, rows)
    np.testing.assert_array_equal(eng.top_flow_rates, rates)
    # every live flow is listed once when k allows it, and no dead slot ever
    listed = eng.top_flows[eng.top_flows >= 0]
    assert len(set(listed.tolist())) == len(listed) and (listed < len(table)).all()


# ----------------------------------------------------------------------
# serve engine, CPU
# ----------------------------------------------------------------------


@pytest.mark.parametrize("capacity", [64, 4])  # 4: the fifth flow crosses it
@pytest.mark.parametrize("key, K", [("ensemble", 2), ("GaussianNB", 1), ("smoothed", 64)])
def test_engine_cpu_lists_follow_the_oracle(voters_cpu, capacity, key, K):
    kw = dict(capacity=capacity, use_graph=False, device="cpu", ensemble=VOTERS, traffic=key)
    if key == "smoothed":
        kw.update(smooth=0.25)
    eng = GpuServeEngine(voters_cpu, top_flows=K, **kw)
    plain = GpuServeEngine(voters_cpu, **kw)
    C = len(voters_cpu["GaussianNB"].classes_)
    assert eng.top_flows is None and eng.top_flow_rates is None
    for table in _polls():
        out, ref = eng.classify(table), plain.classify(table)
        assert list(out) == list(ref)
        for name in ref:  # nothing that was there changes
            np.testing.assert_array_equal(out[name], ref[name])
        assert list(eng.confidence) == list(plain.confidence)
        for name in plain.confidence:
            np.testing.assert_array_equal(eng.confidence[name], plain.confidence[name])
        np.testing.assert_array_equal(eng.traffic, plain.traffic)
        _check(eng, table, out[key], C, K)
        if K == 64:  # room for all: every flow under its own class
            for g in range(C):
                assert sorted(eng.top_flows[g][eng.top_flows[g] >= 0]) == \
                    np.flatnonzero(out[key] == g).tolist()
    assert plain.top_flows is None and plain.top_flow_rates is None
    # a smaller table after a larger one lists no dead slot
    small = next(_polls(polls=1, seed=3))
    out = eng.classify(small)
    _check(eng, small, out[key], C, K)
    assert eng.top_flows.max() < 4


@pytest.mark.parametrize("capacity", [64, 4])
def test_engine_cpu_low_confidence_is_listed_as_unknown(voters_cpu, capacity):
    kw = dict(capacity=capacity, use_graph=False, device="cpu", ensemble=VOTERS,
              traffic="ensemble", top_flows=3)
    thr = 0.75
    eng = GpuServeEngine(voters_cpu, traffic_min_confidence=thr, **kw)
    allu = GpuServeEngine(voters_cpu, traffic_min_confidence=2.0, **kw)
    C = len(eng.traffic_classes) - 1
    below = 0
    for table in _polls():
        out = eng.classify(table)
        conf = eng.confidence["ensemble"]
        _check(eng, table, out["ensemble"], C, 3, conf=conf, min_conf=thr)
        low = set(np.flatnonzero(conf < np.float32(thr)).tolist())
        unknown = set(eng.top_flows[C][eng.top_flows[C] >= 0].tolist())
        assert unknown <= low and len(unknown) == min(3, len(low))
        assert not low & set(eng.top_flows[:C].ravel().tolist())
        below += len(low)
        allu.classify(table)
        assert (allu.top_flows[:C] == -1).all() and (allu.top_flows[C] >= 0).sum() == 3
    assert below > 0  # the threshold did send flows to "unknown"


def test_engine_cpu_other_columns(voters_cpu):
    kw = dict(capacity=64, use_graph=False, device="cpu", traffic="GaussianNB", top_flows=4)
    eng = GpuServeEngine(voters_cpu, top_flows_columns=(8, 2), **kw)
    C = len(eng.traffic_classes) - 1
    for table in _polls(polls=6):
        out = eng.classify(table)
        _check(eng, table, out["GaussianNB"], C, 4, columns=(2, 8))


@pytest.fixture(scope="module")
def detector():
    X, _ = load_six_class_dataset()
    rows = np.random.RandomState(0).permutation(len(X))[::2]
    return IsolationForest(device="cpu").fit(X[rows])


@pytest.mark.parametrize("capacity", [64, 4])
def test_engine_cpu_novel_flows_are_listed_as_unknown(rf_cpu, detector, capacity):
    # halfway between the fitted threshold and the bulk flow's score
    # (tests/test_isolation_forest.py, SERVE_THRESHOLD)
    kw = dict(capacity=capacity, use_graph=False, device="cpu", traffic="rf", top_flows=2,
              novelty=detector, novelty_threshold=0.735)
    eng = GpuServeEngine({"rf": rf_cpu}, **kw)
    C = len(rf_cpu.classes_)
    src = TelemetryReplaySource(specs=default_specs() + [BULK], seed=0)
    parser = PollStreamParser()
    for k in range(6):
        for line in src.poll():
            parser.feed(line)
        out = eng.classify(parser.table)
        masked = np.where(eng.novel, -1, out["rf"])
        _check(eng, parser.table, masked, C, 2)
        if k == 0:
            continue  # the first poll has no rates yet
        assert eng.novel.tolist() == [False] * 4 + [True]
        assert eng.top_flows[C].tolist() == [4, -1]  # the bulk flow, under unknown alone
        assert 4 not in eng.top_flows[:C]
        X = parser.table.feature_matrix(dtype=np.float32)
        assert eng.top_flow_rates[C, 0] == X[4, 4] + X[4, 10]


def test_engine_refusals(voters_cpu):
    kw = dict(use_graph=False, device="cpu")
    with pytest.raises(ValueError, match="traffic="):
        GpuServeEngine(voters_cpu, top_flows=3, **kw)
    with pytest.raises(ValueError, match="top_flows="):
        GpuServeEngine(voters_cpu, traffic="GaussianNB", top_flows_columns=(4,), **kw)
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError):
            GpuServeEngine(voters_cpu, traffic="GaussianNB", top_flows=bad, **kw)
    for bad in ((), (4, 4), (12,), (-1, 4), (4.0,)):
        with pytest.raises(ValueError):
            GpuServeEngine(voters_cpu, traffic="GaussianNB", top_flows=3,
                           top_flows_columns=bad, **kw)
    GpuServeEngine(voters_cpu, traffic="GaussianNB", top_flows=64, top_flows_columns=(0, 11), **kw)


def test_without_top_flows_the_engine_is_todays(voters_cpu):
    kw = dict(capacity=16, use_graph=False, device="cpu", ensemble=VOTERS, traffic="ensemble")
    plain = GpuServeEngine(voters_cpu, **kw)
    eng = GpuServeEngine(voters_cpu, top_flows=2, **kw)
    table = next(_polls(polls=1))
    plain.classify(table), eng.classify(table)
    assert set(vars(eng)) - set(vars(plain)) == {
        "_top_k", "_top_columns", "d_top", "h_top", "top_flows", "top_flow_rates"}
    assert not set(vars(plain)) - set(vars(eng))


# ----------------------------------------------------------------------
# serve engine, GPU: the captured graph against the CPU engine
# ----------------------------------------------------------------------


@needs_gpu
@pytest.mark.gpu
def test_engine_gpu_graph_equals_the_cpu_engine(voters_cpu):
    voters_gpu = {n: _load(n, device="cuda") for n in VOTERS}
    kw = dict(capacity=64, ensemble=VOTERS, traffic="ensemble", top_flows=3)
    graph = GpuServeEngine(voters_gpu, use_graph=True, **kw)
    cpu = GpuServeEngine(voters_cpu, use_graph=False, device="cpu", **kw)
    for k, table in enumerate(_polls()):  # one table object, growing from four flows to six
        out, ref = graph.classify(table), cpu.classify(table)
        np.testing.assert_array_equal(out["ensemble"], ref["ensemble"], err_msg=f"poll {k}")
        np.testing.assert_array_equal(graph.top_flows, cpu.top_flows, err_msg=f"poll {k}")
        np.testing.assert_array_equal(graph.top_flow_rates, cpu.top_flow_rates, err_msg=f"poll {k}")
        # three of every class that has as many, all of a smaller one
        assert (graph.top_flows >= 0).sum() == graph.traffic[:, 0].clip(max=3).sum()
    assert graph._graph is not None
    small = next(_polls(polls=1, seed=3))  # a smaller table: no slot of the larger one
    out, ref = graph.classify(small), cpu.classify(small)
    np.testing.assert_array_equal(graph.top_flows, cpu.top_flows)
    np.testing.assert_array_equal(graph.top_flow_rates, cpu.top_flow_rates)
    assert graph.top_flows.max() < 4


# ----------------------------------------------------------------------
# RealtimeClassifier, --stats, the CLI
# ----------------------------------------------------------------------

HEAD = ["Traffic Type", "Flow ID", "Src MAC", "Dest MAC", "B/s", "Share of class"]


def _rows(block):
    return [[c.strip() for c in l.strip("|").split("|")] for l in block if l.startswith("|")]


def _split(text):
    """(flow-table, summary-table, top-flows-table lines) of one pass's output."""
    lines = text.splitlines()
    at = next(i for i, l in enumerate(lines) if "Bytes share" in l) - 1
    top = next(i for i, l in enumerate(lines) if "Share of class" in l) - 1
    assert at < top
    return lines[:at], lines[at:top], lines[top:]


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


@pytest.mark.parametrize("kw", [dict(), dict(min_confidence=0.75)])
def test_top_flows_table_and_stats(rf_cpu, kw):
    rc, passes, text, stats = _passes(rf_cpu, summary=True, top=2, **kw)
    _, _, plain_text, plain_stats = _passes(rf_cpu, summary=True, **kw)
    classes = [str(c) for c in rf_cpu.classes_] + ["unknown"]
    kept = []
    listed = 0
    for (block, X), line in zip(passes, stats):
        flows, summary, top = _split(block)
        kept += flows + summary
        shown = {int(r[0]): r for r in _rows(flows)[1:]}  # Flow ID -> its line above
        rows = _rows(top)
        assert rows[0] == HEAD
        idx = torch.tensor([classes.index(shown[i][3]) for i in range(len(X))], dtype=torch.int32)
        Xt = torch.from_numpy(np.ascontiguousarray(X))
        want_rows, want_rates = oc.class_top_flows(Xt, idx, len(classes) - 1, 2)
        totals = oc.class_traffic(Xt, idx, len(classes) - 1).numpy()
        want = []
        for g, name in enumerate(classes):  # classes with no flows have no line
            for r, v in zip(want_rows[g].tolist(), want_rates[g].tolist()):
                if r < 0:
                    continue
                assert v == float(X[r, 4] + X[r, 10])  # B/s is the flow's feature sum
                class_bytes = totals[g, 5] + totals[g, 11]
                share = v / class_bytes if class_bytes else 0.0
                want.append([name, str(r), shown[r][1], shown[r][2], "%.1f" % v,
                             "%.1f%%" % (100.0 * share)])
        assert rows[1:] == want
        for r in rows[1:]:  # every listed flow carries that class in the flow table
            assert shown[int(r[1])][3] == r[0]
        for name in classes:  # at most two per class, largest first
            rates = [float(r[4]) for r in rows[1:] if r[0] == name]
            assert len(rates) <= 2 and rates == sorted(rates, reverse=True)
        listed += len(rows) - 1
        # the --stats line carries the same lists, padding left out
        assert list(line["top_flows"]) == classes
        for g, name in enumerate(classes):
            assert line["top_flows"][name] == [
                [r, v] for r, v in zip(want_rows[g].tolist(), want_rates[g].tolist()) if r >= 0]
    assert listed > 0
    np.testing.assert_array_equal(rc.top_flows, want_rows.numpy())
    np.testing.assert_array_equal(rc.top_flow_rates, want_rates.numpy())
    # everything else is what it is without the option
    assert "\n".join(kept) + "\n" == plain_text
    for line, plain in zip(stats, plain_stats):
        line.pop("top_flows")
        for timing in ("predict_ms", "flows_per_sec"):
            line.pop(timing), plain.pop(timing)
        assert line == plain and "top_flows" not in plain


def test_top_needs_summary(rf_cpu):
    with pytest.raises(ValueError, match="summary"):
        RealtimeClassifier(rf_cpu, out=io.StringIO(), top=2)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            RealtimeClassifier(rf_cpu, out=io.StringIO(), summary=True, top=bad)
    rc = RealtimeClassifier(rf_cpu, out=io.StringIO(), summary=True)
    assert rc.top is None and rc.top_flows is None and rc.top_flow_rates is None


def test_cli_top(rf_cpu, capsys):
    args = ["Randomforest", "--source", "replay", "--replay-polls", "6", "--device", "cpu"]
    _, _, on, _ = _passes(rf_cpu, summary=True, top=2)
    assert cli.main(args + ["--summary", "--top", "2"]) == 0
    got = capsys.readouterr()
    assert got.out == on and "Share of class" in got.out
    assert cli.main(args + ["--top", "2"]) == 2
    got = capsys.readouterr()
    assert got.out == "" and got.err.startswith("ERROR:") and "summary" in got.err
    assert cli.main(args + ["--summary", "--top", "65"]) == 2
    assert capsys.readouterr().err.startswith("ERROR:")
