"""Per-flow smoothing through FlowSmoother, the serve engine, the console
table and the CLI, and what it buys: fewer label changes per flow."""

import io
import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import cli
from traffic_classifier_sdn_amd.flow.parser import PollStreamParser
from traffic_classifier_sdn_amd.flow.replay import SynthFlowSpec, TelemetryReplaySource
from traffic_classifier_sdn_amd.models import FlowSmoother, SoftVoteEnsemble, load_model
from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.serve import RealtimeClassifier
from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine
from traffic_classifier_sdn_amd.utils.table import Table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
VOTERS = ["RandomForestClassifier", "GaussianNB", "LogisticRegression"]
ALPHA, MARGIN = 0.25, 1.0 / 16.0

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


def _polls(polls=10, late_at=5, seed=0):
    """The flow table after each poll: the four default flows, joined by two
    more from poll ``late_at`` on (the table is the same object throughout)."""
    first = TelemetryReplaySource(seed=seed)
    late = TelemetryReplaySource(specs=LATE, seed=seed + 100,
                                 t0=first.t + late_at * first.interval)
    parser = PollStreamParser()
    for k in range(polls):
        for line in first.poll() + (late.poll() if k >= late_at else []):
            parser.feed(line)
        yield parser.table


# ----------------------------------------------------------------------
# FlowSmoother
# ----------------------------------------------------------------------


def test_flow_smoother_owns_its_state():
    sm = FlowSmoother(3, 2, 0.5, 0.125)
    assert sm.capacity == 2 and sm.state.shape == (2, 3) and sm.held.tolist() == [-1, -1]
    assert sm.state.dtype == torch.float32 and sm.held.dtype == torch.int32
    p = torch.tensor([[0.5, 0.25, 0.25], [0.125, 0.125, 0.75]])
    label, conf = sm.update(p)
    assert label.tolist() == [0, 2] and conf.tolist() == [0.5, 0.75]
    assert sm.ensure_capacity(2) is False
    assert sm.ensure_capacity(3) is True and sm.capacity >= 3
    assert torch.equal(sm.state[:2], p) and sm.held[:3].tolist() == [0, 2, -1]
    assert not bool(sm.state[2:].any())
    # the history came along: the next update averages rows 0 and 1
    q = torch.tensor([[0.25, 0.5, 0.25], [0.75, 0.125, 0.125], [0.25, 0.25, 0.5]])
    label, conf = sm.update(q)
    assert sm.state[:3].tolist() == [[0.375, 0.375, 0.25], [0.4375, 0.125, 0.4375], [0.25, 0.25, 0.5]]
    assert label.tolist() == [0, 2, 2] and conf.tolist() == [0.375, 0.4375, 0.5]
    state, held = sm.state, sm.held
    sm.reset()
    assert sm.state is state and sm.held is held  # the buffers stay
    assert not bool(state.any()) and bool((held == -1).all())
    with pytest.raises(ValueError):
        sm.update(torch.full((sm.capacity + 1, 3), 1 / 3))


@pytest.mark.parametrize("kw", [
    dict(n_classes=1), dict(n_classes=9), dict(capacity=0), dict(alpha=0.0), dict(alpha=1.5),
    dict(alpha=float("nan")), dict(switch_margin=-0.1), dict(switch_margin=float("inf")),
])
def test_flow_smoother_refuses(kw):
    args = dict(n_classes=3, capacity=4, alpha=0.5, switch_margin=0.0)
    args.update(kw)
    with pytest.raises(ValueError):
        FlowSmoother(**args)


# ----------------------------------------------------------------------
# serve engine, CPU: against the oracle driven by hand
# ----------------------------------------------------------------------


@pytest.mark.parametrize("capacity", [64, 4])  # 4: the sixth flow crosses it
def test_engine_cpu_smoothed_follows_the_oracle(voters_cpu, capacity):
    kw = dict(capacity=capacity, use_graph=False, device="cpu", ensemble=VOTERS)
    eng = GpuServeEngine(voters_cpu, smooth=ALPHA, switch_margin=MARGIN, **kw)
    plain = GpuServeEngine(voters_cpu, **kw)
    ens = SoftVoteEnsemble(voters_cpu)
    C = len(ens.classes_)
    state = torch.zeros(8, C)
    held = torch.full((8,), -1, dtype=torch.int32)
    sizes, averaged = [], False
    for table in _polls():
        n = len(table)
        sizes.append(n)
        out, ref = eng.classify(table), plain.classify(table)
        assert list(out) == VOTERS + ["ensemble", "smoothed"]
        assert list(ref) == VOTERS + ["ensemble"] and list(plain.confidence) == ["ensemble"]
        for name in ref:  # nothing that was there changes
            np.testing.assert_array_equal(out[name], ref[name])
        np.testing.assert_array_equal(eng.confidence["ensemble"], plain.confidence["ensemble"])
        proba = ens.predict_proba(table.feature_matrix(dtype=np.float32))
        before = held[:n].clone()
        label, conf = oc.proba_smooth(proba, state, held, ALPHA, MARGIN)
        assert out["smoothed"].dtype == np.int32 and out["smoothed"].shape == (n,)
        np.testing.assert_array_equal(out["smoothed"], label.numpy())
        assert list(eng.confidence) == ["ensemble", "smoothed"]
        assert eng.confidence["smoothed"].dtype == np.float32
        np.testing.assert_array_equal(eng.confidence["smoothed"], conf.numpy())
        # a flow's first poll is its row as it is, not an average with
        # whatever its slot saw while it was empty
        new = before < 0
        np.testing.assert_array_equal(conf.numpy()[new.numpy()], proba.max(dim=1).values.numpy()[new.numpy()])
        averaged = averaged or bool((conf != proba.gather(1, label.long().unsqueeze(1)).squeeze(1)).any())
    assert sizes == [4] * 5 + [6] * 5
    assert averaged  # the sequence did exercise the average
    assert eng.smoother.capacity >= 6

    # a fresh table holds other flows in the same slots: the history goes
    other = list(_polls(polls=2, late_at=9, seed=5))[-1]
    out = eng.classify(other)
    proba = ens.predict_proba(other.feature_matrix(dtype=np.float32))
    best = proba.max(dim=1)
    np.testing.assert_array_equal(eng.confidence["smoothed"], best.values.numpy())
    np.testing.assert_array_equal(out["smoothed"], out["ensemble"])
    # and the same table again is a second poll of those flows
    out = eng.classify(other)
    state, held = proba.clone(), best.indices.to(torch.int32)
    label, conf = oc.proba_smooth(proba, state, held, ALPHA, MARGIN)
    np.testing.assert_array_equal(out["smoothed"], label.numpy())
    np.testing.assert_array_equal(eng.confidence["smoothed"], conf.numpy())


def test_engine_refusals(voters_cpu):
    kw = dict(use_graph=False, device="cpu")
    with pytest.raises(ValueError, match="ensemble"):
        GpuServeEngine(voters_cpu, smooth=0.3, **kw)
    named = dict(voters_cpu)
    named["smoothed"] = voters_cpu["GaussianNB"]
    with pytest.raises(ValueError, match="smoothed"):
        GpuServeEngine(named, ensemble=VOTERS, smooth=0.3, **kw)
    GpuServeEngine(named, ensemble=VOTERS, **kw)  # without smooth= the name is free
    for bad in (dict(smooth=0.0), dict(smooth=1.5), dict(smooth=0.3, switch_margin=-1.0)):
        with pytest.raises(ValueError):
            GpuServeEngine(voters_cpu, ensemble=VOTERS, **bad, **kw)


# ----------------------------------------------------------------------
# serve engine, GPU: the captured graph against the plain launches
# ----------------------------------------------------------------------


@pytest.fixture(scope="module")
def voters_gpu():
    return {n: _load(n, device="cuda") for n in VOTERS}


def _graph_against_eager(models, capacity):
    kw = dict(capacity=capacity, ensemble=VOTERS, smooth=ALPHA, switch_margin=MARGIN)
    graph = GpuServeEngine(models, use_graph=True, **kw)
    eager = GpuServeEngine(models, use_graph=False, **kw)
    plain = GpuServeEngine(models, use_graph=True, capacity=capacity, ensemble=VOTERS)
    history = []
    for k, table in enumerate(_polls()):
        n = len(table)
        out, ref, raw = graph.classify(table), eager.classify(table), plain.classify(table)
        assert list(out) == VOTERS + ["ensemble", "smoothed"]
        for name in out:
            assert out[name].shape == (n,), (k, name)
            np.testing.assert_array_equal(out[name], ref[name], err_msg=f"poll {k} {name}")
        for name in raw:
            np.testing.assert_array_equal(out[name], raw[name], err_msg=f"poll {k} {name}")
        assert list(graph.confidence) == ["ensemble", "smoothed"]
        for name in graph.confidence:  # equal to the f32 bit
            np.testing.assert_array_equal(
                graph.confidence[name], eager.confidence[name], err_msg=f"poll {k} {name}")
        history.append((out, dict(graph.confidence)))
    return graph, history


@needs_gpu
@pytest.mark.gpu
def test_engine_gpu_graph_equals_eager(voters_gpu):
    graph, history = _graph_against_eager(voters_gpu, capacity=256)
    assert graph._graph is not None
    # the two late flows are first sightings at poll 5: their smoothed
    # verdict is the vote's own, not an average with their empty slot's
    out, conf = history[5]
    np.testing.assert_array_equal(out["smoothed"][4:], out["ensemble"][4:])
    np.testing.assert_array_equal(conf["smoothed"][4:], conf["ensemble"][4:])
    # and the smoothed confidence did move away from the vote's somewhere
    assert any((c["smoothed"] != c["ensemble"]).any() for _, c in history[1:])


@needs_gpu
@pytest.mark.gpu
def test_engine_gpu_crosses_its_capacity(voters_gpu):
    graph, history = _graph_against_eager(voters_gpu, capacity=4)
    assert graph._graph is None and graph.smoother.capacity >= 6
    out, conf = history[5]
    np.testing.assert_array_equal(conf["smoothed"][4:], conf["ensemble"][4:])
    # the first four flows kept their history across the reallocation
    assert (conf["smoothed"][:4] != conf["ensemble"][:4]).any()


# ----------------------------------------------------------------------
# RealtimeClassifier and the CLI
# ----------------------------------------------------------------------


def _render_today(table, labels):
    """The six-column table as it is rendered without the new options."""
    t = Table(["Flow ID", "Src MAC", "Dest MAC", "Traffic Type", "Forward Status", "Reverse Status"])
    for i, (meta, (fs, rs)) in enumerate(zip(table.metas(), table.statuses())):
        t.add_row([i, meta.ethsrc, meta.ethdst, labels[i], fs, rs])
    return str(t)


def _passes(model, polls=6, seed=0, **kw):
    """([(rendered text, feature matrix)] of every pass, the whole output,
    and what the model's own labels render to without any option)."""
    out = io.StringIO()
    rc = RealtimeClassifier(model, out=out, **kw)
    passes, today = [], ""
    for line in TelemetryReplaySource(seed=seed).stream(polls):
        before = out.tell()
        if rc.feed(line):
            X = rc.parser.table.feature_matrix(dtype=np.float32)
            passes.append((out.getvalue()[before:], X))
            today += _render_today(rc.parser.table, model.predict(X)) + "\n"
    assert len(passes) >= 4
    return passes, out.getvalue(), today


def _rows(text):
    return [[c.strip() for c in l.strip("|").split("|")] for l in text.splitlines()[3:-1]]


def test_without_smooth_the_tables_are_todays(rf_cpu, capsys):
    passes, text, today = _passes(rf_cpu)
    assert text == today and "Confidence" not in text
    rc = cli.main(["Randomforest", "--source", "replay", "--replay-polls", "6", "--device", "cpu"])
    assert rc == 0
    assert capsys.readouterr().out == text


def test_realtime_labels_follow_a_hand_driven_smoother(rf_cpu):
    passes, _, _ = _passes(rf_cpu, polls=12, seed=1, smooth=0.3, switch_margin=0.1, confidence=True)
    raw, _, _ = _passes(rf_cpu, polls=12, seed=1, confidence=True)
    sm = FlowSmoother(len(rf_cpu.classes_), 16, 0.3, 0.1)
    moved = False
    for (text, X), (raw_text, _) in zip(passes, raw):
        idx, conf = sm.update(rf_cpu.predict_proba(X))
        rows = _rows(text)
        assert len(rows) == len(X) > 0
        for i, row in enumerate(rows):
            assert row[3] == rf_cpu.classes_[int(idx[i])]
            assert row[-1] == "%.2f" % float(conf[i])
        moved = moved or text != raw_text
    assert moved  # smoothing did change what is shown


def test_realtime_min_confidence_applies_to_the_smoothed_value(rf_cpu):
    thr = 0.75  # exact in f32, like the comparison
    passes, _, _ = _passes(rf_cpu, polls=12, seed=1, smooth=0.3, min_confidence=thr)
    sm = FlowSmoother(len(rf_cpu.classes_), 16, 0.3)
    below = 0
    for text, X in passes:
        idx, conf = sm.update(rf_cpu.predict_proba(X))
        for i, row in enumerate(_rows(text)):
            want = "unknown" if float(conf[i]) < np.float32(thr) else rf_cpu.classes_[int(idx[i])]
            assert row[3] == want
            below += want == "unknown"
    assert below > 0


def test_kmeans_is_refused(capsys):
    with pytest.raises(ValueError, match="KMeans"):
        RealtimeClassifier(_load("KMeans_Clustering"), out=io.StringIO(), smooth=0.3)
    rc = cli.main(["kmeans", "--source", "replay", "--replay-polls", "4", "--smooth", "0.3",
                   "--device", "cpu"])
    assert rc == 2
    cap = capsys.readouterr()
    assert cap.out == "" and len(cap.err.strip().splitlines()) == 1
    assert "--smooth" in cap.err


def test_cli_smooth(capsys):
    args = ["--source", "replay", "--replay-polls", "6", "--device", "cpu"]
    assert cli.main(["ensemble", "--members", "Randomforest,gaussiannb", "--smooth", "0.3",
                     "--switch-margin", "0.1", "--confidence"] + args) == 0
    assert "Confidence" in capsys.readouterr().out
    assert cli.main(["gaussiannb", "--smooth", "0.3"] + args) == 0
    assert "Confidence" not in capsys.readouterr().out
    for bad in (["--smooth", "1.5"], ["--smooth", "0"], ["--smooth", "0.3", "--switch-margin", "-1"]):
        assert cli.main(["Randomforest"] + bad + args) == 2
        cap = capsys.readouterr()
        assert cap.out == "" and len(cap.err.strip().splitlines()) == 1


# ----------------------------------------------------------------------
# what it buys
# ----------------------------------------------------------------------


@pytest.fixture(scope="module")
def replayed_probas(voters_cpu):
    """seed -> per poll, (the forest's, the four-member vote's) probabilities
    of the four default flows over 80 polls, classifying after every poll.
    The forest is walked once per poll for both."""
    ens = SoftVoteEnsemble({**voters_cpu, "KNeighbors": _load("KNeighbors")})
    assert list(ens.members)[0] == "RandomForestClassifier"
    cache = {}

    def get(seed):
        if seed not in cache:
            src = TelemetryReplaySource(seed=seed)
            parser = PollStreamParser()
            rows = []
            for _ in range(80):
                for line in src.poll():
                    parser.feed(line)
                members = ens.member_probas(parser.table.feature_matrix(dtype=np.float32))
                rows.append((members[0], ens.vote(members, want_proba=True)[0]))
            cache[seed] = rows
        return cache[seed]

    return get


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("which", [0, 1], ids=["forest", "vote"])
def test_flicker(replayed_probas, which, seed):
    """Label changes from one poll to the next, summed over the four flows:
    smoothing with alpha 0.3 and margin 0.1 leaves a quarter at the most."""
    probas = [row[which] for row in replayed_probas(seed)]
    sm = FlowSmoother(probas[0].shape[1], 4, 0.3, 0.1)
    raw = np.asarray([p.argmax(dim=1).numpy() for p in probas])
    smooth = np.asarray([sm.update(p)[0].numpy() for p in probas])
    raw, smooth = (int((seq[1:] != seq[:-1]).sum()) for seq in (raw, smooth))
    print(f"{('forest', 'vote')[which]} seed {seed}: raw {raw} smoothed {smooth}")
    assert raw > 0
    assert 4 * smooth <= raw
