"""Isolation forest novelty detector on the CPU: models/isolation_forest.py,
its flatten/pack/score ops in ops/cpu.py, and the serve paths that use it.

The split of every test here: the six-class dataset, rows permuted by
RandomState(0), even positions to fit and odd positions held out.
"""

import io
import json
import math
import os

import numpy as np
import pytest
import torch

from traffic_classifier_sdn_amd import cli, ops
from traffic_classifier_sdn_amd.flow.parser import PollStreamParser
from traffic_classifier_sdn_amd.flow.replay import (
    SynthFlowSpec, TelemetryReplaySource, default_specs,
)
from traffic_classifier_sdn_amd.models import (
    IsolationForest, SoftVoteEnsemble, load_model,
)
from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.serve import RealtimeClassifier
from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine
from traffic_classifier_sdn_amd.utils.datasets import (
    load_six_class_dataset, replay_feature_rows,
)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")

# flows that none of the six classes describes (pps x bytes per packet)
BULK = SynthFlowSpec("00:00:00:00:01:01", "00:00:00:00:01:02", 8000.0, 1400.0, 4000.0, 64.0)
SCAN = SynthFlowSpec("00:00:00:00:01:03", "00:00:00:00:01:04", 2000.0, 60.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def halves():
    """(X, y, fit rows, held-out rows)."""
    try:
        X, y = load_six_class_dataset()
    except FileNotFoundError:
        pytest.skip("no dataset available")
    perm = np.random.RandomState(0).permutation(len(X))
    return X, y, perm[::2], perm[1::2]


@pytest.fixture(scope="module")
def own(halves):
    X, _, tr, _ = halves
    return IsolationForest(device="cpu").fit(X[tr])


@pytest.fixture(scope="module")
def sk_fit(halves):
    ens = pytest.importorskip("sklearn.ensemble")
    X, _, tr, _ = halves
    return ens.IsolationForest(n_estimators=100, max_samples=256, random_state=0).fit(X[tr])


# ----------------------------------------------------------------------
# parity with sklearn
# ----------------------------------------------------------------------


def test_sklearn_score_and_leaf_parity(halves, sk_fit):
    """The f32 leaf values carry 2^-24 relative error into the mean path
    length, the exponent 2^(-s) with s <= ~1.5 turns that into about 1e-7
    relative on a score below 1, and the f32 output adds 2^-25: about 1.2e-7
    in all.  The bound is twice that."""
    X, _, _, te = halves
    Q = np.concatenate([X[te], X[te] * 3.7]).astype(np.float32)
    m = IsolationForest.from_sklearn(sk_fit, device="cpu")
    got = m.score_samples(Q)
    ref = -sk_fit.score_samples(Q)
    assert got.dtype == np.float32 and got.shape == (len(Q),)
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"max |score - sklearn| = {err:.3e}")
    assert err <= 2.5e-7
    assert (got > 0).all() and (got <= 1).all()
    leaves = oc.iforest_leaves(torch.from_numpy(Q), m.forest).numpy()
    offsets = m.forest["tree_offset"].numpy()
    for t, est in enumerate(sk_fit.estimators_):
        np.testing.assert_array_equal(leaves[:, t] - offsets[t], est.apply(Q))
    assert m.max_samples_ == sk_fit.max_samples_ == 256
    assert m.threshold_ == -sk_fit.offset_


def test_from_sklearn_rejects_feature_subsampling(halves):
    ens = pytest.importorskip("sklearn.ensemble")
    X, _, tr, _ = halves
    sk = ens.IsolationForest(n_estimators=3, max_samples=32, max_features=0.5,
                             random_state=0).fit(X[tr][:200])
    with pytest.raises(ValueError, match="max_features"):
        IsolationForest.from_sklearn(sk)


# ----------------------------------------------------------------------
# threshold rounding
# ----------------------------------------------------------------------


def _stump(thr, n_left=1, n_right=2):
    return {
        "left": np.array([1, -1, -1]), "right": np.array([2, -1, -1]),
        "feature": np.array([0, -1, -1]), "threshold": np.array([thr, 0.0, 0.0]),
        "n_node_samples": np.array([n_left + n_right, n_left, n_right]),
    }


@pytest.mark.parametrize("frac", [0.25, 0.5, 0.75])
def test_threshold_between_two_f32_routes_like_f64(frac):
    """An f64 threshold strictly between the adjacent f32 values a < b: a
    goes left and b goes right.  A cast to the nearest f32 gives b for
    frac > 0.5 (and for the tie, whose even neighbour b is) and sends b left."""
    a = np.float32(1.0)
    b = np.nextafter(a, np.float32(np.inf))
    thr = float(a) + frac * (float(b) - float(a))
    assert float(a) < thr < float(b)
    forest = oc.iforest_flatten([_stump(thr)], 3)
    assert float(forest["threshold"][0]) == float(a)
    X = torch.zeros(2, 12)
    X[0, 0], X[1, 0] = float(a), float(b)
    leaves = oc.iforest_leaves(X, forest)[:, 0].tolist()
    assert leaves == [1 if float(x) <= thr else 2 for x in (a, b)] == [1, 2]
    _, _, _, psum = oc.iforest_score(X, forest, want_sum=True)
    assert psum.tolist() == [1.0 + 0.0, 1.0 + 1.0]  # depth 1 + c(1), depth 1 + c(2)


def test_threshold_rounding_keeps_exact_and_extreme_values():
    v = np.array([1.0, -2.5, 1e300, -1e300, float(np.float32(0.1))])
    t = oc._f32_round_down(v)
    assert t.dtype == np.float32
    assert t[0] == 1.0 and t[1] == -2.5 and t[4] == np.float32(0.1)
    assert t[2] == np.finfo(np.float32).max and t[3] == -np.inf
    assert (t.astype(np.float64) <= v).all()


def test_average_path_length():
    c = oc.iforest_c([0, 1, 2, 3, 256])
    assert c[0] == 0 and c[1] == 0 and c[2] == 1
    assert c[3] == 2 * (math.log(2) + 0.5772156649015329) - 4 / 3
    assert c[4] == 2 * (math.log(255) + 0.5772156649015329) - 2 * 255 / 256
    assert abs(c[4] - 10.2447709) < 1e-6  # the c(256) of the isolation forest paper's psi


# ----------------------------------------------------------------------
# own fit
# ----------------------------------------------------------------------


def _depths(tree):
    depth = np.zeros(len(tree["left"]), dtype=np.int64)
    for i in np.nonzero(tree["left"] >= 0)[0]:
        depth[tree["left"][i]] = depth[tree["right"][i]] = depth[i] + 1
    return depth


def test_fit_invariants(halves, own):
    X, _, tr, _ = halves
    Xtr = X[tr].astype(np.float32).astype(np.float64)
    assert own.max_samples_ == 256 and len(own.trees_) == 100
    assert own.classes_ is None and own.kind == "isolation_forest"
    for t, tree in enumerate(own.trees_):
        left, right, nns = tree["left"], tree["right"], tree["n_node_samples"]
        inner = np.nonzero(left >= 0)[0]
        np.testing.assert_array_equal(left[inner], inner + 1)  # depth-first order
        assert _depths(tree).max() <= math.ceil(math.log2(256)) == 8
        assert nns[0] == 256
        np.testing.assert_array_equal(nns[left[inner]] + nns[right[inner]], nns[inner])
        # every threshold strictly inside its node's feature range: replay
        # the rows the tree drew down the tree
        rng = np.random.default_rng([own.random_state, t])
        rows = {0: Xtr[rng.choice(len(Xtr), size=256, replace=False)]}
        for i in inner:
            x = rows.pop(i)
            f, thr = tree["feature"][i], tree["threshold"][i]
            assert x[:, f].min() < thr < x[:, f].max()
            rows[left[i]], rows[right[i]] = x[x[:, f] <= thr], x[x[:, f] > thr]
        for i, x in rows.items():  # leaves: one row, identical rows, or the depth cap
            assert len(x) == nns[i]
            assert len(x) == 1 or (x == x[0]).all() or _depths(tree)[i] == 8


def test_fit_is_reproducible_and_trees_do_not_depend_on_their_number(halves, own):
    X, _, tr, _ = halves
    again = IsolationForest(device="cpu").fit(X[tr])
    few = IsolationForest(n_estimators=10, device="cpu").fit(X[tr])
    other = IsolationForest(random_state=1, n_estimators=10, device="cpu").fit(X[tr])
    assert again.threshold_ == own.threshold_
    for t in range(100):
        for k in own.trees_[t]:
            np.testing.assert_array_equal(again.trees_[t][k], own.trees_[t][k])
    for t in range(10):
        for k in own.trees_[t]:
            np.testing.assert_array_equal(few.trees_[t][k], own.trees_[t][k])
    assert any(
        len(other.trees_[t]["left"]) != len(own.trees_[t]["left"])
        or not np.array_equal(other.trees_[t]["threshold"], own.trees_[t]["threshold"])
        for t in range(10)
    )


def test_threshold_is_the_training_quantile(halves, own):
    X, _, tr, _ = halves
    flagged = own.predict_novel(X[tr]).mean()
    assert 0.0 < own.threshold_ < 1.0
    assert abs(flagged - own.contamination) <= 1.0 / len(tr) + 1e-12
    s = own.score_samples(X[tr][:500])
    nov = own.predict_novel(X[tr][:500])
    clear = np.abs(s - own.threshold_) > 1e-6  # away from the f32 rounding of s
    np.testing.assert_array_equal(nov[clear], (s > own.threshold_)[clear])
    assert own.predict_novel(X[tr][:500], threshold=0.999).sum() == 0


# ----------------------------------------------------------------------
# detection
# ----------------------------------------------------------------------


def test_heldout_flagged_share_is_within_a_point_of_sklearns(halves, own, sk_fit):
    """The own fit may flag at most 0.01 more of the held-out rows than
    sklearn's on the same split (one binomial sd at p = 0.01 over 4448 rows
    is 0.0015)."""
    X, y, tr, te = halves
    sk_thr = np.quantile(-sk_fit.score_samples(X[tr]), 0.99)
    sk_share = float((-sk_fit.score_samples(X[te]) > sk_thr).mean())
    share = float(own.predict_novel(X[te]).mean())
    print(f"held-out flagged: own {share:.4f}, sklearn {sk_share:.4f}")
    assert share <= sk_share + 0.01


@pytest.mark.parametrize("spec", [BULK, SCAN], ids=["bulk", "scan"])
def test_unknown_flows_are_flagged(own, spec):
    rows = replay_feature_rows([spec], 400, seed=0)
    assert rows.shape == (400, 12)
    share = float(own.predict_novel(rows).mean())
    print(f"flagged {share:.3f}, median score {np.median(own.score_samples(rows)):.3f}")
    assert share >= 0.95


# ----------------------------------------------------------------------
# checkpoint and refusals
# ----------------------------------------------------------------------


def test_checkpoint_round_trip(tmp_path, halves, own):
    X, _, _, te = halves
    path = str(tmp_path / "IsolationForest.npz")
    own.save(path)
    back = load_model(path, device="cpu")
    assert isinstance(back, IsolationForest)
    assert back.threshold_ == own.threshold_ and back.max_samples_ == own.max_samples_
    assert back.contamination == own.contamination and back.random_state == own.random_state
    Q = X[te][:300]
    np.testing.assert_array_equal(back.score_samples(Q), own.score_samples(Q))
    np.testing.assert_array_equal(back.predict_novel(Q), own.predict_novel(Q))


def test_refused_as_a_classifier(tmp_path, own, halves):
    X = halves[0]
    rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device="cpu")
    with pytest.raises(ValueError, match="not a classifier"):
        own.predict_index(X[:3])
    with pytest.raises(ValueError, match="not a classifier"):
        own.predict(X[:3])
    with pytest.raises(ValueError, match="IsolationForest"):
        SoftVoteEnsemble({"rf": rf, "iso": own})
    with pytest.raises(ValueError, match="IsolationForest"):
        GpuServeEngine({"rf": rf, "iso": own}, device="cpu", use_graph=False)
    with pytest.raises(ValueError, match="IsolationForest"):
        RealtimeClassifier(own)
    with pytest.raises(ValueError, match="novelty= takes an IsolationForest"):
        GpuServeEngine({"rf": rf}, device="cpu", use_graph=False, novelty=rf)
    with pytest.raises(ValueError, match="novelty= takes an IsolationForest"):
        RealtimeClassifier(rf, novelty=rf)
    with pytest.raises(ValueError, match="fitted"):
        GpuServeEngine({"rf": rf}, device="cpu", use_graph=False, novelty=IsolationForest(device="cpu"))
    with pytest.raises(ValueError, match="fitted"):
        RealtimeClassifier(rf, novelty=IsolationForest(device="cpu"))
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            GpuServeEngine({"rf": rf}, device="cpu", use_graph=False, novelty=own,
                           novelty_threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            RealtimeClassifier(rf, novelty=own, novelty_threshold=bad)
    # the CLI: a detector's checkpoint under a classifier's name
    own.save(str(tmp_path / "RandomForestClassifier.npz"))
    assert cli.main(["Randomforest", "--source", "replay", "--replay-polls", "2",
                     "--device", "cpu", "--models-dir", str(tmp_path)]) == 2
    assert cli.main(["ensemble", "--members", "Randomforest,gaussiannb", "--source", "replay",
                     "--replay-polls", "2", "--device", "cpu", "--models-dir", str(tmp_path)]) == 2


def _chain(depth):
    """One tree that is a chain of ``depth`` inner nodes going left."""
    n = 2 * depth + 1
    left = np.full(n, -1)
    right = np.full(n, -1)
    feature = np.full(n, -1)
    for i in range(depth):
        left[i], right[i], feature[i] = i + 1, n - 1 - i, 0
    return {
        "left": left, "right": right, "feature": feature,
        "threshold": np.where(feature >= 0, 1.0, 0.0),
        "n_node_samples": np.ones(n, dtype=np.int64),
    }


def test_pack_time_rules():
    good = oc.iforest_flatten([_stump(0.5), _chain(8)], 256)
    packed = ops.iforest_pack(good, "cpu")
    assert packed["nodes"].shape == (3 + 17, 2) and packed["roots"].tolist() == [0, 3]
    assert packed["n_trees"] == 2
    # a tree not in depth-first order: at flatten time and at pack time
    swapped = _stump(0.5)
    swapped["left"], swapped["right"] = swapped["right"].copy(), swapped["left"].copy()
    with pytest.raises(ValueError, match="depth-first"):
        oc.iforest_flatten([swapped], 256)
    bad = dict(good, right=good["right"].clone())
    bad["right"][0] = 1  # the left child's place
    with pytest.raises(ValueError, match="depth-first"):
        ops.iforest_pack(bad, "cpu")
    bad["right"][0] = 3  # the next tree's root
    with pytest.raises(ValueError, match="depth-first"):
        ops.iforest_pack(bad, "cpu")
    # a feature outside 0..11
    t = _stump(0.5)
    t["feature"][0] = 12
    with pytest.raises(ValueError, match="0..11"):
        ops.iforest_pack(oc.iforest_flatten([t], 256), "cpu")
    # more than 4096 trees
    root_only = {k: np.array([v]) for k, v in
                 (("left", -1), ("right", -1), ("feature", -1), ("threshold", 0.0),
                  ("n_node_samples", 2))}
    ops.iforest_pack(oc.iforest_flatten([root_only] * 4096, 256), "cpu")
    with pytest.raises(ValueError, match="4096 trees"):
        ops.iforest_pack(oc.iforest_flatten([root_only] * 4097, 256), "cpu")
    # h >= 64: a leaf at depth 64, and a shallower one with many rows
    with pytest.raises(ValueError, match="64"):
        ops.iforest_pack(oc.iforest_flatten([_chain(64)], 256), "cpu")
    ops.iforest_pack(oc.iforest_flatten([_chain(63)], 256), "cpu")
    crowded = _chain(60)
    crowded["n_node_samples"][60] = 10**6  # c(10^6) = 26.8
    with pytest.raises(ValueError, match="64"):
        ops.iforest_pack(oc.iforest_flatten([crowded], 256), "cpu")
    # more than 2^24 - 1 nodes (tensors of that length without their memory)
    n = 1 << 24
    huge = {
        "threshold": torch.zeros(1).expand(n), "right": torch.zeros(1, dtype=torch.int32).expand(n),
        "feature": torch.full((1,), -1, dtype=torch.int32).expand(n),
        "leaf_h": torch.ones(1).expand(n),
        "tree_offset": torch.tensor([0, n], dtype=torch.int32),
        "max_samples": torch.tensor(256, dtype=torch.int32),
    }
    with pytest.raises(ValueError, match="2\\^24 - 1 nodes"):
        ops.iforest_pack(huge, "cpu")


def test_score_argument_rules(own):
    X = torch.zeros(4, 12)
    lab = torch.zeros(4, dtype=torch.int32)
    f = own.forest
    oc.iforest_score(X, f, 0.5, lab)
    for bad in (X.double(), torch.zeros(4, 11), torch.zeros(12, 4).t(), X.numpy()):
        with pytest.raises(ValueError):
            oc.iforest_score(bad, f)
    for bad in (lab[:3], lab.long(), torch.zeros(8, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="labels"):
            oc.iforest_score(X, f, 0.5, bad)
    for bad in (0, 1, 0.0, 1.0, -1.0, 2.0, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="threshold"):
            oc.iforest_score(X, f, bad)
    score, flags, masked, psum = oc.iforest_score(X, f)  # None flags nothing
    assert flags.dtype == torch.uint8 and not bool(flags.any())
    assert masked is None and psum is None and score.dtype == torch.float32


# ----------------------------------------------------------------------
# serve on the CPU
# ----------------------------------------------------------------------


def _tables(polls=6, seed=0):
    """The flow table after each poll: the four default flows and one bulk
    transfer, which is flow 4."""
    src = TelemetryReplaySource(specs=default_specs() + [BULK], seed=seed)
    parser = PollStreamParser()
    for _ in range(polls):
        for line in src.poll():
            parser.feed(line)
        yield parser.table


# The replay's "voice-like" flow is only loosely voice: it scores 0.64-0.68,
# right under the fitted threshold (0.683), and crosses it on some polls (the
# README says so).  The engine test is about where flagged flows go, so it
# sets the threshold halfway between sklearn's fitted threshold (0.68) and
# its median score of the bulk flow (0.79) on this split; the engine without
# traffic= and the classify loop below keep the detector's own threshold.
SERVE_THRESHOLD = 0.735


def test_engine_cpu_counts_the_bulk_flow_as_unknown(own):
    rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device="cpu")
    kw = dict(capacity=64, use_graph=False, device="cpu")
    nov = dict(novelty=own, novelty_threshold=SERVE_THRESHOLD)
    eng = GpuServeEngine({"rf": rf}, traffic="rf", **nov, **kw)
    small = GpuServeEngine({"rf": rf}, traffic="rf", **nov, **dict(kw, capacity=4))
    only = GpuServeEngine({"rf": rf}, novelty=own, **kw)
    plain = GpuServeEngine({"rf": rf}, traffic="rf", **kw)
    assert plain.novel is None and plain.novelty_score is None
    C = len(rf.classes_)
    for k, table in enumerate(_tables()):
        out, ref = eng.classify(table), plain.classify(table)
        assert list(out) == list(ref) == ["rf"]
        np.testing.assert_array_equal(out["rf"], ref["rf"])  # labels as without novelty=
        np.testing.assert_array_equal(small.classify(table)["rf"], ref["rf"])
        np.testing.assert_array_equal(only.classify(table)["rf"], ref["rf"])
        X = torch.from_numpy(np.ascontiguousarray(table.feature_matrix(dtype=np.float32)))
        lab = torch.from_numpy(out["rf"].astype(np.int32))
        score, flags, masked, _ = oc.iforest_score(X, own.forest, SERVE_THRESHOLD, lab)
        own_flags = oc.iforest_score(X, own.forest, own.threshold_)[1]
        for e, fl in ((eng, flags), (small, flags), (only, own_flags)):
            assert e.novel.dtype == bool and e.novelty_score.dtype == np.float32
            np.testing.assert_array_equal(e.novel, fl.numpy().astype(bool))
            np.testing.assert_array_equal(e.novelty_score, score.numpy())
        if k == 0:
            continue  # the first poll has no rates yet
        assert eng.novel.tolist() == [False] * 4 + [True]
        want = oc.class_traffic(X, masked, C).numpy()
        np.testing.assert_array_equal(eng.traffic, want)
        np.testing.assert_array_equal(small.traffic, want)
        assert only.traffic is None
        # the bulk flow's row, bytes included, is the unknown row
        assert eng.traffic[C, 0] == 1
        np.testing.assert_array_equal(eng.traffic[C, 1:], X[4].double().numpy())
        assert plain.traffic[C, 0] == 0
        np.testing.assert_array_equal(eng.traffic[:C].sum(0) + eng.traffic[C], plain.traffic.sum(0))


def test_classify_loop_shows_the_bulk_flow_as_unknown(own):
    rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device="cpu")
    out, stats = io.StringIO(), io.StringIO()
    rc = RealtimeClassifier(rf, out=out, stats=True, stats_out=stats, summary=True, novelty=own)
    plain = RealtimeClassifier(rf, out=io.StringIO(), summary=True)
    src = TelemetryReplaySource(specs=default_specs() + [BULK], seed=0)
    for line in src.stream(8):
        rc.feed(line)
        plain.feed(line)
    got, ref = rc.classify_now(), plain.classify_now()
    assert got[4] == "unknown" and ref[4] != "unknown"
    assert list(got[:4]) == list(ref[:4])
    assert rc.last_novel.tolist() == [False] * 4 + [True]
    C = len(rc.traffic_classes) - 1
    totals = rc.account(got)
    assert totals[C, 0] == 1
    np.testing.assert_array_equal(
        totals[C, 1:], rc.parser.table.feature_matrix(dtype=np.float32)[4].astype(np.float64))
    lines = [json.loads(l) for l in stats.getvalue().splitlines()]
    assert lines and all("novel" in l for l in lines)
    assert lines[-1]["novel"] == 1 and lines[-1]["traffic"]["unknown"]["flows"] == 1
    assert "unknown" in out.getvalue()


def test_cli_novelty_fits_at_start_up_without_a_checkpoint(tmp_path, capsys):
    rc = cli.main(["Randomforest", "--source", "replay", "--replay-polls", "3", "--device", "cpu",
                   "--novelty", "--novelty-threshold", "0.6", "--stats",
                   "--models-dir", str(tmp_path)])
    captured = capsys.readouterr()
    assert rc == 0
    shipped = os.path.exists(os.path.join(MODELS, "IsolationForest.npz"))
    assert shipped or "fitting the novelty detector" in captured.err
    assert '"novel":' in captured.err
    assert cli.main(["Randomforest", "--source", "replay", "--device", "cpu",
                     "--novelty-threshold", "0.6", "--models-dir", str(tmp_path)]) == 2
    assert cli.main(["Randomforest", "--source", "replay", "--device", "cpu", "--novelty",
                     "--novelty-threshold", "1.5", "--models-dir", str(tmp_path)]) == 2
