"""Isolation forest novelty detection: the numbers behind profiles/novelty.md
and the README section.

    python tools/novelty_bench.py detect              # CPU: what the detector flags
    python tools/novelty_bench.py kernel              # MI355X: kernel, cutover, serve poll
    python tools/novelty_bench.py kernel --quick      # the same at small sizes (a rehearsal)

`detect` fits the detector (and sklearn's, when sklearn is there) on one half
of the six-class dataset, reports the share of the held-out half it flags per
class, and pushes three flows that no class describes through the replay ->
flow-table -> feature path: what the shipped forest calls them, with what
confidence, and how many of their rows each detector flags.  Seeds 0, 1, 2.

`kernel` times ops.iforest_score between device events, several rounds, all
listed: at 8192 rows (wave-per-row) and 10M rows (row-per-lane) next to
ops.rf_predict_scores of the shipped forest at the same shapes, alternating
the two round by round; both modes across 32K..512K rows for the cutover; and
the serve poll and its captured replay at 8192 flows x 5 models with and
without novelty=, alternating engines round by round.  One JSON line per
section.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from traffic_classifier_sdn_amd.flow.replay import SynthFlowSpec
from traffic_classifier_sdn_amd.models import IsolationForest, load_model
from traffic_classifier_sdn_amd.utils.datasets import (
    load_six_class_dataset, replay_feature_rows, synthetic_flow_rows,
)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
SERVE_MODELS = ["RandomForestClassifier", "GaussianNB", "LogisticRegression", "SVC",
                "KMeans_Clustering"]

# fwd pps x bytes per packet / rev pps x bytes per packet
UNKNOWN_FLOWS = {
    "bulk transfer 8000x1400 / 4000x64": (8000.0, 1400.0, 4000.0, 64.0),
    "video 30x64 / 450x1300": (30.0, 64.0, 450.0, 1300.0),
    "one-way scan 2000x60 / 0": (2000.0, 60.0, 0.0, 0.0),
}


def _split():
    X, y = load_six_class_dataset()
    perm = np.random.RandomState(0).permutation(len(X))
    return X, y, perm[::2], perm[1::2]


def _flow_rows(rates, seed):
    spec = SynthFlowSpec("00:00:00:00:01:01", "00:00:00:00:01:02", *rates)
    return replay_feature_rows([spec], 400, seed=seed)


def detect():
    X, y, tr, te = _split()
    rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device="cpu")
    t0 = time.perf_counter()
    own = IsolationForest(device="cpu").fit(X[tr])
    out = {
        "section": "detect", "fit_rows": len(tr), "heldout_rows": len(te),
        "own": {"fit_seconds": round(time.perf_counter() - t0, 3),
                "threshold": own.threshold_,
                "nodes": int(sum(len(t["left"]) for t in own.trees_)),
                "max_depth": int(max(_max_depth(t) for t in own.trees_))},
    }
    detectors = {"own": (own.score_samples, own.threshold_)}
    try:
        from sklearn.ensemble import IsolationForest as SkIF

        sk = SkIF(n_estimators=100, max_samples=256, random_state=0).fit(X[tr])
        sk_thr = float(np.quantile(-sk.score_samples(X[tr]), 0.99))
        detectors["sklearn"] = (lambda Q: -sk.score_samples(np.asarray(Q, dtype=np.float32)), sk_thr)
        out["sklearn"] = {"threshold": sk_thr}
    except ImportError:
        pass
    for name, (score, thr) in detectors.items():
        s = score(X[te])
        flagged = s > thr
        out[name]["heldout_flagged"] = round(float(flagged.mean()), 5)
        out[name]["heldout_flagged_per_class"] = {
            str(c): round(float(flagged[y[te] == c].mean()), 5) for c in np.unique(y)
        }
    flows = {}
    for label, rates in UNKNOWN_FLOWS.items():
        per_seed = []
        for seed in (0, 1, 2):
            rows = _flow_rows(rates, seed)
            names, conf = rf.predict_with_confidence(rows)
            top = max(set(names), key=list(names).count)
            rec = {"seed": seed, "forest_says": str(top),
                   "forest_confidence_median": round(float(np.median(conf)), 3)}
            for name, (score, thr) in detectors.items():
                s = score(rows)
                rec[name] = {"flagged": round(float((s > thr).mean()), 4),
                             "score_median": round(float(np.median(s)), 3)}
            per_seed.append(rec)
        flows[label] = per_seed
    out["flows"] = flows
    print(json.dumps(out))


def _max_depth(tree):
    depth = np.zeros(len(tree["left"]), dtype=np.int64)
    for i in np.nonzero(tree["left"] >= 0)[0]:
        depth[tree["left"][i]] = depth[tree["right"][i]] = depth[i] + 1
    return depth.max()


# ----------------------------------------------------------------------
# MI355X
# ----------------------------------------------------------------------


def _us_per_call(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps * 1e3


def _alternate(fns, rounds, budget_s):
    """{name: [us per call of each round]}: per round every function in turn,
    `reps` calls back to back between two device events, reps sized from one
    timed call so that all rounds fit the budget."""
    reps = {}
    for name, fn in fns.items():
        _us_per_call(fn, 1)  # code objects, allocator, packed tables
        one = _us_per_call(fn, 2) * 1e-6
        reps[name] = max(1, min(500, int(budget_s / rounds / len(fns) / one)))
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            out[name].append(round(_us_per_call(fn, reps[name]), 2))
    return {"reps": reps, "us": out}


def _set_mode(mode):
    if mode is None:
        os.environ.pop("TCSDN_IFOREST_MODE", None)
    else:
        os.environ["TCSDN_IFOREST_MODE"] = mode


def kernel(quick):
    from traffic_classifier_sdn_amd import ops
    from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine

    assert torch.cuda.is_available(), "the kernel section needs the GPU"
    Xd, _, tr, _ = _split()
    det = IsolationForest(device="cuda").fit(Xd[tr])
    rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device="cuda")
    forest = det.forest
    thr = det.threshold_
    sizes = (2048, 100_000) if quick else (8192, 10_000_000)
    rounds = 3 if quick else 5

    # 1. the kernels next to rf_scores, at the serve and the bulk size
    for n in sizes:
        X = torch.from_numpy(synthetic_flow_rows(n, seed=0)).cuda().contiguous()
        labels = torch.zeros(n, dtype=torch.int32, device="cuda")
        _set_mode(None)
        res = _alternate(
            {
                "iforest_score": lambda: ops.iforest_score(X, forest, thr, labels),
                "iforest_score, score only": lambda: ops.iforest_score(X, forest),
                "rf_predict_scores": lambda: ops.rf_predict_scores(X, rf.forest, want_proba=False),
            },
            rounds, budget_s=2.0 if quick else 12.0,
        )
        print(json.dumps({"section": "kernel", "rows": n, "trees": len(det.trees_),
                          "nodes": int(forest["feature"].numel()), **res}))

    # 2. the cutover: both modes, same inputs
    sweep = (32768, 65536) if quick else (32768, 65536, 131072, 163840, 196608, 262144, 393216, 524288)
    for n in sweep:
        X = torch.from_numpy(synthetic_flow_rows(n, seed=1)).cuda().contiguous()

        def run(mode):
            def fn():
                _set_mode(mode)
                ops.iforest_score(X, forest, thr)
            return fn

        res = _alternate({"wave": run("wave"), "lane": run("lane")}, rounds,
                         budget_s=1.0 if quick else 4.0)
        print(json.dumps({"section": "cutover", "rows": n, **res}))
    _set_mode(None)

    # 3. the serve poll at 8192 flows x 5 models, with and without novelty=
    n = 512 if quick else 8192
    models = {m: load_model(os.path.join(MODELS, m + ".npz"), device="cuda") for m in SERVE_MODELS}
    table = _table(n)
    engines = {
        "plain": GpuServeEngine(models, capacity=n),
        "novelty": GpuServeEngine(models, capacity=n, novelty=det),
        "traffic": GpuServeEngine(models, capacity=n, traffic="RandomForestClassifier"),
        "traffic + novelty": GpuServeEngine(models, capacity=n, traffic="RandomForestClassifier",
                                            novelty=det),
    }
    polls = 20 if quick else 100
    poll_ms = {k: [] for k in engines}
    replay_us = {k: [] for k in engines}
    for eng in engines.values():
        for _ in range(3):
            eng.classify(table)
    for _ in range(rounds):
        for name, eng in engines.items():
            t0 = time.perf_counter()
            for _ in range(polls):
                eng.classify(table)
            poll_ms[name].append(round((time.perf_counter() - t0) / polls * 1e3, 4))
            replay_us[name].append(round(_us_per_call(eng._graph.replay, polls), 2))
    print(json.dumps({"section": "serve", "flows": n, "models": SERVE_MODELS, "polls": polls,
                      "poll_ms": poll_ms, "graph_replay_us": replay_us,
                      "novel_flows": int(engines["novelty"].novel.sum())}))


def _table(n):
    """The flow table of bench.py's serve workload: n random flows, two polls."""
    from traffic_classifier_sdn_amd.flow.parser import replay
    from traffic_classifier_sdn_amd.flow.replay import TelemetryReplaySource

    rng = np.random.default_rng(0)
    specs = [
        SynthFlowSpec(
            "02:%02x:%02x:%02x:%02x:%02x" % tuple(int(v) for v in rng.integers(0, 256, 5)),
            "06:%02x:%02x:%02x:%02x:%02x" % tuple(int(v) for v in rng.integers(0, 256, 5)),
            float(rng.uniform(1, 60)), float(rng.uniform(60, 1200)),
            float(rng.uniform(1, 60)), float(rng.uniform(60, 1200)),
        )
        for _ in range(n)
    ]
    src = TelemetryReplaySource(specs=specs, seed=0)
    try:
        from traffic_classifier_sdn_amd.flow.native import NativePollParser

        parser = NativePollParser()
        parser.feed_buffer("\n".join(src.stream(2)) + "\n")
        return parser.table
    except (ImportError, RuntimeError):
        return replay(src.stream(2))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("section", choices=("detect", "kernel"))
    ap.add_argument("--quick", action="store_true", help="kernel: small sizes, short rounds")
    args = ap.parse_args()
    detect() if args.section == "detect" else kernel(args.quick)
