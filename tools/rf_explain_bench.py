"""Why a forest gave a flow its class: the numbers behind profiles/rf_explain.md
and the README section.

    python tools/rf_explain_bench.py mix       # CPU: the Why of the replay flows and of three unknown ones
    python tools/rf_explain_bench.py kernels   # MI355X: op timings, both kernels across row counts
    python tools/rf_explain_bench.py cost      # MI355X: the serve poll without and with explain=
    python tools/rf_explain_bench.py cost --engine-file OLD_SERVE_GPU.py

`mix` replays the default four flows for 80 polls with the shipped forest and
prints what `Randomforest --explain` shows after the last poll, seed 0; then,
for the three flows of `tools/novelty_bench.py detect` that belong to no
class, what the forest calls them and which features make it say so (the
mean contribution over 400 polls of the flow).  `kernels` times
ops.rf_explain on the shipped forest next to ops.rf_predict_scores on the
same rows, the two kernels (TCSDN_RF_EXPLAIN_MODE) across row counts, and
checks every result against the CPU oracle at the sizes where that is quick.
`cost` alternates serve engines over 8192 flows and five models without and
with explain= inside one process, round by round; --engine-file adds the
engine of another revision's serve_gpu.py (same package, same kernels).  One
JSON line per section.  The timing helpers are those of tools/traffic_bench.py.
"""

import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from traffic_bench import _engine_class, _load, _ms_per_call, _rounds

POLLS = 80
SERVE_MODELS = ["RandomForestClassifier", "GaussianNB", "LogisticRegression", "SVC",
                "KMeans_Clustering"]
CROSS_ROWS = (1024, 6144, 8192, 32768, 49152, 65536, 131072, 262144, 524288, 1 << 20, 1 << 22)
BIG = 10_000_000


def mix():
    from novelty_bench import UNKNOWN_FLOWS, _flow_rows
    from traffic_classifier_sdn_amd.flow.replay import TelemetryReplaySource
    from traffic_classifier_sdn_amd.serve import RealtimeClassifier
    from traffic_classifier_sdn_amd.utils.schema import FEATURE_SHORT_NAMES

    forest = _load("RandomForestClassifier", "cpu")
    out = io.StringIO()
    rc = RealtimeClassifier(forest, out=out, confidence=True, explain=True)
    src = TelemetryReplaySource(seed=0)
    last = ""
    for _ in range(POLLS):
        for line in src.poll():
            before = out.tell()
            if rc.feed(line):
                last = out.getvalue()[before:]
    print(f"seed 0, {len(rc.parser.table)} flows after {POLLS} polls")
    print(last, end="")
    res = {"section": "mix", "polls": POLLS, "model": "RandomForestClassifier",
           "why": [[FEATURE_SHORT_NAMES[f], round(float(v), 4)] if f >= 0 else None
                   for f, v in zip(rc.last_why, rc.last_why_value)]}
    bias = forest.explain_tables["bias"].numpy()
    flows = {}
    for label, rates in UNKNOWN_FLOWS.items():
        rows = _flow_rows(rates, 0)
        names, conf = forest.predict_with_confidence(rows)
        top = max(set(names), key=list(names).count)
        c = list(forest.classes_).index(top)
        lab = torch.full((len(rows),), c, dtype=torch.int32)
        contrib = forest.explain_device(rows, lab)[0].numpy().astype(np.float64).mean(axis=0)
        order = np.argsort(-contrib)[:3]
        flows[label] = {
            "forest_says": str(top),
            "forest_confidence_median": round(float(np.median(conf)), 3),
            "bias": round(float(bias[c]), 4),
            "mean_probability_of_that_class": round(float(bias[c] + contrib.sum()), 4),
            "top_features": [[FEATURE_SHORT_NAMES[f], round(float(contrib[f]), 4)] for f in order],
        }
        print(f"{label}: {top} at {np.median(conf):.2f}; "
              + ", ".join("%s %+.2f" % (FEATURE_SHORT_NAMES[f], contrib[f]) for f in order)
              + f" (bias {bias[c]:.2f})")
    res["unknown_flows"] = flows
    print(json.dumps(res))


def _set_mode(mode):
    if mode is None:
        os.environ.pop("TCSDN_RF_EXPLAIN_MODE", None)
    else:
        os.environ["TCSDN_RF_EXPLAIN_MODE"] = mode


def _equal(got, want):
    return all((a is None and b is None) or torch.equal(a.cpu(), b) for a, b in zip(got, want))


def kernels():
    """ops.gpu.rf_explain (one kernel and three allocations per call) on the
    shipped forest and synthetic flow rows, labels the forest's own."""
    from traffic_classifier_sdn_amd.ops import cpu as oc
    from traffic_classifier_sdn_amd.ops import gpu as og
    from traffic_classifier_sdn_amd.utils.datasets import synthetic_flow_rows

    rf = _load("RandomForestClassifier", "cuda")
    forest, tables = rf.forest, rf.explain_tables
    cpu_forest = _load("RandomForestClassifier", "cpu").forest
    X_all = torch.from_numpy(np.ascontiguousarray(synthetic_flow_rows(BIG, seed=0), dtype=np.float32)).cuda()
    for n in CROSS_ROWS + (BIG,):
        X = X_all[:n].contiguous()
        labels = og.rf_predict_scores(X, forest, want_proba=False)[1]
        res = {"section": "kernels", "rows": n, "trees": len(rf.trees_), "nodes": int(tables["delta"].shape[0])}
        budget = 2.0 if n < BIG else 6.0
        res["scores_reps"], res["scores_us"] = _rounds(
            lambda: og.rf_predict_scores(X, forest, want_proba=False), budget_s=budget)
        for mode in ("wave", "lane"):
            _set_mode(mode)
            res[f"{mode}_reps"], res[f"{mode}_us"] = _rounds(
                lambda: og.rf_explain(X, forest, tables, labels, want_matrix=False), budget_s=budget)
            if n <= 1 << 20:
                res[f"{mode}_matrix_us"] = _rounds(
                    lambda: og.rf_explain(X, forest, tables, labels), budget_s=budget)[1]
            if n <= 65536:
                got = og.rf_explain(X, forest, tables, labels, True, True)
                want = oc.rf_explain(X.cpu(), cpu_forest, tables, labels.cpu(), True, True)
                res[f"{mode}_equal_to_oracle"] = _equal(got, want)
        _set_mode(None)
        res["default_us"] = _rounds(
            lambda: og.rf_explain(X, forest, tables, labels, want_matrix=False), budget_s=budget)[1]
        print(json.dumps(res), flush=True)


def cost(engine_file=None):
    """GpuServeEngine.classify over 8192 live flows and five models, hipGraph
    path, without and with explain= (and with the matrix): whole-poll latency
    and the graph replay alone."""
    from traffic_classifier_sdn_amd.flow.parser import replay
    from traffic_classifier_sdn_amd.flow.replay import SynthFlowSpec, TelemetryReplaySource
    from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine

    n = 8192
    rng = np.random.default_rng(0)
    mac = lambda p: p + ":%02x:%02x:%02x:%02x:%02x" % tuple(int(v) for v in rng.integers(0, 256, 5))
    specs = [SynthFlowSpec(mac("02"), mac("06"), float(rng.uniform(1, 60)), float(rng.uniform(60, 1200)),
                           float(rng.uniform(1, 60)), float(rng.uniform(60, 1200)))
             for _ in range(n)]
    table = replay(TelemetryReplaySource(specs=specs, seed=0).stream(2))
    models = {name: _load(name, "cuda") for name in SERVE_MODELS}
    kw = dict(capacity=n, use_graph=True)
    engines = {}
    if engine_file:
        engines["other"] = _engine_class(engine_file)(models, **kw)
    engines["plain"] = GpuServeEngine(models, **kw)
    engines["explain"] = GpuServeEngine(models, explain="RandomForestClassifier", **kw)
    engines["matrix"] = GpuServeEngine(models, explain="RandomForestClassifier", explain_matrix=True, **kw)
    out = {"section": "cost", "flows": len(table), "models": SERVE_MODELS, "engines": list(engines)}
    labels = {}
    for key, eng in engines.items():
        for _ in range(5):
            labels[key] = eng.classify(table)  # capture + warm-up
    for key in engines:
        assert all(np.array_equal(labels[key][m], labels["plain"][m]) for m in labels[key]), key
    assert np.array_equal(engines["explain"].why, engines["matrix"].why)
    for _ in range(5):
        for key, eng in engines.items():
            polls = []
            for _ in range(100):
                eng.classify(table)
                polls.append(eng.last_latency_s * 1e3)
            out.setdefault(f"poll_p50_ms_{key}", []).append(round(float(np.percentile(polls, 50)), 4))
            out.setdefault(f"poll_p99_ms_{key}", []).append(round(float(np.percentile(polls, 99)), 4))
            out.setdefault(f"replay_ms_{key}", []).append(round(_ms_per_call(eng._graph.replay, 100), 4))
    eng = engines["explain"]
    feats, counts = np.unique(eng.why, return_counts=True)
    out["flows_per_why"] = {("none" if f < 0 else eng.explain_features[f]): int(c)
                            for f, c in zip(feats, counts)}
    print(json.dumps(out))


if __name__ == "__main__":
    args = sys.argv[1:] or ["mix"]
    if args[0] == "mix":
        mix()
    elif args[0] in ("kernels", "cost"):
        assert torch.cuda.is_available(), f"{args[0]} needs a GPU"
        if args[0] == "kernels":
            kernels()
        else:
            cost(args[args.index("--engine-file") + 1] if "--engine-file" in args else None)
    else:
        sys.exit(f"unknown section {args[0]!r}: mix, kernels or cost")
