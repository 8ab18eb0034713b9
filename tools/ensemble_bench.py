"""Soft-vote ensemble measurements behind profiles/ensemble.md.  Run on an
MI355X box:

    python tools/ensemble_bench.py serve     # serve poll latency: plain / confidence / ensemble
    python tools/ensemble_bench.py kernels   # the four new kernels at 8192 and 4M rows
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/ensemble_bench.py kernels
    python tools/ensemble_bench.py trace DIR # per-kernel times out of that trace

Versions that are compared alternate inside one process, round by round,
and every round is reported, so the spread is visible next to the
difference.  One JSON line per section.  `serve` also runs on a tree
without the ensemble (it then reports the engines that tree has).
"""

import csv
import glob
import inspect
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from traffic_classifier_sdn_amd.models import load_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
SHIPPED = ("RandomForestClassifier", "GaussianNB", "LogisticRegression", "SVC", "KMeans_Clustering")
VOTERS = ["RandomForestClassifier", "GaussianNB", "LogisticRegression"]
SIZES = (8192, 4_000_000)
# the shipped ensemble's shape: forest, NB and KNN know 6 classes, logistic 4
MEMBER_CLASSES = (6, 6, 4, 6)
COLMAPS = [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [0, 2, 4, 5], [0, 1, 2, 3, 4, 5]]


def ms_per_call(fn, steps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def serve():
    """GpuServeEngine.classify over 8192 live flows, five shipped models,
    hipGraph path: whole-poll latency (snapshot, H2D, replay, D2H) and the
    graph replay alone."""
    from traffic_classifier_sdn_amd.flow.parser import replay
    from traffic_classifier_sdn_amd.flow.replay import SynthFlowSpec, TelemetryReplaySource
    from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine

    rng = np.random.default_rng(0)
    mac = lambda p: p + ":%02x:%02x:%02x:%02x:%02x" % tuple(int(v) for v in rng.integers(0, 256, 5))
    specs = [SynthFlowSpec(mac("02"), mac("06"), float(rng.uniform(1, 60)), float(rng.uniform(60, 1200)),
                           float(rng.uniform(1, 60)), float(rng.uniform(60, 1200)))
             for _ in range(8192)]
    table = replay(TelemetryReplaySource(specs=specs, seed=0).stream(2))
    models = {n: load_model(os.path.join(MODELS, n + ".npz"), device="cuda") for n in SHIPPED}
    kw = dict(capacity=8192, use_graph=True)
    engines = {"plain": GpuServeEngine(models, **kw),
               "conf": GpuServeEngine(models, confidence=True, **kw)}
    if "ensemble" in inspect.signature(GpuServeEngine.__init__).parameters:
        engines["ens"] = GpuServeEngine(models, ensemble=VOTERS, **kw)
        engines["conf_ens"] = GpuServeEngine(models, confidence=True, ensemble=VOTERS, **kw)
    out = {"section": "serve", "flows": len(table), "engines": list(engines)}
    for eng in engines.values():
        for _ in range(5):
            eng.classify(table)  # capture + warm-up
    for _ in range(5):
        for key, eng in engines.items():
            polls = []
            for _ in range(100):
                eng.classify(table)
                polls.append(eng.last_latency_s * 1e3)
            out.setdefault(f"poll_p50_ms_{key}", []).append(round(float(np.percentile(polls, 50)), 4))
            out.setdefault(f"poll_p99_ms_{key}", []).append(round(float(np.percentile(polls, 99)), 4))
            out.setdefault(f"replay_ms_{key}", []).append(round(ms_per_call(eng._graph.replay, 100), 4))
    if "conf_ens" in engines:
        out["mean_ensemble_confidence"] = float(engines["conf_ens"].confidence["ensemble"].mean())
    print(json.dumps(out))


def _kernel_calls(n):
    """{name: (callable, bytes moved per call)} at n rows."""
    from traffic_classifier_sdn_amd.ops import gpu as og
    from traffic_classifier_sdn_amd.utils.datasets import load_reference_dataset, synthetic_flow_rows

    gnb = load_model(os.path.join(MODELS, "GaussianNB.npz"), device="cuda")
    lr = load_model(os.path.join(MODELS, "LogisticRegression.npz"), device="cuda")
    knn = load_model(os.path.join(MODELS, "KNeighbors.npz"), device="cuda")
    X_real, _ = load_reference_dataset()
    X = torch.from_numpy(synthetic_flow_rows(n, seed=0, reference_X=X_real)).cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    k = knn.n_neighbors
    idx = torch.randint(0, knn.y_.numel(), (n, k), device="cuda", generator=g, dtype=torch.int32)
    y8 = knn.y_.to(torch.uint8)
    probas = []
    for cm in MEMBER_CLASSES:
        p = torch.rand(n, cm, device="cuda", generator=g)
        probas.append((p / p.sum(dim=1, keepdim=True)).contiguous())
    member_bytes = sum(4 * cm for cm in MEMBER_CLASSES)
    return {
        "gnb_proba": (lambda: og.gnb_proba(X, gnb.theta_, gnb.var_, gnb.class_prior_), n * (48 + 24)),
        "linear_proba": (lambda: og.linear_proba(X, lr.coef_, lr.intercept_), n * (48 + 16)),
        "knn_vote_proba": (lambda: og.knn_vote_proba(idx, y8, 6), n * (4 * k + k + 24)),
        "ensemble_vote": (lambda: og.ensemble_vote(probas, COLMAPS, None, 6, want_proba=False),
                          n * (member_bytes + 8)),
        "ensemble_vote_avg": (lambda: og.ensemble_vote(probas, COLMAPS, None, 6, want_proba=True),
                              n * (member_bytes + 8 + 24)),
    }


def kernels():
    """Each new kernel at 8192 and 4M rows.  ms is the wall time per call of
    back-to-back launches ending in a synchronise: at 4M rows that is the
    kernel, at 8192 rows it is the launch path (kernel times at that size
    come from the trace).  Under rocprofv3 the same launches feed `trace`."""
    out = {"section": "kernels"}
    for n in SIZES:
        for name, (fn, nbytes) in _kernel_calls(n).items():
            rounds = [ms_per_call(fn, 50 if n > 100_000 else 500) for _ in range(3)]
            out[f"{name}@{n}"] = {
                "ms": [round(r, 5) for r in rounds], "bytes": nbytes,
                "GB_per_s": [round(nbytes / (r * 1e-3) / 1e9, 1) for r in rounds],
            }
    print(json.dumps(out))


def trace(directory):
    """Per-kernel device times out of a rocprofv3 --kernel-trace CSV: median
    and minimum per (kernel, grid size), which tells the two row counts
    apart (32 blocks at 8192 rows, the 2048-block cap at 4M)."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {directory}"
    groups = {}
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                if not any(k in name for k in ("_proba_kernel", "ensemble_vote_kernel")):
                    continue
                short = name.split("(")[0].replace("void ", "")
                key = f"{short} grid {row.get('Grid_Size_X', row.get('Grid_Size', '?'))}"
                groups.setdefault(key, []).append(
                    (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = {"section": "trace"}
    for key, us in sorted(groups.items()):
        out[key] = {"calls": len(us), "median_us": round(float(np.median(us)), 2),
                    "min_us": round(float(np.min(us)), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    args = sys.argv[1:] or ["serve", "kernels"]
    if args[0] == "trace":
        trace(args[1])
    else:
        assert torch.cuda.is_available(), "needs a GPU"
        sections = {"serve": serve, "kernels": kernels}
        for name in args:
            sections[name]()
