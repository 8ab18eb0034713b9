"""Forest class-score measurements behind profiles/rf_proba.md.  Run on an
MI355X box:

    python tools/rf_proba_bench.py proba100k   # device predict_proba vs the torch traversal
    python tools/rf_proba_bench.py serve       # serve poll latency, confidence off / on

Versions that are compared alternate inside one process, round by round,
and every round is reported, so the spread is visible next to the
difference.  One JSON line per section.
"""

import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from traffic_classifier_sdn_amd.models import load_model
from traffic_classifier_sdn_amd.ops import cpu as oc
from traffic_classifier_sdn_amd.ops import gpu as og
from traffic_classifier_sdn_amd.utils.datasets import load_reference_dataset, synthetic_flow_rows

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
SHIPPED = ("RandomForestClassifier", "GaussianNB", "LogisticRegression", "SVC", "KMeans_Clustering")


def ms_per_call(fn, steps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def rows(n):
    X_real, _ = load_reference_dataset()
    return torch.from_numpy(synthetic_flow_rows(n, seed=0, reference_X=X_real)).cuda()


def proba100k():
    """RandomForestClassifier.predict_proba at 100 000 rows: the scores
    kernel against the torch level-by-level traversal that ops.gpu aliased
    before (ops.cpu.rf_predict_proba on CUDA tensors)."""
    rf = load_model(os.path.join(MODELS, "RandomForestClassifier.npz"), device="cuda")
    X = rows(100_000)
    new, old = og.rf_predict_proba(X, rf.forest), oc.rf_predict_proba(X, rf.forest)
    out = {"section": "proba100k", "max_abs_diff": float((new - old).abs().max()),
           "kernel_ms": [], "torch_ms": []}
    for _ in range(3):
        out["kernel_ms"].append(ms_per_call(lambda: og.rf_predict_proba(X, rf.forest), 50))
        out["torch_ms"].append(ms_per_call(lambda: oc.rf_predict_proba(X, rf.forest), 2, warmup=1))
    print(json.dumps(out))


def serve():
    """GpuServeEngine.classify over 8192 live flows, five shipped models,
    hipGraph path: whole-poll latency (snapshot, H2D, replay, D2H) and the
    graph replay alone, confidence off and on."""
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
    engines = {"off": GpuServeEngine(models, capacity=8192, use_graph=True),
               "on": GpuServeEngine(models, capacity=8192, use_graph=True, confidence=True)}
    out = {"section": "serve", "flows": len(table)}
    for eng in engines.values():
        for _ in range(5):
            eng.classify(table)  # capture + warm-up
    for _ in range(5):
        for key, eng in engines.items():
            polls = []
            for _ in range(100):
                eng.classify(table)
                polls.append(eng.last_latency_s * 1e3)
            out.setdefault(f"poll_p50_ms_{key}", []).append(float(np.percentile(polls, 50)))
            out.setdefault(f"poll_p99_ms_{key}", []).append(float(np.percentile(polls, 99)))
            out.setdefault(f"replay_ms_{key}", []).append(ms_per_call(eng._graph.replay, 100))
    conf = engines["on"].confidence["RandomForestClassifier"]
    out["mean_confidence"] = float(conf.mean())
    print(json.dumps(out))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    sections = {"proba100k": proba100k, "serve": serve}
    for name in sys.argv[1:] or list(sections):
        sections[name]()
