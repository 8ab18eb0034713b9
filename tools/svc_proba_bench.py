"""SVC class-probability measurements behind profiles/svc_proba.md.  Run on
an MI355X box:

    python tools/svc_proba_bench.py kernels   # decision + couple against the label kernel
    python tools/svc_proba_bench.py serve     # serve poll, plain against calibrated SVC

    python tools/svc_proba_bench.py reject    # CPU: the README's kept-share table

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
from traffic_classifier_sdn_amd.utils.datasets import (
    load_reference_dataset,
    load_six_class_dataset,
    synthetic_flow_rows,
)

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


def calibrated_shipped(device):
    """The shipped SVC with sigmoids fitted on 3000 rows of the six-class
    dataset (rows 2100..5100 of its seed-0 permutation); also returns the
    800 rows after them."""
    X, y = load_six_class_dataset()
    perm = np.random.RandomState(0).permutation(len(X))
    svc = load_model(os.path.join(MODELS, "SVC.npz"), device=device)
    rows = perm[2100:5100]
    held = perm[5100:5900]
    return svc, svc.calibrate(X[rows], y[rows]), X[held], y[held]


def kernels():
    """svc_decision + svc_couple against svc_predict alone, shipped model
    (2281 SVs), at 8192 rows (wave kernels) and 2^20 rows (tiled kernels)."""
    from traffic_classifier_sdn_amd.ops import gpu as og

    svc, cal, _, _ = calibrated_shipped("cuda")
    X_real, _ = load_reference_dataset()
    args = (cal.support_vectors_, cal.dual_coef_, cal.intercept_, cal.n_support_, cal.gamma_)
    for n, steps in ((8192, 200), (1 << 20, 10)):
        X = torch.from_numpy(synthetic_flow_rows(n, seed=0, reference_X=X_real)).cuda()
        sc = cal._sv_classes(X.device)
        dec = og.svc_decision(X, *args, svclass=sc)
        labels = og.svc_predict(X, *args, svclass=sc)
        _, idx, _ = og.svc_couple(dec, cal.probA_, cal.probB_, 6)
        out = {"section": "kernels", "rows": n, "nsv": int(cal.support_vectors_.shape[0]),
               "votes_equal_labels": bool(torch.equal(idx, labels)),
               "predict_ms": [], "decision_ms": [], "couple_ms": [], "scores_ms": []}
        for _ in range(5):
            out["predict_ms"].append(ms_per_call(lambda: og.svc_predict(X, *args, svclass=sc), steps))
            out["decision_ms"].append(ms_per_call(lambda: og.svc_decision(X, *args, svclass=sc), steps))
            out["couple_ms"].append(ms_per_call(lambda: og.svc_couple(dec, cal.probA_, cal.probB_, 6), steps))
            out["scores_ms"].append(ms_per_call(lambda: cal.predict_scores(X), steps))
        print(json.dumps(out))


def serve():
    """GpuServeEngine.classify over 8192 live flows, five shipped models,
    hipGraph path, confidence on: the plain SVC (labels only) against the
    calibrated one (labels and confidence)."""
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
    _, cal, _, _ = calibrated_shipped("cuda")
    engines = {"plain": GpuServeEngine(models, capacity=8192, use_graph=True, confidence=True),
               "calibrated": GpuServeEngine({**models, "SVC": cal}, capacity=8192, use_graph=True,
                                            confidence=True)}
    out = {"section": "serve", "flows": len(table)}
    res = {}
    for key, eng in engines.items():
        for _ in range(5):
            res[key] = eng.classify(table)  # capture + warm-up
    out["svc_labels_equal"] = bool(np.array_equal(res["plain"]["SVC"], res["calibrated"]["SVC"]))
    for _ in range(5):
        for key, eng in engines.items():
            polls = []
            for _ in range(100):
                eng.classify(table)
                polls.append(eng.last_latency_s * 1e3)
            out.setdefault(f"poll_p50_ms_{key}", []).append(float(np.percentile(polls, 50)))
            out.setdefault(f"poll_p99_ms_{key}", []).append(float(np.percentile(polls, 99)))
            out.setdefault(f"replay_ms_{key}", []).append(ms_per_call(eng._graph.replay, 100))
    out["mean_svc_confidence"] = float(engines["calibrated"].confidence["SVC"].mean())
    print(json.dumps(out))


def reject():
    """CPU: share of rows kept and vote accuracy on them at a confidence
    threshold, calibrated shipped model, 800 held-out rows."""
    _, cal, X, y = calibrated_shipped("cpu")
    labels, conf = cal.predict_with_confidence(X)
    proba = cal.predict_proba(X)
    ok = labels == y
    out = {"section": "reject", "rows": len(y), "accuracy_all": float(ok.mean()),
           "vote_differs_from_argmax": float((cal.classes_[proba.argmax(axis=1)] != labels).mean())}
    for t in (0.5, 0.7, 0.9):
        keep = conf >= t
        out[f"kept_{t}"] = float(keep.mean())
        out[f"accuracy_{t}"] = float(ok[keep].mean())
    print(json.dumps(out))


if __name__ == "__main__":
    sections = {"kernels": kernels, "serve": serve, "reject": reject}
    names = sys.argv[1:] or ["kernels", "serve"]
    if any(n != "reject" for n in names):
        assert torch.cuda.is_available(), "needs a GPU"
    for name in names:
        sections[name]()
