"""Per-flow smoothing measurements behind profiles/smooth.md and the README
table.

    python tools/smooth_bench.py flicker    # CPU: label changes per flow, raw and smoothed
    python tools/smooth_bench.py cost       # MI355X: serve poll with and without smooth=
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/smooth_bench.py cost
    python tools/smooth_bench.py trace DIR  # the vote and smoothing kernels out of that trace

`flicker` replays the default four flows for 80 polls, classifies after
every poll, and counts per flow the polls at which its label differs from
the poll before.  `cost` alternates the two engines inside one process,
round by round, and reports every round.  One JSON line per section.
"""

import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from traffic_classifier_sdn_amd.models import FlowSmoother, SoftVoteEnsemble, load_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "data", "ref_models")
VOTERS = ["RandomForestClassifier", "GaussianNB", "LogisticRegression"]
DEFAULT_MEMBERS = ["RandomForestClassifier", "GaussianNB", "LogisticRegression", "KNeighbors"]
POLLS = 80
ALPHA = 0.3


def _load(name, device):
    return load_model(os.path.join(MODELS, name + ".npz"), device=device)


def label_changes(labels):
    """labels [polls, flows] -> per flow, the polls whose label differs from
    the poll before."""
    labels = np.asarray(labels)
    return [int(v) for v in (labels[1:] != labels[:-1]).sum(axis=0)]


def flicker_run(model, seed, margins, polls=POLLS, alpha=ALPHA):
    """{'raw': changes per flow, margin: changes per flow, ...} of one
    replay: the model's own argmax, and a FlowSmoother per margin fed the
    same probabilities."""
    from traffic_classifier_sdn_amd.flow.parser import PollStreamParser
    from traffic_classifier_sdn_amd.flow.replay import TelemetryReplaySource

    src = TelemetryReplaySource(seed=seed)
    parser = PollStreamParser()
    smoothers = {m: FlowSmoother(len(model.classes_), 8, alpha, m) for m in margins}
    seen = {"raw": [], **{m: [] for m in margins}}
    for _ in range(polls):
        for line in src.poll():
            parser.feed(line)
        X = parser.table.feature_matrix(dtype=np.float32)
        proba = torch.as_tensor(model.predict_proba(X)).to(torch.float32).contiguous()
        seen["raw"].append(proba.argmax(dim=1).numpy())
        for m, sm in smoothers.items():
            seen[m].append(sm.update(proba)[0].numpy())
    return {k: label_changes(v) for k, v in seen.items()}


def flicker():
    forest = _load("RandomForestClassifier", "cpu")
    vote = SoftVoteEnsemble({n: _load(n, "cpu") for n in DEFAULT_MEMBERS})
    out = {"section": "flicker", "polls": POLLS, "alpha": ALPHA, "margins": [0.0, 0.1]}
    for name, model in (("forest", forest), ("soft vote of the four default members", vote)):
        for seed in (0, 1):
            res = flicker_run(model, seed, (0.0, 0.1))
            out[f"{name}, seed {seed}"] = {
                "raw": res["raw"], "margin 0": res[0.0], "margin 0.1": res[0.1],
            }
    print(json.dumps(out))
    print("| model | seed | raw argmax | smoothed α=0.3, margin 0 | smoothed α=0.3, margin 0.1 |")
    print("|---|---|---|---|---|")
    for key, res in out.items():
        if not isinstance(res, dict):
            continue
        name, seed = key.rsplit(", seed ", 1)
        cells = [" / ".join(str(v) for v in res[k]) + f" (total {sum(res[k])})"
                 for k in ("raw", "margin 0", "margin 0.1")]
        print(f"| {name} | {seed} | " + " | ".join(cells) + " |")


def _ms_per_call(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def cost():
    """GpuServeEngine.classify over 8192 live flows, forest + NB + logistic
    with ensemble=, hipGraph path, with smooth=None and smooth=0.3: whole-poll
    latency and the graph replay alone.  Then the oracle's torch formulation
    of the smoothing step on the vote's device tensors, per call: what the
    step costs when it is not one kernel."""
    from traffic_classifier_sdn_amd.flow.parser import replay
    from traffic_classifier_sdn_amd.flow.replay import SynthFlowSpec, TelemetryReplaySource
    from traffic_classifier_sdn_amd.ops import cpu as oc
    from traffic_classifier_sdn_amd.ops import gpu as og
    from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine

    n = 8192
    rng = np.random.default_rng(0)
    mac = lambda p: p + ":%02x:%02x:%02x:%02x:%02x" % tuple(int(v) for v in rng.integers(0, 256, 5))
    specs = [SynthFlowSpec(mac("02"), mac("06"), float(rng.uniform(1, 60)), float(rng.uniform(60, 1200)),
                           float(rng.uniform(1, 60)), float(rng.uniform(60, 1200)))
             for _ in range(n)]
    table = replay(TelemetryReplaySource(specs=specs, seed=0).stream(2))
    models = {name: _load(name, "cuda") for name in VOTERS}
    kw = dict(capacity=n, use_graph=True, ensemble=VOTERS)
    engines = {"vote": GpuServeEngine(models, **kw),
               "smooth": GpuServeEngine(models, smooth=ALPHA, switch_margin=0.1, **kw)}
    out = {"section": "cost", "flows": len(table), "engines": list(engines)}
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
            out.setdefault(f"replay_ms_{key}", []).append(round(_ms_per_call(eng._graph.replay, 100), 4))
    out["mean_smoothed_confidence"] = float(engines["smooth"].confidence["smoothed"].mean())

    # the step alone, eager, on the same kind of tensors: kernel and torch
    g = torch.Generator(device="cuda").manual_seed(0)
    C = len(engines["smooth"].ensemble.classes_)
    p = torch.rand(n, C, device="cuda", generator=g)
    p = (p / p.sum(dim=1, keepdim=True)).contiguous()
    live = torch.tensor([n], dtype=torch.int32, device="cuda")
    for key, fn in (("kernel", og.proba_smooth), ("torch", oc.proba_smooth)):
        state = torch.zeros(n, C, device="cuda")
        held = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        call = lambda: fn(p, state, held, ALPHA, 0.1, live)
        out[f"step_eager_ms_{key}"] = [round(_ms_per_call(call, 200), 4) for _ in range(3)]
    print(json.dumps(out))


def trace(directory):
    """Device times of the vote and smoothing kernels out of a rocprofv3
    --kernel-trace CSV: calls, median and minimum per kernel and grid."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {directory}"
    groups = {}
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                if not any(k in name for k in ("proba_smooth_kernel", "ensemble_vote_kernel")):
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
    args = sys.argv[1:] or ["flicker"]
    if args[0] == "trace":
        trace(args[1])
    elif args[0] == "flicker":
        flicker()
    elif args[0] == "cost":
        assert torch.cuda.is_available(), "cost needs a GPU"
        cost()
    else:
        sys.exit(f"unknown section {args[0]!r}: flicker, cost or trace DIR")
