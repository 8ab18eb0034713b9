"""Top talkers per class: the numbers behind profiles/top_flows.md and the
README table.

    python tools/top_flows_bench.py mix         # CPU: the three tables of the replay source
    python tools/top_flows_bench.py gpu         # MI355X: the serve poll, then op timings
    python tools/top_flows_bench.py gpu --no-torch --engine-file OLD_SERVE_GPU.py
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/top_flows_bench.py kernels
    python tools/top_flows_bench.py trace DIR   # the two kernels out of that trace

`mix` replays the default four flows for 80 polls with the shipped forest and
prints what `--summary --top 3` shows after the last poll, seed 0.  `gpu`
alternates serve engines with traffic= alone and with top_flows=10 inside one
process, round by round, and reports every round; --engine-file adds the
engine of another revision's serve_gpu.py with traffic= (same package, same
kernels).  Then it times ops.class_top_flows per call for random row order and
for keys ascending within one class (every row an insertion), and (unless
--no-torch) the same selection in torch on the same device tensors: the
oracle, and a masked torch.topk per group.  `kernels` only launches the op
(for a profiler), `trace` reads the device times back.  One JSON line per
section.  The timing helpers are those of tools/traffic_bench.py.
"""

import csv
import glob
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from traffic_bench import _engine_class, _load, _ms_per_call, _rounds

VOTERS = ["RandomForestClassifier", "GaussianNB", "LogisticRegression"]
POLLS = 80
SIZES = (8192, 1 << 20, 10_000_000)
KS = (10, 64)
ORDERS = ("random", "ascending")
C = 6


def mix():
    from traffic_classifier_sdn_amd.flow.replay import TelemetryReplaySource
    from traffic_classifier_sdn_amd.serve import RealtimeClassifier, top_flow_lists

    forest = _load("RandomForestClassifier", "cpu")

    out = io.StringIO()
    rc = RealtimeClassifier(forest, out=out, summary=True, top=3)
    src = TelemetryReplaySource(seed=0)
    last = ""
    for _ in range(POLLS):
        for line in src.poll():
            before = out.tell()
            if rc.feed(line):
                last = out.getvalue()[before:]  # the three tables of that pass
    print(f"seed 0, {len(rc.parser.table)} flows after {POLLS} polls")
    print(last, end="")
    print(json.dumps({"section": "mix", "polls": POLLS, "model": "RandomForestClassifier",
                      "top_flows": top_flow_lists(rc.traffic_classes, rc.top_flows,
                                                  rc.top_flow_rates)}))


def _inputs(n, order, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.exp(8.0 + 4.0 * torch.randn(n, 12, device="cuda", generator=g)).contiguous()
    conf = torch.rand(n, device="cuda", generator=g)
    if order == "random":
        labels = torch.randint(-1, C + 1, (n,), device="cuda", generator=g, dtype=torch.int32)
    else:  # one class, the key strictly ascending in row order (exact below 2^24)
        labels = torch.zeros(n, device="cuda", dtype=torch.int32)
        X[:, 4] = torch.arange(n, device="cuda", dtype=torch.float32)
        X[:, 10] = 0.0
    return X, labels, conf


def _masked_topk(X, labels, k):
    """The selection as one masked torch.topk per group: no tie rule, no
    padding, no live count; what a user would write first."""
    key = X[:, 4] + X[:, 10]
    lab = labels.long()
    group = torch.where((lab >= 0) & (lab < C), lab, torch.full_like(lab, C))
    low = torch.full_like(key, float("-inf"))
    return [torch.topk(torch.where(group == g, key, low), min(k, key.numel())) for g in range(C + 1)]


def op_times(torch_too):
    """ops.gpu.class_top_flows (two kernels and three allocations per call).
    Bytes requested per row for the default columns: 32 of features and 4 of
    label (36), and 4 of confidence when it is given (40)."""
    from traffic_classifier_sdn_amd.ops import cpu as oc
    from traffic_classifier_sdn_amd.ops import gpu as og

    for n in SIZES:
        for order in ORDERS:
            X, labels, conf = _inputs(n, order)
            for k in KS:
                res = {"section": "op", "rows": n, "classes": C, "k": k, "order": order}
                res["kernel_reps"], res["kernel_us"] = _rounds(
                    lambda: og.class_top_flows(X, labels, C, k))
                res["kernel_conf_reps"], res["kernel_conf_us"] = _rounds(
                    lambda: og.class_top_flows(X, labels, C, k, conf=conf, min_conf=0.5))
                if torch_too:
                    res["topk_reps"], res["topk_us"] = _rounds(
                        lambda: _masked_topk(X, labels, k), budget_s=2.0)
                    res["oracle_reps"], res["oracle_us"] = _rounds(
                        lambda: oc.class_top_flows(X, labels, C, k), budget_s=2.0)
                    got = og.class_top_flows(X, labels, C, k, conf=conf, min_conf=0.5)
                    want = oc.class_top_flows(X, labels, C, k, conf=conf, min_conf=0.5)
                    res["equal_to_oracle"] = bool(
                        torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
                print(json.dumps(res), flush=True)
            del X, labels, conf


def _kernel_calls(n):
    """Calls per variant that `kernels` makes at n rows; `trace` counts on it."""
    return 50 if n <= 1 << 20 else 20


def kernels():
    """Launches only, for a profiler: per size, order and k in turn."""
    from traffic_classifier_sdn_amd.ops import gpu as og

    for n in SIZES:
        for order in ORDERS:
            X, labels, _ = _inputs(n, order)
            for k in KS:
                for _ in range(_kernel_calls(n)):
                    og.class_top_flows(X, labels, C, k)
                torch.cuda.synchronize()
            del X, labels
    print(json.dumps({"section": "kernels", "sizes": list(SIZES)}))


def cost(engine_file=None):
    """GpuServeEngine.classify over 8192 live flows, forest + NB + logistic
    with ensemble= and traffic="ensemble", hipGraph path, without and with
    top_flows=10: whole-poll latency and the graph replay alone."""
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
    models = {name: _load(name, "cuda") for name in VOTERS}
    kw = dict(capacity=n, use_graph=True, ensemble=VOTERS, traffic="ensemble")
    engines = {}
    if engine_file:
        engines["other"] = _engine_class(engine_file)(models, **kw)
    engines["traffic"] = GpuServeEngine(models, **kw)
    engines["top10"] = GpuServeEngine(models, top_flows=10, **kw)
    out = {"section": "cost", "flows": len(table), "engines": list(engines)}
    labels = {}
    for key, eng in engines.items():
        for _ in range(5):
            labels[key] = eng.classify(table)  # capture + warm-up
    for key, eng in engines.items():
        assert all(np.array_equal(labels[key][m], labels["traffic"][m]) for m in labels[key]), key
        assert np.array_equal(eng.traffic, engines["traffic"].traffic), key
    for _ in range(5):
        for key, eng in engines.items():
            polls = []
            for _ in range(100):
                eng.classify(table)
                polls.append(eng.last_latency_s * 1e3)
            out.setdefault(f"poll_p50_ms_{key}", []).append(round(float(np.percentile(polls, 50)), 4))
            out.setdefault(f"poll_p99_ms_{key}", []).append(round(float(np.percentile(polls, 99)), 4))
            out.setdefault(f"replay_ms_{key}", []).append(round(_ms_per_call(eng._graph.replay, 100), 4))
    top = engines["top10"]
    out["flows_per_class"] = dict(zip(top.traffic_classes, top.traffic[:, 0].tolist()))
    out["listed_per_class"] = dict(zip(top.traffic_classes, (top.top_flows >= 0).sum(1).tolist()))
    print(json.dumps(out))


def trace(directory):
    """Device times of the two kernels out of a rocprofv3 --kernel-trace CSV
    of `kernels`: per size, order and k, calls, median, minimum and 90th
    percentile.  The trace does not carry the arguments, so the launches are
    taken in start order and dealt out by the call counts of `kernels`; the
    first call of each cell is dropped."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {directory}"
    rows = []
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "class_top_flows" in row["Kernel_Name"]:
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]),
                                 "partial" if "partial" in row["Kernel_Name"] else "finish"))
    rows.sort()
    assert len(rows) == sum(2 * len(ORDERS) * len(KS) * _kernel_calls(n) for n in SIZES), len(rows)
    out = {"section": "trace"}
    at = 0
    for n in SIZES:
        for order in ORDERS:
            for k in KS:
                calls = rows[at:at + 2 * _kernel_calls(n)]
                at += len(calls)
                pair = [calls[i:i + 2] for i in range(0, len(calls), 2)][1:]
                assert all(a[2] == "partial" and b[2] == "finish" for a, b in pair)
                for j, kernel in enumerate(("partial", "finish")):
                    us = [(c[j][1] - c[j][0]) / 1e3 for c in pair]
                    out[f"{n} rows, {order}, k {k}, {kernel}"] = {
                        "calls": len(us), "median_us": round(float(np.median(us)), 2),
                        "min_us": round(float(np.min(us)), 2),
                        "p90_us": round(float(np.percentile(us, 90)), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    args = sys.argv[1:] or ["mix"]
    if args[0] == "mix":
        mix()
    elif args[0] == "trace":
        trace(args[1])
    elif args[0] in ("gpu", "kernels"):
        assert torch.cuda.is_available(), f"{args[0]} needs a GPU"
        if args[0] == "kernels":
            kernels()
        else:
            engine_file = args[args.index("--engine-file") + 1] if "--engine-file" in args else None
            cost(engine_file)
            op_times(torch_too="--no-torch" not in args)
    else:
        sys.exit(f"unknown section {args[0]!r}: mix, gpu, kernels or trace DIR")
