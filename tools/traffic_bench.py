"""Per-class traffic accounting: the numbers behind profiles/traffic.md and the
README table.

    python tools/traffic_bench.py mix         # CPU: the per-class table of the replay source
    python tools/traffic_bench.py gpu         # MI355X: the serve poll, then op timings
    python tools/traffic_bench.py gpu --no-torch --engine-file OLD_SERVE_GPU.py
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/traffic_bench.py kernels
    python tools/traffic_bench.py trace DIR   # the two kernels out of that trace

`mix` replays the default four flows for 80 polls with the shipped forest
and prints what `--summary` shows after the last poll, for seeds 0 and 1.
`gpu` alternates serve engines with and without traffic= inside one process,
round by round, and reports every round; then it times ops.class_traffic
and (unless --no-torch) the same reduction in torch (index_add_) between
device events, several rounds, all listed.
--engine-file adds a third engine built from another revision's
serve_gpu.py (same package, same kernels), to put the engine without
traffic= next to what it was.  `kernels` only launches the op (for a
profiler), `trace` reads the device times back.  One JSON line per section.
"""

import csv
import glob
import importlib.util
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
VOTERS = ["RandomForestClassifier", "GaussianNB", "LogisticRegression"]
POLLS = 80
SIZES = (8192, 1 << 20, 10_000_000)
C = 6


def _load(name, device):
    return load_model(os.path.join(MODELS, name + ".npz"), device=device)


def mix():
    from traffic_classifier_sdn_amd import ops
    from traffic_classifier_sdn_amd.flow.parser import PollStreamParser
    from traffic_classifier_sdn_amd.flow.replay import TelemetryReplaySource
    from traffic_classifier_sdn_amd.serve import render_traffic_summary, traffic_rates

    forest = _load("RandomForestClassifier", "cpu")
    classes = [str(c) for c in forest.classes_] + ["unknown"]
    out = {"section": "mix", "polls": POLLS, "model": "RandomForestClassifier"}
    for seed in (0, 1):
        src = TelemetryReplaySource(seed=seed)
        parser = PollStreamParser()
        for _ in range(POLLS):
            for line in src.poll():
                parser.feed(line)
        X = torch.from_numpy(np.ascontiguousarray(parser.table.feature_matrix(dtype=np.float32)))
        labels = forest.predict_index(X).to(torch.int32)
        totals = ops.class_traffic(X, labels, len(classes) - 1).numpy()
        out[f"seed {seed}"] = traffic_rates(classes, totals)
        print(f"seed {seed}, {len(parser.table)} flows after {POLLS} polls")
        print(render_traffic_summary(classes, totals))
    print(json.dumps(out))


def _inputs(n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.exp(8.0 + 4.0 * torch.randn(n, 12, device="cuda", generator=g)).contiguous()
    labels = torch.randint(-1, C + 1, (n,), device="cuda", generator=g, dtype=torch.int32)
    conf = torch.rand(n, device="cuda", generator=g)
    return X, labels, conf


def _us_per_call(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps * 1e3


def _rounds(fn, budget_s=4.0, rounds=5):
    """(reps, [us per call of each round]): `reps` calls back to back between
    two device events per round.  reps comes from two calls timed alone, so
    that the rounds fit `budget_s` whatever a call costs: torch's index_add_
    into 9 rows serialises its atomics, and how long that takes at 10M rows
    was not known before it was measured."""
    _us_per_call(fn, 1)  # first call: code objects, allocator
    one = _us_per_call(fn, 1) * 1e-6
    reps = max(1, min(200, int(budget_s / rounds / one)))
    if one * rounds > budget_s:
        rounds = max(1, int(budget_s / one))
    return reps, [round(_us_per_call(fn, reps), 2) for _ in range(rounds)]


def op_times(torch_too):
    """ops.gpu.class_traffic (two kernels and two small allocations per call)
    and, with `torch_too`, ops.cpu.class_traffic on the same device tensors
    (torch's index_add_ and what feeds it).  One JSON line per size.  Bytes
    read per row: 48 of features and 4 of label, and 4 of confidence when it
    is given."""
    from traffic_classifier_sdn_amd.ops import cpu as oc
    from traffic_classifier_sdn_amd.ops import gpu as og

    entries = [("kernel", og.class_traffic, False, 52), ("kernel_conf", og.class_traffic, True, 56)]
    if torch_too:
        entries.append(("torch", oc.class_traffic, False, None))
    for n in SIZES:
        X, labels, conf = _inputs(n)
        res = {"section": "op", "rows": n, "classes": C}
        for key, fn, with_conf, per_row in entries:
            call = lambda: fn(X, labels, C, conf if with_conf else None, 0.5)
            res[f"{key}_reps"], res[f"{key}_us"] = _rounds(call)
            if per_row:
                res[f"{key}_TBps"] = [round(n * per_row / (us * 1e-6) / 1e12, 3)
                                      for us in res[f"{key}_us"]]
        if torch_too:
            got = og.class_traffic(X, labels, C, conf, 0.5)
            want = oc.class_traffic(X, labels, C, conf, 0.5)
            res["max_rel_diff_kernel_vs_torch"] = float(
                ((got - want).abs() / want.abs().clamp(min=1e-300)).max())
            res["counts_equal"] = bool(torch.equal(got[:, 0], want[:, 0]))
        print(json.dumps(res), flush=True)
        del X, labels, conf


def _kernel_calls(n):
    """Calls per variant that `kernels` makes at n rows; `trace` counts on it."""
    return 50 if n <= 1 << 20 else 20


def kernels():
    """Launches only, for a profiler: the op at every size in turn, without
    and with a confidence, alternating."""
    from traffic_classifier_sdn_amd.ops import gpu as og

    for n in SIZES:
        X, labels, conf = _inputs(n)
        for _ in range(_kernel_calls(n)):
            og.class_traffic(X, labels, C)
            og.class_traffic(X, labels, C, conf, 0.5)
        torch.cuda.synchronize()
        del X, labels, conf
    print(json.dumps({"section": "kernels", "sizes": list(SIZES)}))


def _ms_per_call(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def _engine_class(path):
    """GpuServeEngine out of another revision's serve_gpu.py, loaded as a
    module of this package so that its relative imports find this tree."""
    name = "traffic_classifier_sdn_amd._other_serve_gpu"
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod.GpuServeEngine


def cost(engine_file=None):
    """GpuServeEngine.classify over 8192 live flows, forest + NB + logistic
    with ensemble=, hipGraph path, without traffic= and with
    traffic="ensemble": whole-poll latency and the graph replay alone."""
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
    kw = dict(capacity=n, use_graph=True, ensemble=VOTERS)
    engines = {}
    if engine_file:
        engines["other"] = _engine_class(engine_file)(models, **kw)
    engines["off"] = GpuServeEngine(models, **kw)
    engines["traffic"] = GpuServeEngine(models, traffic="ensemble", **kw)
    engines["traffic_conf"] = GpuServeEngine(
        models, traffic="ensemble", traffic_min_confidence=0.5, **kw)
    out = {"section": "cost", "flows": len(table), "engines": list(engines)}
    labels = {}
    for key, eng in engines.items():
        for _ in range(5):
            labels[key] = eng.classify(table)  # capture + warm-up
    for key in labels:
        assert all(np.array_equal(labels[key][m], labels["off"][m]) for m in labels["off"]), key
    for _ in range(5):
        for key, eng in engines.items():
            polls = []
            for _ in range(100):
                eng.classify(table)
                polls.append(eng.last_latency_s * 1e3)
            out.setdefault(f"poll_p50_ms_{key}", []).append(round(float(np.percentile(polls, 50)), 4))
            out.setdefault(f"poll_p99_ms_{key}", []).append(round(float(np.percentile(polls, 99)), 4))
            out.setdefault(f"replay_ms_{key}", []).append(round(_ms_per_call(eng._graph.replay, 100), 4))
    t = engines["traffic"].traffic
    out["flows_per_class"] = dict(zip(engines["traffic"].traffic_classes, t[:, 0].tolist()))
    out["unknown_with_min_confidence"] = float(engines["traffic_conf"].traffic[-1, 0])
    print(json.dumps(out))


def trace(directory):
    """Device times of the two kernels out of a rocprofv3 --kernel-trace CSV
    of `kernels`: per size and variant, calls, median, minimum and 90th
    percentile.  The trace does not carry the row count, so the launches are
    taken in start order and dealt to the sizes by the call counts of
    `kernels`; the first call of each size and variant is dropped."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {directory}"
    rows = []
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "class_traffic" in row["Kernel_Name"]:
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]),
                                 "partial" if "partial" in row["Kernel_Name"] else "finish"))
    rows.sort()
    assert len(rows) == sum(4 * _kernel_calls(n) for n in SIZES), len(rows)
    out = {"section": "trace"}
    at = 0
    for n in SIZES:
        calls = rows[at:at + 4 * _kernel_calls(n)]
        at += len(calls)
        # per call: partial, finish; calls alternate without / with a confidence
        for v, variant in enumerate(("no conf", "conf")):
            pair = [calls[i:i + 2] for i in range(2 * v, len(calls), 4)][1:]
            assert all(a[2] == "partial" and b[2] == "finish" for a, b in pair)
            for k, kernel in enumerate(("partial", "finish")):
                us = [(c[k][1] - c[k][0]) / 1e3 for c in pair]
                out[f"{n} rows, {variant}, {kernel}"] = {
                    "calls": len(us), "median_us": round(float(np.median(us)), 2),
                    "min_us": round(float(np.min(us)), 2),
                    "p90_us": round(float(np.percentile(us, 90)), 2)}
            span = [(b[1] - a[0]) / 1e3 for a, b in pair]
            out[f"{n} rows, {variant}, partial start to finish end"] = {
                "median_us": round(float(np.median(span)), 2)}
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
