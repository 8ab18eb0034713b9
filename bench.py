"""Benchmarks for the BASELINE.json configs on MI355X.

Flagship (driver contract, default):
    python bench.py --gpus N --steps K --warmup W [--rows-per-gpu R]
runs the RandomForest (100 trees, 6-class) predict throughput on synthetic
flow-stat rows (config #2), weak-scaled over N GPUs (one rank per GPU, RCCL).
Rank 0 prints ONE JSON line; elapsed is the MAX over ranks, timed region
bracketed by barrier + torch.cuda.synchronize on both sides.

Extra workloads (same JSON contract, run explicitly):
    --workload knn           config #4: k=5 brute-force, reference set
                             sharded across ranks (12.5M rows/GPU -> 100M at
                             8), per-step top-k + RCCL all-gather merge over
                             64K query rows; --knn-approx switches to the
                             bf16 coarse-pass selection (exact refine,
                             measured recall)
    --workload svc-fit       config #3 inner loop: fixed block of fused SMO
                             iterations on 1M rows, strong-scaled
    --workload svc-fit-full  config #3 proper: the full 6-class one-vs-one
                             fit, all 15 pairs to tolerance, held-out
                             accuracy reported untimed
    --workload serve         config #5: full poll cycle — counter snapshot
                             -> H2D -> hipGraph replay of feature-extract +
                             5-model ensemble predict -> D2H labels
    --workload rf-fit        level-synchronous histogram forest build

A plain run does only what the headline figure needs: set up, warm up, time
the K steps, print the result line.  Two options add to that:
    --full               also run the untimed extras of the workload (the RF
                         flagship's 5-class accuracy on the shipped rows and
                         the 6-class refit + accuracy) and report them in
                         the result line's "config"
    --dump-outputs DIR   after the timed steps, write what the last timed
                         step returned as DIR/<name>.npy (float32/float64,
                         <= 64 MB in all; larger outputs are written as a
                         fixed seeded sample).  Inputs depend only on the
                         arguments, so two builds can be compared output
                         for output.

The forest/model shapes are the reference's own checkpoints (converted to
data/ref_models/*.npz), so model config matches the named baseline; data is
synthetic (no network for datasets) with the real rows' scale/jitter.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import Optional

# Cap the OpenMP/BLAS pool BEFORE torch import: GPU boxes run under a cgroup
# CPU quota (cpu.max 16/100ms here) and a full-width spin-waiting thread pool
# exhausts it, freezing the whole process ~90 ms per period — measured as a
# p99 latency cliff on the 1 ms serve path (profiles/serve_latency_r01.md).
os.environ.setdefault("OMP_NUM_THREADS", "4")

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from traffic_classifier_sdn_amd.models import load_model
from traffic_classifier_sdn_amd.parallel import dist
from traffic_classifier_sdn_amd.utils.datasets import (
    load_reference_dataset,
    synthetic_flow_rows,
    train_test_split_ref,
)
from traffic_classifier_sdn_amd.utils.metrics import accuracy

REPO = os.path.dirname(os.path.abspath(__file__))
RF_CKPT = os.path.join(REPO, "data", "ref_models", "RandomForestClassifier.npz")


# what the last timed step returned (kept for --dump-outputs)
_LAST_OUTPUT = [None]

# --dump-outputs budget for all arrays of one run together
DUMP_MAX_BYTES = 64 * 1000 * 1000


def _timed(step, steps: int, warmup: int, use_gpu: bool) -> float:
    """Warmup, barrier+sync, time K steps, barrier+sync; MAX over ranks."""
    for _ in range(warmup):
        step()
    if use_gpu:
        torch.cuda.synchronize()
    dist.barrier()
    out = None
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    if use_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    # NCCL collectives need device tensors (a CPU tensor would fail at N>1)
    e = torch.tensor([elapsed], dtype=torch.float64,
                     device="cuda" if use_gpu else "cpu")
    if dist.is_initialized():
        torch.distributed.all_reduce(e, op=torch.distributed.ReduceOp.MAX)
    dist.barrier()
    _LAST_OUTPUT[0] = out
    return float(e[0])


def _dump_outputs(args, rank: int, arrays: dict) -> None:
    """Write the last timed step's outputs as <--dump-outputs>/<name>.npy
    (rank 0's shard on a multi-rank run; no-op without the option).

    Floating arrays keep float32/float64; everything else (label indices,
    counts) is written as float32 when every value is exactly representable
    there, else float64.  When the arrays together exceed DUMP_MAX_BYTES each
    is cut to its share of the budget by a seeded, sorted row sample, so the
    same arguments always pick the same rows.
    """
    out_dir, seed = args.dump_outputs, args.seed
    if not out_dir or rank != 0:
        return
    os.makedirs(out_dir, exist_ok=True)
    conv = {}
    for name, a in arrays.items():
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        if a.dtype not in (np.float32, np.float64):
            exact32 = a.size == 0 or float(np.abs(a).max()) <= 2.0 ** 24
            a = a.astype(np.float32 if exact32 else np.float64)
        conv[name] = a.reshape(-1) if a.ndim == 0 else a
    share = DUMP_MAX_BYTES // max(1, len(conv))
    over = sum(v.nbytes for v in conv.values()) > DUMP_MAX_BYTES
    for name, a in conv.items():
        if over and a.nbytes > share:
            row_bytes = max(1, a.nbytes // a.shape[0])
            keep = max(1, share // row_bytes)
            idx = np.sort(np.random.default_rng(seed).choice(a.shape[0], size=keep, replace=False))
            a = a[idx]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def _emit(rank, metric, value, unit, world, args, ms_per_step, scaling, config):
    if rank != 0:
        return
    print(
        json.dumps(
            {
                "metric": metric,
                "value": value,
                "unit": unit,
                "n_gpus": world,
                "steps": args.steps,
                "warmup": args.warmup,
                "ms_per_step": ms_per_step,
                "higher_is_better": True,
                "scaling": scaling,
                "vs_baseline": None,
                "dtype": "fp32",
                "data": "synthetic",
                "config": config,
            }
        )
    )


def bench_rf(args, rank, world, device, use_gpu):
    model = load_model(RF_CKPT, device=device)
    X_real, y_real = load_reference_dataset()
    config = {
        "model": "RandomForestClassifier-100trees-6class",
        "global_batch": args.rows_per_gpu * world,
        "seq_len": 12,
        "parallelism": f"dp{world}",
        "dtype_note": "f32 features/thresholds, prediction-parity-tested vs f64 sklearn oracles; fit paths accumulate f64",
    }
    if args.full:
        # measured (non-timed) accuracies, reference split protocol.  The
        # reference's 6_quake_training_data.csv is NOT shipped (SURVEY §2.1
        # C11), so the shipped rows cover 5 classes; the 6-class number refits
        # on shipped rows + synthetic quake (D-ITG Quake3 replay through the
        # real collection path) and is labelled _quake_synth accordingly.
        _, Xte, _, yte = train_test_split_ref(X_real, y_real)
        acc5 = accuracy(yte, model.predict(Xte))
        from traffic_classifier_sdn_amd.models import RandomForestClassifier
        from traffic_classifier_sdn_amd.utils.datasets import load_six_class_dataset

        X6, y6 = load_six_class_dataset(seed=args.seed)
        Xtr6, Xte6, ytr6, yte6 = train_test_split_ref(X6, y6)
        m6 = RandomForestClassifier(
            n_estimators=100, seed=args.seed,
            builder="hist" if use_gpu else "exact", device=device,
        ).fit(Xtr6, ytr6)
        acc6 = accuracy(yte6, m6.predict(Xte6))
        config.update({
            "accuracy_6class_quake_synth": acc6,
            "accuracy_5class_shipped": acc5,
            "accuracy_published_ref_6class": 0.9987,
            "quake_note": "reference's 6_quake_training_data.csv (1244 rows) is not shipped; 6th class synthesized via D-ITG Quake3 replay (utils.datasets.synthesize_quake_rows)",
        })

    Xn = synthetic_flow_rows(args.rows_per_gpu, seed=args.seed + 1000 * rank, reference_X=X_real)
    X = torch.from_numpy(Xn).to(device)
    if use_gpu:
        torch.cuda.synchronize()

    elapsed = _timed(lambda: model.predict_index(X), args.steps, args.warmup, use_gpu)
    total_rows = args.rows_per_gpu * world * args.steps
    # what a caller of predict_index receives: one class index per row
    _dump_outputs(args, rank, {"rf_predict_index": _LAST_OUTPUT[0]})
    _emit(
        rank,
        "flows/sec, RandomForest 100-tree 6-class predict on synthetic flow-stat rows",
        total_rows / elapsed,
        "flows/s",
        world,
        args,
        elapsed / args.steps * 1000.0,
        "weak",
        config,
    )


def bench_knn(args, rank, world, device, use_gpu):
    """Config #4: sharded-reference brute-force KNN with all-gather merge."""
    from traffic_classifier_sdn_amd.models import KNeighborsClassifier

    ref_rows = args.knn_ref_rows_per_gpu
    X_real, _ = load_reference_dataset()
    Xref = synthetic_flow_rows(ref_rows, seed=args.seed + 7000 + 1000 * rank, reference_X=X_real)
    yref = np.random.default_rng(args.seed + rank).integers(0, 6, size=ref_rows)
    m = KNeighborsClassifier(n_neighbors=5, batch_rows=args.knn_queries,
                             device=device, approx=args.knn_approx)
    m.fit(Xref, yref, sharded=world > 1)
    Q = torch.from_numpy(
        synthetic_flow_rows(args.knn_queries, seed=args.seed + 31 + rank, reference_X=X_real)
    ).to(device)
    if use_gpu:
        torch.cuda.synchronize()

    elapsed = _timed(lambda: m.predict_index(Q), args.steps, args.warmup, use_gpu)
    total_q = args.knn_queries * world * args.steps
    _dump_outputs(args, rank, {"knn_predict_index": _LAST_OUTPUT[0]})
    _emit(
        rank,
        "queries/sec, KNeighbors k=5 brute-force over sharded reference set (RCCL all-gather top-k)",
        total_q / elapsed,
        "queries/s",
        world,
        args,
        elapsed / args.steps * 1000.0,
        "weak",
        {
            "model": "KNeighbors-k5",
            "global_batch": args.knn_queries * world,
            "seq_len": 12,
            "parallelism": f"shard{world}",
            "reference_rows_total": ref_rows * world,
            "reference_rows_per_gpu": ref_rows,
            "selection": "bf16-coarse+exact-refine" if args.knn_approx else "exact-f32",
        },
    )


def bench_svc_fit(args, rank, world, device, use_gpu):
    """Config #3: SMO iteration throughput on 1M rows, strong-scaled."""
    from traffic_classifier_sdn_amd.models.svc_fit import smo_fit_pair

    n_total = args.svc_rows
    n_local = n_total // world
    rng = np.random.default_rng(args.seed + rank)
    X_real, _ = load_reference_dataset()
    Xn = synthetic_flow_rows(n_local, seed=args.seed + 50 + rank, reference_X=X_real).astype(np.float32)
    # separable-ish binary labels over two features (one OVO subproblem)
    y = np.where(Xn[:, 0] + 0.3 * Xn[:, 6] > np.median(Xn[:, 0]), 1.0, -1.0).astype(np.float32)
    X = torch.from_numpy(Xn).to(device)
    yt = torch.from_numpy(y).to(device)
    gamma = 1.0 / (12 * float(X.var()))
    iters = args.svc_iters_per_step
    if use_gpu:
        torch.cuda.synchronize()

    done = []

    def step():
        alpha, b, it = smo_fit_pair(X, yt, C=1.0, gamma=gamma, tol=0.0, max_iter=iters)
        done.append(it)
        return alpha, b

    elapsed = _timed(step, args.steps, args.warmup, use_gpu)
    timed_iters = sum(done[args.warmup :])
    alpha, b = _LAST_OUTPUT[0]
    _dump_outputs(args, rank, {"svc_fit_alpha": alpha, "svc_fit_intercept": np.float64(b)})
    # each SMO iteration updates the full gradient: n_total fused kernel-row
    # evaluations -> row-updates/s is the scale-invariant rate
    row_updates = float(timed_iters) * n_total / max(1, world) * world
    _emit(
        rank,
        "SMO row-updates/sec, RBF-SVC dual fit on 1M synthetic flow rows (fused kernel-row gradient)",
        row_updates / elapsed,
        "row-updates/s",
        world,
        args,
        elapsed / args.steps * 1000.0,
        "strong",
        {
            "model": "RBF-SVC-SMO",
            "global_batch": n_total,
            "seq_len": 12,
            "parallelism": f"dp{world}",
            "rows_total": n_total,
            "smo_iters_per_step": iters,
        },
    )


def _stratified_synth_rows(n, seed, device_unused=None):
    """Class-conditional synthetic 6-class rows: sample each class's
    empirical rows (shipped 5 + synthetic quake) with multiplicative jitter,
    so the fit problem has realistic class structure at any scale."""
    from traffic_classifier_sdn_amd.utils.datasets import load_six_class_dataset

    X6, y6 = load_six_class_dataset(seed=0)
    classes = np.unique(y6.astype(str))
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, len(classes), size=n)
    X = np.empty((n, 12), dtype=np.float64)
    for c in range(len(classes)):
        pool = X6[y6.astype(str) == classes[c]]
        m = lab == c
        X[m] = pool[rng.integers(0, pool.shape[0], size=int(m.sum()))]
    X *= rng.uniform(0.9, 1.1, size=X.shape)
    return X.astype(np.float32), lab, classes


def bench_svc_fit_full(args, rank, world, device, use_gpu):
    """Config #3 proper: the FULL 6-class one-vs-one
    RBF-SVC fit — all 15 pairs to tolerance/cap — on 1M flow rows, row-
    sharded across ranks (strong scaling), with held-out accuracy and
    support counts reported untimed."""
    from traffic_classifier_sdn_amd.models import SVC

    n_total = args.svc_rows
    lo, hi = dist.shard_range(n_total, rank, world)
    Xn, lab, classes = _stratified_synth_rows(hi - lo, args.seed + 997 * rank)
    yn = classes[lab]
    max_iter = args.svc_full_max_iter if use_gpu else min(args.svc_full_max_iter, 300)
    fitted = []

    def step():
        m = SVC(tol=1e-3, max_iter=max_iter, device=device)
        m.fit(Xn, yn, sharded=world > 1)
        fitted.append(m)

    elapsed = _timed(step, args.steps, args.warmup, use_gpu)
    m = fitted[-1]
    _dump_outputs(args, rank, {
        "svc_full_n_iter": np.asarray(m.n_iter_),
        "svc_full_n_support": m.n_support_,
    })
    # held-out evaluation (untimed), fresh class-conditional rows
    Xe, lab_e, _ = _stratified_synth_rows(50_000 if use_gpu else 2_000, args.seed + 31337)
    pred = m.predict(Xe)
    acc = float((np.asarray(pred).astype(str) == classes[lab_e].astype(str)).mean())
    _emit(
        rank,
        "rows-fit/sec, full 6-class OVO RBF-SVC fit (15 pairs, SMO to tol) on 1M synthetic flow rows",
        n_total * args.steps / elapsed,
        "rows-fit/s",
        world,
        args,
        elapsed / args.steps * 1000.0,
        "strong",
        {
            "model": "RBF-SVC-OVO-15pairs-6class",
            "global_batch": n_total,
            "seq_len": 12,
            "parallelism": f"dp{world}",
            "fit_seconds_per_full_fit": elapsed / args.steps,
            "smo_max_iter_per_pair": max_iter,
            "smo_iters_per_pair": [int(v) for v in m.n_iter_],
            "pairs_converged": int(sum(1 for v in m.n_iter_ if v < max_iter)),
            "n_support_total": int(m.n_support_.sum()),
            "accuracy_heldout_6class_synth": acc,
            "tol": 1e-3,
        },
    )


def bench_rf_fit(args, rank, world, device, use_gpu):
    """RF tree build (the BASELINE metric's "tree build" op): one step =
    fit a full forest on the resident row shard with the level-synchronous
    histogram builder (HIP rf_hist kernel); trees split across ranks."""
    from traffic_classifier_sdn_amd.models import RandomForestClassifier

    X_real, _ = load_reference_dataset()
    n = args.rf_fit_rows
    Xn = synthetic_flow_rows(n, seed=args.seed + 77 + rank, reference_X=X_real)
    # patterned labels: realistic tree depth/compressibility
    med = np.median(Xn[:, [1, 4, 7]], axis=0)
    y = ((Xn[:, 1] > med[0]).astype(int) * 3 + (Xn[:, 4] > med[1]).astype(int)
         + (Xn[:, 7] > med[2]).astype(int)) % 6
    trees = args.rf_fit_trees

    def step():
        return RandomForestClassifier(
            n_estimators=trees, seed=args.seed,
            builder="hist" if use_gpu else "exact", device=device,
        ).fit(Xn, y)

    elapsed = _timed(step, args.steps, args.warmup, use_gpu)
    if args.dump_outputs:
        # the fitted forest, seen through its votes on the training rows
        _dump_outputs(args, rank, {"rf_fit_predict_index": _LAST_OUTPUT[0].predict_index(Xn)})
    total = float(n) * trees * args.steps  # trees are split across ranks
    _emit(
        rank,
        "row-trees/sec, RandomForest level-synchronous histogram build (HIP rf_hist)",
        total / elapsed,
        "row-trees/s",
        world,
        args,
        elapsed / args.steps * 1000.0,
        "strong",
        {
            "model": f"RandomForest-{trees}trees-hist256",
            "global_batch": n,
            "seq_len": 12,
            "parallelism": f"tree-par{world}",
            "rows": n,
            "trees": trees,
        },
    )


def bench_serve(args, rank, world, device, use_gpu):
    """Config #5: hipGraph-captured poll cycle over 8192 live flows."""
    from traffic_classifier_sdn_amd.flow.parser import replay
    from traffic_classifier_sdn_amd.flow.replay import SynthFlowSpec, TelemetryReplaySource
    from traffic_classifier_sdn_amd.serve_gpu import GpuServeEngine

    n_flows = args.serve_flows
    rng = np.random.default_rng(args.seed)
    specs = [
        SynthFlowSpec(
            "02:%02x:%02x:%02x:%02x:%02x" % tuple(int(v) for v in rng.integers(0, 256, 5)),
            "06:%02x:%02x:%02x:%02x:%02x" % tuple(int(v) for v in rng.integers(0, 256, 5)),
            float(rng.uniform(1, 60)),
            float(rng.uniform(60, 1200)),
            float(rng.uniform(1, 60)),
            float(rng.uniform(60, 1200)),
        )
        for _ in range(n_flows)
    ]
    src = TelemetryReplaySource(specs=specs, seed=args.seed)
    try:
        # line-rate C++ flow table + bulk TSV parser (same read-out surface)
        from traffic_classifier_sdn_amd.flow.native import NativePollParser

        parser = NativePollParser()
        parser.feed_buffer("\n".join(src.stream(2)) + "\n")
        table = parser.table
    except (ImportError, RuntimeError):
        table = replay(src.stream(2))
    names = ["RandomForestClassifier", "GaussianNB", "LogisticRegression", "SVC", "KMeans_Clustering"]
    models = {
        n: load_model(os.path.join(REPO, "data", "ref_models", n + ".npz"), device=device)
        for n in names
    }
    eng = GpuServeEngine(models, capacity=n_flows, use_graph=use_gpu, device=device)

    lat = []

    def step():
        out = eng.classify(table)
        lat.append(eng.last_latency_s)
        return out

    elapsed = _timed(step, args.steps, args.warmup, use_gpu)
    lat_t = np.asarray(lat[args.warmup :])
    _dump_outputs(args, rank, {"serve_" + k: v for k, v in _LAST_OUTPUT[0].items()})
    _emit(
        rank,
        "flows/sec through full poll cycle (snapshot->hipGraph ensemble predict->labels), 5-model ensemble",
        n_flows * args.steps * world / elapsed,
        "flows/s",
        world,
        args,
        elapsed / args.steps * 1000.0,
        "weak",
        {
            "model": "ensemble-5(RF+GNB+LR+SVC+KMeans)",
            "global_batch": n_flows,
            "seq_len": 12,
            "parallelism": f"dp{world}",
            "poll_latency_ms_p50": float(np.percentile(lat_t, 50) * 1e3),
            "poll_latency_ms_p99": float(np.percentile(lat_t, 99) * 1e3),
            "hipgraph": use_gpu,
        },
    )


WORKLOADS = {
    "rf": bench_rf,
    "knn": bench_knn,
    "svc-fit": bench_svc_fit,
    "svc-fit-full": bench_svc_fit_full,
    "serve": bench_serve,
    "rf-fit": bench_rf_fit,
}


def _maybe_self_spawn(args) -> Optional[int]:
    """Launch N ranks when invoked as ``python bench.py --gpus N`` directly.

    The driver may call bench.py either through torch.distributed.run (which
    sets WORLD_SIZE for every rank) or bare; bare with --gpus > 1 must still
    run N real ranks (--gpus was previously ignored and a
    bare multi-GPU invocation silently measured 1 rank).  Re-exec through
    torchrun on a free loopback port; rank 0's JSON line passes through on
    stdout unchanged.
    """
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return None
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [
        sys.executable, "-m", "torch.distributed.run",
        "--nnodes=1", f"--nproc-per-node={args.gpus}",
        "--master-addr=127.0.0.1", f"--master-port={port}",
        os.path.abspath(__file__), *sys.argv[1:],
    ]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="rf")
    ap.add_argument("--rows-per-gpu", type=int, default=10_000_000)
    ap.add_argument("--knn-ref-rows-per-gpu", type=int, default=12_500_000)
    ap.add_argument("--knn-queries", type=int, default=65_536)
    ap.add_argument("--knn-approx", action="store_true",
                    help="bf16 coarse-pass KNN selection (exact-f32 refine; "
                         "measured recall, opt-in — default is exact)")
    ap.add_argument("--svc-rows", type=int, default=1_000_000)
    ap.add_argument("--svc-iters-per-step", type=int, default=200)
    ap.add_argument("--svc-full-max-iter", type=int, default=20_000)
    ap.add_argument("--serve-flows", type=int, default=8192)
    ap.add_argument("--rf-fit-rows", type=int, default=1_000_000)
    ap.add_argument("--rf-fit-trees", type=int, default=25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--full", action="store_true",
                    help="also run the workload's untimed extras (RF flagship: "
                         "5-class accuracy + 6-class refit accuracy) and report "
                         "them in the result line; a plain run skips them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy "
                         "(float32/float64, at most 64 MB in all)")
    args = ap.parse_args()

    spawned = _maybe_self_spawn(args)
    if spawned is not None:
        return spawned

    use_gpu = torch.cuda.is_available()
    rank, world = dist.init_from_env("nccl" if use_gpu else "gloo")
    if use_gpu:
        torch.cuda.set_device(dist.env_local_rank())
        device = f"cuda:{dist.env_local_rank()}"
    else:
        device = "cpu"
        args.rows_per_gpu = min(args.rows_per_gpu, 20_000)
        args.knn_ref_rows_per_gpu = min(args.knn_ref_rows_per_gpu, 20_000)
        args.svc_rows = min(args.svc_rows, 20_000)
        args.serve_flows = min(args.serve_flows, 512)
        args.rf_fit_rows = min(args.rf_fit_rows, 20_000)
        args.rf_fit_trees = min(args.rf_fit_trees, 5)

    WORKLOADS[args.workload](args, rank, world, device, use_gpu)

    if dist.is_initialized():
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
