"""CLI with the reference's exact subcommand surface
(reference: traffic_classifier.py:174-246), plus flags for the new engine.

    python -m traffic_classifier_sdn_amd train <TypeOfData> [--source ...]
    python -m traffic_classifier_sdn_amd <algo>              [--source ...]
    python -m traffic_classifier_sdn_amd ensemble [--members a,b,...] [--weights ...]

Subcommands: train, logistic, kmeans, knearest, svm, Randomforest,
gaussiannb (SUBCOMMANDS at traffic_classifier.py:189; the reference's
unreachable-`knearest` loader bug, SURVEY.md §2.1, is fixed: `knearest`
loads the KNeighbors checkpoint).  `ensemble` is new here: a soft vote over
the class probabilities of several checkpoints (models/ensemble.py).
`--smooth ALPHA [--switch-margin M]` averages each flow's class probabilities
across passes, for every model that has them (models/smoothing.py).
`--summary` adds a per-class table of flows, packets/s and bytes/s below
each flow table (ops.class_traffic).
`--novelty [--novelty-threshold S]` shows flows unlike the training data as
'unknown', whatever the classifier says of them (models/isolation_forest.py).
`Randomforest --explain` adds a "Why" column: the feature that adds most to
the forest's probability of the class shown, and how much (ops.rf_explain).

Telemetry sources:
  --source subprocess   spawn a monitor command (default: the in-package
                        OpenFlow-1.3 monitor) and scrape its stdout — the
                        reference's process model (traffic_classifier.py:228)
  --source stdin        read `data\t` TSV lines from stdin
  --source replay       built-in synthetic telemetry (no network needed)
"""

from __future__ import annotations

import argparse
import os
import signal
import subprocess
import sys
from typing import Iterable, Optional

SUBCOMMANDS = ("train", "logistic", "kmeans", "knearest", "svm", "Randomforest", "gaussiannb",
               "ensemble")
DEFAULT_MEMBERS = "Randomforest,gaussiannb,logistic,knearest"

DEFAULT_TIMEOUT = 15 * 60  # training-collection window (traffic_classifier.py:27)


def _monitor_cmd() -> str:
    # the in-package native OpenFlow 1.3 monitor (no Ryu dependency)
    return f"{sys.executable} -m traffic_classifier_sdn_amd.flow.monitor"


def _line_source(args) -> Iterable:
    if args.source == "stdin":
        return sys.stdin
    if args.source == "replay":
        from .flow.replay import TelemetryReplaySource

        return TelemetryReplaySource(seed=args.seed).stream(args.replay_polls)
    # subprocess: spawn monitor, scrape stdout (reference process model)
    cmd = args.monitor_cmd or _monitor_cmd()
    p = subprocess.Popen(
        cmd, shell=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
        preexec_fn=os.setsid,
    )

    def gen():
        try:
            for line in p.stdout:
                yield line
        finally:
            try:
                os.killpg(os.getpgid(p.pid), signal.SIGTERM)
            except (ProcessLookupError, PermissionError):
                pass

    return gen()


def _checkpoint_path(algo: str, models_dir: str) -> str:
    """Resolve the checkpoint like the reference loader (models/<Name>),
    trying the engine .npz first, then the sklearn pickle, then the
    in-repo converted reference checkpoints (data/ref_models) so a fresh
    clone serves out of the box."""
    from .models import ALGO_TO_CHECKPOINT

    fname, _ = ALGO_TO_CHECKPOINT[algo]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in (models_dir, os.path.join(repo, "data", "ref_models")):
        for cand in (os.path.join(d, fname + ".npz"), os.path.join(d, fname)):
            if os.path.exists(cand):
                return cand
    return os.path.join(models_dir, fname)


def _load_ensemble(args):
    """The `ensemble` subcommand's model, or None after one line on stderr
    (unknown or missing member, member without probabilities, bad weights)."""
    from .models import ALGO_TO_CHECKPOINT, SoftVoteEnsemble, load_model

    names = [m.strip() for m in args.members.split(",") if m.strip()]
    try:
        weights = None
        if args.weights is not None:
            weights = [float(w) for w in args.weights.split(",")]
        members = {}
        for name in names:
            if name not in ALGO_TO_CHECKPOINT:
                raise ValueError(f"unknown ensemble member {name!r}")
            if name in members:
                raise ValueError(f"ensemble member {name!r} is named twice")
            path = _checkpoint_path(name, args.models_dir)
            if not os.path.exists(path):
                raise ValueError(f"checkpoint {path} not found")
            members[name] = load_model(path, device=args.device)
        return SoftVoteEnsemble(members, weights)
    except ValueError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return None


NOVELTY_CHECKPOINT = "IsolationForest.npz"


def _load_novelty(args):
    """The `--novelty` detector: <models-dir>/IsolationForest.npz, else the
    in-repo one (data/ref_models), else a fit at start-up on the six-class
    dataset, announced on stderr."""
    from .models import IsolationForest, load_model

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in (args.models_dir, os.path.join(repo, "data", "ref_models")):
        path = os.path.join(d, NOVELTY_CHECKPOINT)
        if os.path.exists(path):
            model = load_model(path, device=args.device)
            if not isinstance(model, IsolationForest):
                raise ValueError(f"{path} holds a {type(model).__name__}, not an IsolationForest")
            return model
    from .utils.datasets import load_six_class_dataset

    print(f"NOTE: no {NOVELTY_CHECKPOINT} found: fitting the novelty detector on the "
          "six-class dataset now", file=sys.stderr)
    X, _ = load_six_class_dataset()
    return IsolationForest(device=args.device).fit(X)


def main(argv: Optional[list] = None) -> int:
    parser = argparse.ArgumentParser(
        prog="traffic_classifier_sdn_amd",
        description=__doc__,
        formatter_class=argparse.RawDescriptionHelpFormatter,
    )
    parser.add_argument("subcommand", choices=SUBCOMMANDS)
    parser.add_argument("traffic_type", nargs="?", help="traffic class (train mode)")
    parser.add_argument("--source", choices=("subprocess", "stdin", "replay"), default="subprocess")
    parser.add_argument("--monitor-cmd", default=None, help="override monitor command")
    parser.add_argument("--models-dir", default="models", help="checkpoint directory")
    parser.add_argument("--device", default=None, help="cpu / cuda (default: auto)")
    parser.add_argument("--timeout", type=int, default=DEFAULT_TIMEOUT, help="train collection seconds")
    parser.add_argument("--replay-polls", type=int, default=30)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--prometheus", type=int, default=0, metavar="PORT",
                        help="expose serve metrics on a Prometheus scrape port")
    parser.add_argument("--stats", action="store_true",
                        help="emit one JSON perf line (flows, predict_ms, flows/sec) per prediction pass on stderr")
    parser.add_argument("--confidence", action="store_true",
                        help="append a Confidence column (top class probability) to the table")
    parser.add_argument("--min-confidence", type=float, default=0.0, metavar="P",
                        help="show flows whose confidence is below P as 'unknown' (implies --confidence)")
    parser.add_argument("--smooth", type=float, default=None, metavar="ALPHA",
                        help="average each flow's class probabilities across passes with this "
                             "weight in (0, 1] on the newest; labels and confidence come from the average")
    parser.add_argument("--switch-margin", type=float, default=0.0, metavar="M",
                        help="with --smooth: a flow changes its label only when another class "
                             "leads the average by more than M")
    parser.add_argument("--summary", action="store_true",
                        help="below each flow table, print flows, packets/s and bytes/s per "
                             "traffic class (summed on the model's device); adds them to --stats "
                             "and --prometheus")
    parser.add_argument("--top", type=int, default=None, metavar="K",
                        help="needs --summary: below the summary, list the K flows of every "
                             "traffic class with the most bytes/s (selected on the model's "
                             "device); adds them to --stats")
    parser.add_argument("--novelty", action="store_true",
                        help="show flows unlike the training data as 'unknown': an isolation "
                             "forest scores every flow on the model's device "
                             "(<models-dir>/IsolationForest.npz, else fitted at start-up)")
    parser.add_argument("--novelty-threshold", type=float, default=None, metavar="S",
                        help="with --novelty: a flow is novel when its score in (0, 1) is "
                             "above S (default: the detector's own threshold)")
    parser.add_argument("--explain", action="store_true",
                        help="Randomforest only: add a 'Why' column, the feature that adds most "
                             "to the forest's probability of the class shown and how much "
                             "(computed on the model's device); adds feature counts to --stats")
    parser.add_argument("--members", default=DEFAULT_MEMBERS, metavar="A,B,...",
                        help="ensemble: the subcommand names of the member models")
    parser.add_argument("--weights", default=None, metavar="W,W,...",
                        help="ensemble: one positive weight per member (default: equal)")
    args = parser.parse_args(argv)

    if args.subcommand == "train":
        if not args.traffic_type:
            print("ERROR: specify traffic type.\n", file=sys.stderr)
            return 2
        from .serve import TrainingCollector

        out_path = f"{args.traffic_type}_training_data.csv"
        lines = _line_source(args)
        with open(out_path, "w") as f:
            collector = TrainingCollector(args.traffic_type, f)

            if args.source == "subprocess":
                # the reference's 15-min SIGALRM window
                # (traffic_classifier.py:214-215)
                def _alarm(signum, frame):
                    raise KeyboardInterrupt

                signal.signal(signal.SIGALRM, _alarm)
                signal.alarm(args.timeout)
            try:
                collector.run(lines)
            except KeyboardInterrupt:
                print("Finished collecting data.")
        return 0

    # serve mode: load checkpoint, stream, classify
    from .models import load_model
    from .serve import RealtimeClassifier

    if args.subcommand == "ensemble":
        model = _load_ensemble(args)
        if model is None:
            return 2
    else:
        path = _checkpoint_path(args.subcommand, args.models_dir)
        if not os.path.exists(path):
            print(f"ERROR: checkpoint {path} not found", file=sys.stderr)
            return 2
        model = load_model(path, device=args.device)
    confidence = args.confidence or args.min_confidence > 0.0
    if confidence and not hasattr(model, "predict_proba"):
        print(f"ERROR: {args.subcommand} has no class probabilities: no --confidence",
              file=sys.stderr)
        return 2
    if args.smooth is not None and not hasattr(model, "predict_proba"):
        print(f"ERROR: {args.subcommand} has no class probabilities: no --smooth",
              file=sys.stderr)
        return 2
    if args.explain and getattr(model, "kind", "") != "random_forest":
        print(f"ERROR: {args.subcommand} is not a random forest: --explain explains a forest's "
              "verdicts only", file=sys.stderr)
        return 2
    # the streams as they are now, not as they were when serve was imported
    try:
        if args.novelty_threshold is not None and not args.novelty:
            raise ValueError("--novelty-threshold needs --novelty")
        novelty = _load_novelty(args) if args.novelty else None
        rc = RealtimeClassifier(model, out=sys.stdout, stats=args.stats, stats_out=sys.stderr,
                                prometheus_port=args.prometheus,
                                confidence=confidence, min_confidence=args.min_confidence,
                                smooth=args.smooth, switch_margin=args.switch_margin,
                                summary=args.summary, novelty=novelty,
                                novelty_threshold=args.novelty_threshold, top=args.top,
                                explain=args.explain)
    except ValueError as e:  # --smooth, --switch-margin or --novelty-threshold out of range,
        # --summary over 8 classes, a detector's checkpoint in a classifier's place,
        # --top without --summary or outside 1..64
        print(f"ERROR: {e}", file=sys.stderr)
        return 2
    try:
        rc.run(_line_source(args))
    except KeyboardInterrupt:
        pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
