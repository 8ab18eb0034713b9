"""Real-time classification engine (the reference's serve path, rebuilt).

Pipeline per poll cycle (reference: traffic_classifier.py:144-171):
telemetry line -> flow-table update; every N accepted records (N=10, the
reference's PrettyTable cadence) -> batched feature matrix -> ONE device
predict over all live flows -> rendered table.

Differences from the reference, by design: prediction is
one batched kernel launch over every live flow instead of a Python loop of
batch-1 ``model.predict`` calls; on GPU the launch sequence is hipGraph-
captured (ops.gpu) to amortise launch overhead at high poll rates.
"""

from __future__ import annotations

import json
import sys
import time
from typing import Iterable, Optional, TextIO

import numpy as np

from .flow.parser import PollStreamParser
from .flow.state import FlowTable
from .models.base import Estimator
from .utils.schema import CLASS_NAMES, CSV_HEADER, FEATURE_SHORT_NAMES
from .utils.table import Table


def why_cells(why, why_value) -> list:
    """One cell per flow for the "Why" column: the short name of the feature
    that adds most to the probability of the class shown and what it adds,
    "Rev avg B/s +0.21"; blank where no feature speaks for it (why < 0)."""
    return [
        "%s %+.2f" % (FEATURE_SHORT_NAMES[f], v) if f >= 0 else ""
        for f, v in zip(why, why_value)
    ]


def render_flow_table(table: FlowTable, labels, confidence=None, why=None) -> str:
    """The reference's console table (traffic_classifier.py:100-118); with
    ``confidence`` (one value per flow) a further column shows it, and with
    ``why`` (one cell per flow, see why_cells) a last column "Why"."""
    cols = ["Flow ID", "Src MAC", "Dest MAC", "Traffic Type", "Forward Status", "Reverse Status"]
    if confidence is not None:
        cols.append("Confidence")
    if why is not None:
        cols.append("Why")
    t = Table(cols)
    metas = table.metas()
    statuses = table.statuses()
    for i, (meta, (fs, rs)) in enumerate(zip(metas, statuses)):
        row = [i, meta.ethsrc, meta.ethdst, labels[i], fs, rs]
        if confidence is not None:
            row.append("%.2f" % confidence[i])
        if why is not None:
            row.append(why[i])
        t.add_row(row)
    return str(t)


# (heading, key in a --stats line, column of the totals) of the summary's rates:
# the four instantaneous-rate features
_SUMMARY_RATES = (
    ("Fwd pkt/s", "fwd_pps", "Forward Instantaneous Packets per Second"),
    ("Fwd B/s", "fwd_Bps", "Forward Instantaneous Bytes per Second"),
    ("Rev pkt/s", "rev_pps", "DeltaReverse Instantaneous Packets per Second"),
    ("Rev B/s", "rev_Bps", "Reverse Instantaneous Bytes per Second"),
)


def traffic_rates(classes, totals) -> dict:
    """{class: {flows, fwd_pps, fwd_Bps, rev_pps, rev_Bps}} out of the totals
    of ops.class_traffic (rows: ``classes``, the last one "unknown")."""
    from .ops.cpu import TRAFFIC_COLUMNS

    cols = [(key, TRAFFIC_COLUMNS.index(name)) for _, key, name in _SUMMARY_RATES]
    out = {}
    for g, name in enumerate(classes):
        row = {"flows": int(totals[g, 0])}
        row.update({key: float(totals[g, c]) for key, c in cols})
        out[name] = row
    return out


def render_traffic_summary(classes, totals) -> str:
    """The per-class table below the flow table: one row per class and
    "unknown", also where a class has no flows."""
    rates = traffic_rates(classes, totals)
    total_bytes = sum(r["fwd_Bps"] + r["rev_Bps"] for r in rates.values())
    t = Table(["Traffic Type", "Flows"] + [h for h, _, _ in _SUMMARY_RATES] + ["Bytes share"])
    for name, r in rates.items():
        share = (r["fwd_Bps"] + r["rev_Bps"]) / total_bytes if total_bytes != 0 else 0.0
        t.add_row(
            [name, r["flows"]]
            + ["%.1f" % r[key] for _, key, _ in _SUMMARY_RATES]
            + ["%.1f%%" % (100.0 * share)]
        )
    return str(t)


def top_flow_lists(classes, rows, rates) -> dict:
    """{class: [[flow_id, Bps], ...]} out of ops.class_top_flows' results,
    largest first, the padding left out."""
    return {
        name: [[int(r), float(v)] for r, v in zip(rows[g], rates[g]) if r >= 0]
        for g, name in enumerate(classes)
    }


def render_top_flows(table: FlowTable, classes, rows, rates, totals) -> str:
    """The table below the summary: one line per listed flow, largest first
    within its class; a class with no flows has no line.  The share is the
    flow's rate over its class's forward plus reverse bytes per second."""
    class_bytes = {
        name: r["fwd_Bps"] + r["rev_Bps"] for name, r in traffic_rates(classes, totals).items()
    }
    t = Table(["Traffic Type", "Flow ID", "Src MAC", "Dest MAC", "B/s", "Share of class"])
    metas = table.metas()
    for name, flows in top_flow_lists(classes, rows, rates).items():
        for flow_id, rate in flows:
            share = rate / class_bytes[name] if class_bytes[name] != 0 else 0.0
            t.add_row([name, flow_id, metas[flow_id].ethsrc, metas[flow_id].ethdst,
                       "%.1f" % rate, "%.1f%%" % (100.0 * share)])
    return str(t)


def map_cluster_labels(idx: np.ndarray) -> np.ndarray:
    """Integer cluster ids -> class names (reference label map,
    traffic_classifier.py:109-114)."""
    names = np.asarray(CLASS_NAMES, dtype=object)
    idx = np.asarray(idx).ravel().astype(np.int64)
    out = np.empty(idx.shape, dtype=object)
    in_range = (idx >= 0) & (idx < len(names))
    out[in_range] = names[idx[in_range]]
    out[~in_range] = "unknown"
    return out


class RealtimeClassifier:
    """Streaming classify loop over any line source."""

    def __init__(
        self,
        model: Estimator,
        predict_every: int = 10,
        out: TextIO = sys.stdout,
        stats: bool = False,
        stats_out: TextIO = sys.stderr,
        prometheus_port: int = 0,
        confidence: bool = False,
        min_confidence: float = 0.0,
        smooth: Optional[float] = None,
        switch_margin: float = 0.0,
        summary: bool = False,
        prometheus_registry=None,
        novelty: Optional[Estimator] = None,
        novelty_threshold: Optional[float] = None,
        top: Optional[int] = None,
        explain: bool = False,
    ) -> None:
        if getattr(model, "kind", "") == "isolation_forest":
            raise ValueError(
                "an IsolationForest is a novelty detector with no classes to predict: "
                "pass it as novelty=, next to a classifier"
            )
        self.model = model
        # explain=True: per flow, the feature that adds most to the forest's
        # probability of the class SHOWN (smoothed if smoothing is on; a flow
        # shown as "unknown" gets none) and what it adds (ops.rf_explain on
        # the model's device), as a "Why" column and in the --stats line
        self.explain = bool(explain)
        self.last_why: Optional[np.ndarray] = None  # int32[n] feature index, -1: none
        self.last_why_value: Optional[np.ndarray] = None  # float32[n]
        if self.explain:
            if getattr(model, "kind", "") != "random_forest" or not hasattr(model, "explain_device"):
                raise ValueError(
                    f"{type(model).__name__} is not a random forest: only a forest's verdicts "
                    "are explained"
                )
            self._explain_index = {str(c): i for i, c in enumerate(model.classes_)}
        # novelty=IsolationForest: a flow whose novelty score is above the
        # threshold (the detector's own by default) is shown as "unknown",
        # after the confidence rule
        self.novelty = None
        self.last_novel: Optional[np.ndarray] = None  # bool[n] of the last pass
        self.last_novelty_score: Optional[np.ndarray] = None  # float32[n]
        if novelty is not None:
            from .ops.cpu import iforest_depth_cut

            if getattr(novelty, "kind", "") != "isolation_forest":
                raise ValueError(
                    f"novelty= takes an IsolationForest, got {type(novelty).__name__}"
                )
            if novelty.trees_ is None or novelty.threshold_ is None:
                raise ValueError("novelty= takes a fitted IsolationForest")
            thr = novelty.threshold_ if novelty_threshold is None else novelty_threshold
            iforest_depth_cut(thr, 1, 1.0)  # ValueError unless inside (0, 1)
            self.novelty = novelty
            self.novelty_threshold = float(thr)
        elif novelty_threshold is not None:
            raise ValueError("novelty_threshold needs novelty=")
        # summary=True: flows, packets/s and bytes/s per class after each
        # pass (ops.class_traffic on the model's device), as a second table,
        # in the --stats line and in the Prometheus gauges
        self.summary = bool(summary)
        self.traffic: Optional[np.ndarray] = None  # f64 [C + 1, 13] of the last pass
        self.traffic_classes: Optional[list] = None
        if self.summary:
            names = getattr(model, "classes_", None)
            if names is None:
                names = getattr(model, "cluster_label_names_", None)
            if names is None:
                names = CLASS_NAMES
            # a cluster map may give two clusters one name
            names = [n for n in dict.fromkeys(str(n) for n in names) if n != "unknown"]
            if not 2 <= len(names) <= 8:
                raise ValueError(
                    f"summary accounts 2..8 classes, {type(model).__name__} has {len(names)}"
                )
            self.traffic_classes = names + ["unknown"]
            self._class_index = {n: i for i, n in enumerate(names)}
            self._last_X = np.zeros((0, 12), dtype=np.float32)
        # top=K (with summary): the K flows of every class with the most
        # bytes per second (ops.class_top_flows on the same features and
        # labels), as a third table and in the --stats line.  No Prometheus
        # series: a label per flow has no bound.
        self.top = None
        self.top_flows: Optional[np.ndarray] = None  # int32 [C + 1, K] flow ids, -1: none
        self.top_flow_rates: Optional[np.ndarray] = None  # f32 [C + 1, K]
        if top is not None:
            from .ops.cpu import top_flows_k_check

            if not self.summary:
                raise ValueError("top= lists the flows behind the summary: it needs summary=True")
            self.top = top_flows_k_check(top)
        # smooth=alpha: labels and confidence come from the flow's class
        # probabilities averaged across passes (models/smoothing.py)
        self.smoother = None
        if smooth is not None:
            from .models.smoothing import FlowSmoother

            if not hasattr(model, "predict_proba") or getattr(model, "classes_", None) is None:
                raise ValueError(
                    f"{type(model).__name__} has no class probabilities to smooth"
                )
            self.smoother = FlowSmoother(
                len(model.classes_), 64, smooth, switch_margin,
                device=getattr(model, "device", "cpu"),
            )
        # per-flow confidence column; a flow below min_confidence (which
        # implies the column) is shown as "unknown"
        self.min_confidence = float(min_confidence)
        self.confidence = bool(confidence) or self.min_confidence > 0.0
        self.last_confidence = None  # float32[n] of the last pass
        self.parser = PollStreamParser()
        self.predict_every = predict_every
        self.out = out
        self.stats = stats
        self.stats_out = stats_out
        self._last_batch = 0
        self.prom = None
        if prometheus_port:
            from .utils.prom import PromServeMetrics

            self.prom = PromServeMetrics(
                prometheus_port, registry=prometheus_registry, summary=self.summary
            )

    def classify_now(self) -> np.ndarray:
        pred = self._classify_now()
        if self.novelty is not None:
            n = len(self.parser.table)
            if n == 0:
                self.last_novel = np.zeros(0, dtype=bool)
                self.last_novelty_score = np.zeros(0, dtype=np.float32)
            else:
                X = self.parser.table.feature_matrix(dtype=np.float32)
                score, flags, _ = self.novelty.novelty_device(X, None, self.novelty_threshold)
                self.last_novelty_score = score.cpu().numpy()
                self.last_novel = flags.cpu().numpy().astype(bool)
                pred = np.asarray(pred, dtype=object)
                pred[self.last_novel] = "unknown"
        if self.explain:
            self._explain_now(pred)
        return pred

    def _explain_now(self, pred) -> None:
        """Why of the classes shown: a name that is no class of the forest
        ("unknown") is label -1, which the op answers with no feature."""
        n = len(self.parser.table)
        if n == 0:
            self.last_why = np.zeros(0, dtype=np.int32)
            self.last_why_value = np.zeros(0, dtype=np.float32)
            return
        shown = np.fromiter(
            (self._explain_index.get(str(name), -1) for name in pred), dtype=np.int32, count=n
        )
        X = self.parser.table.feature_matrix(dtype=np.float32)
        _, why, why_value, _ = self.model.explain_device(X, shown, want_matrix=False)
        self.last_why = why.cpu().numpy()
        self.last_why_value = why_value.cpu().numpy()

    def _classify_now(self) -> np.ndarray:
        table = self.parser.table
        if len(table) == 0:
            if self.confidence:
                self.last_confidence = np.zeros(0, dtype=np.float32)
            if self.summary:
                self._last_X = np.zeros((0, 12), dtype=np.float32)
            return np.asarray([], dtype=object)
        X = table.feature_matrix(dtype=np.float32)
        if self.summary:
            self._last_X = X
        if self.smoother is not None:
            return self._classify_smoothed(X)
        if self.confidence:
            pred, conf = self.model.predict_with_confidence(X)
            self.last_confidence = conf
            pred = np.asarray(pred, dtype=object)
            pred[conf < self.min_confidence] = "unknown"
            return pred
        pred = self.model.predict(X)
        if self.model.classes_ is None:  # unsupervised: cluster ids -> names
            names = getattr(self.model, "cluster_label_names_", None)
            if names is not None:
                # mode-based map learned at fit time (fit.py); the reference's
                # fixed index->name map silently mislabels
                idx = np.asarray(pred).ravel().astype(np.int64)
                pred = np.asarray(names, dtype=object)[idx]
            else:
                pred = map_cluster_labels(pred)
        return pred

    def _classify_smoothed(self, X: np.ndarray) -> np.ndarray:
        """Row i of the table is flow slot i of the smoother, for life."""
        import torch

        sm = self.smoother
        proba_fn = getattr(self.model, "predict_proba_device", None) or self.model.predict_proba
        proba = torch.as_tensor(proba_fn(X)).to(device=sm.device, dtype=torch.float32).contiguous()
        sm.ensure_capacity(proba.shape[0])
        idx, conf = sm.update(proba)
        pred = np.asarray(self.model.classes_, dtype=object)[idx.cpu().numpy()]
        conf = conf.cpu().numpy()
        if self.confidence:
            self.last_confidence = conf
            pred[conf < self.min_confidence] = "unknown"
        return pred

    def account(self, labels) -> np.ndarray:
        """Totals [C + 1, 13] of the pass that gave ``labels`` (names, with
        "unknown" already applied): summed on the model's device."""
        import torch

        from . import ops

        C = len(self.traffic_classes) - 1
        device = torch.device(str(getattr(self.model, "device", "cpu")))
        idx = np.fromiter(
            (self._class_index.get(str(name), C) for name in labels),
            dtype=np.int32, count=len(labels),
        )
        X = torch.from_numpy(np.ascontiguousarray(self._last_X)).to(device)
        idx = torch.from_numpy(idx).to(device)
        totals = ops.class_traffic(X, idx, C)
        self.traffic = totals.cpu().numpy()
        if self.top is not None:
            rows, rates = ops.class_top_flows(X, idx, C, self.top)
            self.top_flows = rows.cpu().numpy()
            self.top_flow_rates = rates.cpu().numpy()
        return self.traffic

    def feed(self, line) -> bool:
        """Feed one telemetry line; returns True when a prediction pass ran.

        The cadence counts accepted data records, mirroring the reference's
        per-line counter (traffic_classifier.py:167-171: its `time % 10`
        ticks once per flow row, not per second).
        """
        before = self.parser.records
        self.parser.feed(line)
        if self.parser.records == before:
            return False
        if (self.parser.records - self._last_batch) >= self.predict_every:
            self._last_batch = self.parser.records
            t0 = time.perf_counter()
            labels = self.classify_now()
            predict_s = time.perf_counter() - t0
            conf = self.last_confidence if self.confidence else None
            if self.explain:
                flow_table = render_flow_table(
                    self.parser.table, labels, conf, why_cells(self.last_why, self.last_why_value))
            else:
                flow_table = render_flow_table(self.parser.table, labels, conf)
            self.out.write(flow_table + "\n")
            if self.summary:
                totals = self.account(labels)
                self.out.write(render_traffic_summary(self.traffic_classes, totals) + "\n")
                if self.top is not None:
                    self.out.write(render_top_flows(
                        self.parser.table, self.traffic_classes, self.top_flows,
                        self.top_flow_rates, totals) + "\n")
            self.out.flush()
            if self.prom is not None:
                self.prom.observe_pass(
                    len(self.parser.table), self.parser.records, predict_s, labels
                )
                if self.summary:
                    self.prom.observe_traffic(traffic_rates(self.traffic_classes, totals))
            if self.stats:
                n = len(self.parser.table)
                line = {
                    "flows": n,
                    "records": self.parser.records,
                    "predict_ms": predict_s * 1e3,
                    "flows_per_sec": n / predict_s if predict_s > 0 else None,
                    "device": str(getattr(self.model, "device", "cpu")),
                }
                if conf is not None:
                    line["mean_confidence"] = float(conf.mean()) if n else None
                    line["unknown"] = int((conf < self.min_confidence).sum())
                if self.novelty is not None:
                    line["novel"] = int(self.last_novel.sum())
                if self.explain:
                    feats, counts = np.unique(self.last_why[self.last_why >= 0], return_counts=True)
                    line["why"] = {
                        FEATURE_SHORT_NAMES[f]: int(c) for f, c in zip(feats, counts)
                    }
                if self.summary:
                    line["traffic"] = traffic_rates(self.traffic_classes, totals)
                if self.top is not None:
                    line["top_flows"] = top_flow_lists(
                        self.traffic_classes, self.top_flows, self.top_flow_rates)
                self.stats_out.write(json.dumps(line) + "\n")
                self.stats_out.flush()
            return True
        return False

    def run(self, lines: Iterable) -> None:
        for line in lines:
            self.feed(line)


class TrainingCollector:
    """Training-data collection loop (reference: traffic_classifier.py:209-223):
    writes the 17-column header then one TSV row per tracked flow per
    accepted telemetry record."""

    def __init__(self, traffic_type: str, f: TextIO) -> None:
        self.traffic_type = traffic_type
        self.f = f
        self.parser = PollStreamParser()
        self.f.write(CSV_HEADER)

    def feed(self, line) -> None:
        before = self.parser.records
        self.parser.feed(line)
        if self.parser.records != before:
            for row in self.parser.table.training_rows(self.traffic_type):
                self.f.write(row + "\n")

    def run(self, lines: Iterable) -> None:
        for line in lines:
            self.feed(line)
