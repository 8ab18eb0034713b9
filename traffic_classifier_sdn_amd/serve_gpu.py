"""GPU real-time serve engine (BASELINE.json config #5).

Per poll cycle: the host flow table tracks raw counters only; the GPU runs
feature extraction (flow_features kernel: the reference's rate math,
traffic_classifier.py:63-96) fused back-to-back with the ensemble's predict
kernels, all captured once in a hipGraph (torch.cuda.CUDAGraph == hipGraph
on ROCm) and replayed per poll — one graph launch instead of K kernel
launches, sized for a 1 ms poll cadence.

Buffers are fixed-capacity (graphs need static shapes); flows beyond
capacity fall back to a plain (non-graph) launch path.

``ensemble=[names]`` adds a soft vote over those models' class probabilities
(models/ensemble.py): the result gains the key ``"ensemble"`` (indices into
``engine.ensemble.classes_``) and ``engine.confidence`` its averaged top
probability.  The members' probability kernels and the vote kernel are part
of the same captured graph.

``smooth=alpha`` (with ``ensemble=``) carries each flow's averaged
probability row from poll to poll (models/smoothing.py): the result gains
the key ``"smoothed"``, a label that changes only when another class leads
the moving average by more than ``switch_margin``, and ``engine.confidence``
the smoothed probability of that label.  ``"ensemble"`` stays the raw vote.
The smoothing kernel is part of the captured graph too; the live-row count
reaches it through device memory, so that the rows past it, which the graph
also runs over, are reset and not averaged.

``traffic=key`` accounts the pass per class of that key's labels (a
supervised model's name, ``"ensemble"`` or ``"smoothed"``): after
``classify``, ``engine.traffic`` holds the f64 [C + 1, 13] totals of
ops.class_traffic, flow count and the 12 feature sums per class and for
``"unknown"`` (``engine.traffic_classes``).  With ``traffic_min_confidence``
a flow whose confidence is below it counts as unknown.  The reduction runs
in the captured graph on the features that exist only on the device; one
table of under 1 KB comes back instead of them.

``novelty=model`` (an IsolationForest) scores every flow for how unlike the
training rows it is (csrc/iforest_kernels.hip), in the same captured pass on
the same features: after ``classify``, ``engine.novelty_score`` holds the
f32 [n] scores and ``engine.novel`` the bool [n] flags (score above
``novelty_threshold``, by default the model's own).  The result dict does not
change.  With ``traffic=`` the flagged flows count as unknown: the score
kernel hands the accounting that key's labels with -1 in the flagged rows.

``top_flows=K`` (with ``traffic=``) lists, per class and for "unknown", the K
flows with the largest rate (csrc/top_flows_kernels.hip): after ``classify``,
``engine.top_flows`` holds the int32 [C + 1, K] flow-table slots (rows:
``traffic_classes``; -1 where a class has fewer) and ``engine.top_flow_rates``
the f32 [C + 1, K] rates, the sum of the feature columns
``top_flows_columns`` (default ops.TOP_FLOW_COLUMNS, forward plus reverse
bytes per second).  It ranks what the accounting counts, the same labels,
confidence rule and live rows, right after it in the same captured pass.

``explain=name`` (a random forest among the models) says why that forest
gave each flow its class (csrc/rf_explain_kernels.hip), in the same captured
pass on the same features and on the forest's own labels of the pass, not
masked by novelty: after ``classify``, ``engine.why`` holds the int32 [n]
index into ``engine.explain_features`` of the feature that adds most to the
class's probability (-1: none adds anything) and ``engine.why_value`` the
f32 [n] amount it adds.  ``explain_matrix=True`` also leaves
``engine.contributions``, f32 [n, 12]: with ``engine.explain_bias`` (f64 [C])
of the flow's class they add up to the forest's probability of that class.
The result dict does not change.
"""

from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .flow.state import FlowTable
from .models.base import Estimator


class GpuServeEngine:
    # set per instance only with traffic=, so that an engine without it is
    # what it was: after classify(), f64 [C + 1, 13] totals of the pass (rows:
    # traffic_classes, columns: ops.TRAFFIC_COLUMNS)
    traffic: Optional[np.ndarray] = None
    traffic_classes: Optional[List[str]] = None
    _traffic_key: Optional[str] = None
    # likewise set per instance only with novelty=: after classify(), the
    # f32 [n] novelty scores and the bool [n] flags of the pass
    novelty_score: Optional[np.ndarray] = None
    novel: Optional[np.ndarray] = None
    _novelty = None
    # likewise set per instance only with top_flows=: after classify(), the
    # int32 [C + 1, K] slots and the f32 [C + 1, K] rates of the pass
    top_flows: Optional[np.ndarray] = None
    top_flow_rates: Optional[np.ndarray] = None
    _top_k: Optional[int] = None
    # likewise set per instance only with explain=: after classify(), the
    # int32 [n] feature index and the f32 [n] contribution of the pass, and
    # with explain_matrix=True the f32 [n, 12] contributions
    why: Optional[np.ndarray] = None
    why_value: Optional[np.ndarray] = None
    contributions: Optional[np.ndarray] = None
    explain_bias: Optional[np.ndarray] = None
    explain_features: Optional[tuple] = None
    _explain: Optional[str] = None

    def __init__(
        self,
        models: Dict[str, Estimator],
        capacity: int = 8192,
        use_graph: bool = True,
        device: str = "cuda",
        confidence: bool = False,
        ensemble: Optional[Sequence[str]] = None,
        ensemble_weights: Optional[Sequence[float]] = None,
        smooth: Optional[float] = None,
        switch_margin: float = 0.0,
        traffic: Optional[str] = None,
        traffic_min_confidence: float = 0.0,
        novelty: Optional[Estimator] = None,
        novelty_threshold: Optional[float] = None,
        top_flows: Optional[int] = None,
        top_flows_columns: Optional[Sequence[int]] = None,
        explain: Optional[str] = None,
        explain_matrix: bool = False,
    ) -> None:
        for name, m in models.items():
            if getattr(m, "kind", "") == "isolation_forest":
                raise ValueError(
                    f"model {name!r} is an IsolationForest, a novelty detector with no classes "
                    "to predict: pass it as novelty=, not among the models"
                )
        self.models = models
        self.capacity = capacity
        self.device = torch.device(device)
        self.use_graph = use_graph and self.device.type == "cuda"
        # pinned staging + device buffers (static for graph capture)
        pin = self.device.type == "cuda"
        self.h_cur = torch.zeros(capacity, 4, dtype=torch.float64, pin_memory=pin)
        self.h_prev = torch.zeros(capacity, 4, dtype=torch.float64, pin_memory=pin)
        self.h_times = torch.zeros(capacity, 6, dtype=torch.float64, pin_memory=pin)
        self.d_cur = torch.zeros(capacity, 4, dtype=torch.float64, device=self.device)
        self.d_prev = torch.zeros(capacity, 4, dtype=torch.float64, device=self.device)
        self.d_times = torch.zeros(capacity, 6, dtype=torch.float64, device=self.device)
        self.d_labels: Dict[str, torch.Tensor] = {}
        self.h_labels: Dict[str, torch.Tensor] = {}
        # per-flow confidence (top class probability) of the models that have
        # predict_index_conf; their labels then come from that same call
        self._conf_models = (
            [n for n, m in models.items() if hasattr(m, "predict_index_conf")]
            if confidence else []
        )
        self.d_conf: Dict[str, torch.Tensor] = {}
        self.h_conf: Dict[str, torch.Tensor] = {}
        # soft vote over the named models; None leaves the pass as it is
        self.ensemble = None
        self._ens_members: List[str] = []
        if ensemble:
            from .models.ensemble import SoftVoteEnsemble
            from .models.kneighbors import KNeighborsClassifier

            names = list(ensemble)
            if "ensemble" in models:
                raise ValueError("with ensemble=, no model can be named 'ensemble'")
            if len(set(names)) != len(names):
                raise ValueError(f"ensemble names a model twice: {names}")
            missing = [n for n in names if n not in models]
            if missing:
                raise ValueError(f"ensemble members {missing} are not in models")
            if self.use_graph:
                knn = [n for n in names if isinstance(models[n], KNeighborsClassifier)]
                if knn:
                    raise ValueError(
                        f"ensemble member {knn[0]!r} is a KNN model, which this engine "
                        "does not capture: use use_graph=False"
                    )
            self.ensemble = SoftVoteEnsemble({n: models[n] for n in names}, ensemble_weights)
            self._ens_members = names
        # per-flow smoothing of the vote's averaged row across polls
        self.smoother = None
        if smooth is not None:
            from .models.smoothing import FlowSmoother

            if self.ensemble is None:
                raise ValueError("smooth= smooths the vote's probabilities: it needs ensemble=")
            if "smoothed" in models:
                raise ValueError("with smooth=, no model can be named 'smoothed'")
            self.smoother = FlowSmoother(
                len(self.ensemble.classes_), capacity, smooth, switch_margin, device=self.device
            )
            self._smooth_table: Optional[FlowTable] = None
            self._smooth_n = 0
        # the keys the vote adds to the result, and every key of
        # self.confidence, in order
        self._vote_keys = (["ensemble"] if self.ensemble else []) + (
            ["smoothed"] if self.smoother else []
        )
        self._conf_keys = self._conf_models + self._vote_keys
        # per-class accounting of one key's labels (ops.class_traffic)
        if traffic is not None:
            if traffic in self._vote_keys:
                classes = self.ensemble.classes_
            elif traffic in models:
                classes = getattr(models[traffic], "classes_", None)
                if classes is None:
                    raise ValueError(
                        f"traffic={traffic!r}: {type(models[traffic]).__name__} has no classes "
                        "to account by"
                    )
            elif traffic in ("ensemble", "smoothed"):
                raise ValueError(
                    f"traffic={traffic!r} needs "
                    + ("ensemble=" if traffic == "ensemble" else "smooth=")
                )
            else:
                raise ValueError(f"traffic={traffic!r} is not a key of the result")
            if not 2 <= len(classes) <= 8:
                raise ValueError(f"traffic= accounts 2..8 classes, {traffic!r} has {len(classes)}")
            mc = float(traffic_min_confidence)
            if not np.isfinite(mc) or mc < 0.0:
                raise ValueError(f"traffic_min_confidence must be finite and >= 0, got {mc}")
            if mc > 0.0 and traffic not in self._conf_keys:
                raise ValueError(
                    f"traffic_min_confidence needs a confidence, and {traffic!r} has none "
                    "(confidence=True and a model with predict_index_conf, the vote or the "
                    "smoothed verdict)"
                )
            self._traffic_key = traffic
            self._traffic_min_conf = mc
            self.traffic_classes = [str(c) for c in classes] + ["unknown"]
            self._d_traffic: Optional[torch.Tensor] = None
            self._h_traffic: Optional[torch.Tensor] = None
        # the K largest flows of every class of that accounting
        if top_flows is not None:
            from .ops.cpu import TOP_FLOW_COLUMNS, top_flow_columns_check, top_flows_k_check

            if traffic is None:
                raise ValueError("top_flows= ranks the flows that traffic= accounts: it needs traffic=")
            self._top_k = top_flows_k_check(top_flows)
            self._top_columns = top_flow_columns_check(
                TOP_FLOW_COLUMNS if top_flows_columns is None else tuple(top_flows_columns)
            )
            self.d_top: Dict[str, torch.Tensor] = {}
            self.h_top: Dict[str, torch.Tensor] = {}
        elif top_flows_columns is not None:
            raise ValueError("top_flows_columns needs top_flows=")
        if self.smoother is not None or traffic is not None:
            # the live-row count, staged like the counters: the captured
            # pass runs over all `capacity` rows and reads it on the device
            self.h_nlive = torch.zeros(1, dtype=torch.int32, pin_memory=pin)
            self._h_nlive_np = self.h_nlive.numpy()  # same memory, cheap to set
            self.d_nlive = torch.zeros(1, dtype=torch.int32, device=self.device)
        if novelty is not None:
            from . import ops

            if getattr(novelty, "kind", "") != "isolation_forest":
                raise ValueError(
                    f"novelty= takes an IsolationForest, got {type(novelty).__name__}"
                )
            if novelty.trees_ is None or novelty.threshold_ is None:
                raise ValueError("novelty= takes a fitted IsolationForest")
            thr = novelty.threshold_ if novelty_threshold is None else novelty_threshold
            ops.iforest_depth_cut(thr, 1, 1.0)  # ValueError unless inside (0, 1)
            self._novelty = novelty.to(str(self.device))
            self._novelty_threshold = float(thr)
            self.d_nov: Dict[str, torch.Tensor] = {}
            self.h_nov: Dict[str, torch.Tensor] = {}
        elif novelty_threshold is not None:
            raise ValueError("novelty_threshold needs novelty=")
        if explain is not None:
            from .utils.schema import FEATURE_SHORT_NAMES

            if explain not in models:
                raise ValueError(f"explain={explain!r} is not a key of models")
            forest = models[explain]
            if getattr(forest, "kind", "") != "random_forest" or not hasattr(forest, "explain_device"):
                raise ValueError(
                    f"explain={explain!r} holds a {type(forest).__name__}, not a random forest: "
                    "only a forest's verdicts are explained"
                )
            if forest.trees_ is None:
                raise ValueError("explain= takes a fitted forest")
            if not 2 <= len(forest.classes_) <= 8:
                raise ValueError(
                    f"explain= explains forests of 2..8 classes, {explain!r} has {len(forest.classes_)}"
                )
            self._explain = explain
            self._explain_matrix = bool(explain_matrix)
            self.explain_bias = forest.explain_tables["bias"].numpy().copy()
            self.explain_features = FEATURE_SHORT_NAMES
            self.d_exp: Dict[str, torch.Tensor] = {}
            self.h_exp: Dict[str, torch.Tensor] = {}
        elif explain_matrix:
            raise ValueError("explain_matrix needs explain=")
        self.confidence: Dict[str, np.ndarray] = {}
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self.last_latency_s = 0.0

    # -- compute pipeline (captured) -----------------------------------
    def _compute(self) -> None:
        from . import ops

        X = ops.flow_features(self.d_cur, self.d_prev, self.d_times)
        staged = self.smoother is not None or self._traffic_key is not None
        n_live = self.d_nlive if staged else None
        if self._novelty is not None and self._traffic_key is None:
            self._score_novelty(X, None)
        for name, labels, conf in self._predict_all(X, n_live):
            if conf is not None:
                self._keep(self.d_conf, self.h_conf, name, conf)
            self._keep(self.d_labels, self.h_labels, name, labels)
            if name == self._explain:
                for key, value in self._explain_pass(X, labels).items():
                    self._keep(self.d_exp, self.h_exp, key, value)
            if name == self._traffic_key:
                if self._novelty is not None:  # flagged flows count as unknown
                    labels = self._score_novelty(X, labels)
                # rows past the live count hold counters of earlier polls
                totals = self._account(X, labels, conf, n_live)
                if self._d_traffic is None:
                    self._d_traffic = totals
                    self._h_traffic = torch.empty_like(
                        totals, device="cpu", pin_memory=self.device.type == "cuda"
                    )
                else:
                    self._d_traffic.copy_(totals)
                if self._top_k is not None:
                    rows, rates = self._rank(X, labels, conf, n_live)
                    self._keep(self.d_top, self.h_top, "rows", rows)
                    self._keep(self.d_top, self.h_top, "rates", rates)

    def _novelty_pass(self, X: torch.Tensor, labels: Optional[torch.Tensor]):
        """(score, flags, labels with -1 in the flagged rows | None): the one
        run of the score kernel of a pass."""
        if labels is not None and labels.dtype != torch.int32:  # a CPU model's int64 argmax
            labels = labels.to(torch.int32)
        return self._novelty.novelty_device(X, labels, self._novelty_threshold)

    def _score_novelty(self, X: torch.Tensor, labels: Optional[torch.Tensor]):
        """_novelty_pass into the static buffers; returns the masked labels."""
        score, flags, masked = self._novelty_pass(X, labels)
        self._keep(self.d_nov, self.h_nov, "score", score)
        self._keep(self.d_nov, self.h_nov, "flags", flags)
        return masked

    def _explain_pass(self, X: torch.Tensor, labels: torch.Tensor) -> Dict[str, torch.Tensor]:
        """{"why", "why_value"[, "contrib"]} of the explained forest's own
        labels: the one run of the explain kernel of a pass."""
        if labels.dtype != torch.int32:
            labels = labels.to(torch.int32)
        contrib, why, why_value, _ = self.models[self._explain].explain_device(
            X, labels, want_matrix=self._explain_matrix
        )
        out = {"why": why, "why_value": why_value}
        if self._explain_matrix:
            out["contrib"] = contrib
        return out

    def _publish_explain(self, got: Dict[str, torch.Tensor], n: int) -> None:
        self.why = got["why"][:n].cpu().numpy().copy()
        self.why_value = got["why_value"][:n].cpu().numpy().copy()
        if self._explain_matrix:
            self.contributions = got["contrib"][:n].cpu().numpy().copy()

    def _account(self, X: torch.Tensor, labels: torch.Tensor,
                 conf: Optional[torch.Tensor], n_live: Optional[torch.Tensor]) -> torch.Tensor:
        from . import ops

        if labels.dtype != torch.int32:  # a CPU model's int64 argmax
            labels = labels.to(torch.int32)
        mc = self._traffic_min_conf
        return ops.class_traffic(
            X, labels, len(self.traffic_classes) - 1, conf if mc > 0.0 else None, mc, n_live
        )

    def _rank(self, X: torch.Tensor, labels: torch.Tensor,
              conf: Optional[torch.Tensor], n_live: Optional[torch.Tensor]):
        """(rows, rates) of ops.class_top_flows over what _account counts."""
        from . import ops

        if labels.dtype != torch.int32:  # a CPU model's int64 argmax
            labels = labels.to(torch.int32)
        mc = self._traffic_min_conf
        return ops.class_top_flows(
            X, labels, len(self.traffic_classes) - 1, self._top_k, self._top_columns,
            conf if mc > 0.0 else None, mc, n_live,
        )

    def _keep(self, dev: Dict[str, torch.Tensor], host: Dict[str, torch.Tensor],
              name: str, value: torch.Tensor) -> None:
        """Into the static buffer of that name (the first call makes it)."""
        if name in dev:
            dev[name].copy_(value)
        else:
            dev[name] = value
            host[name] = torch.empty_like(
                value, device="cpu", pin_memory=self.device.type == "cuda"
            )

    def _predict_all(self, X: torch.Tensor, n_live: Optional[torch.Tensor] = None):
        """Yields (name, labels, conf | None) per model, then the vote's and,
        with smooth=, the smoothed verdict's (``n_live``: the smoother's).
        A member's probabilities come from its own kernel next to its
        unchanged label kernel, except the forest's: a forest is walked once
        per poll, by the scores kernel, which gives its probabilities, and
        its labels and confidence where it is a confidence model too."""
        probas: Dict[str, torch.Tensor] = {}
        for name, model in self.models.items():
            member = name in self._ens_members
            conf = None
            if member and hasattr(model, "predict_scores"):
                probas[name], labels, c = model.predict_scores(X)
                if name in self._conf_models:
                    conf = c
            else:
                if name in self._conf_models:
                    labels, conf = model.predict_index_conf(X)
                else:
                    labels = model.predict_index(X)
                if member:
                    probas[name] = model.predict_proba_device(X)
            yield name, labels, conf
        if self.ensemble is not None:
            avg, labels, conf = self.ensemble.vote(
                [probas[n] for n in self._ens_members], want_proba=self.smoother is not None
            )
            yield "ensemble", labels, conf
            if self.smoother is not None:
                labels, conf = self.smoother.update(avg, n_live)
                yield "smoothed", labels, conf

    def _capture(self) -> None:
        # the warm-up passes would each move the smoother on: put its state
        # back afterwards, so that the first replay is the first update
        if self.smoother is not None:
            saved = self.smoother.state.clone(), self.smoother.held.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):  # warmup allocations outside the graph
                self._compute()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._compute()
        if self.smoother is not None:
            self.smoother.state.copy_(saved[0])
            self.smoother.held.copy_(saved[1])
        self._graph = g

    def _smooth_begin(self, table: FlowTable, n: int) -> None:
        """Before a pass over ``table``: a table that shrank or a different
        table holds other flows in the same slots, so the history goes."""
        if table is not self._smooth_table or n < self._smooth_n:
            self.smoother.reset()
        self._smooth_table, self._smooth_n = table, n

    # -- per-poll entry -------------------------------------------------
    def classify(self, table: FlowTable) -> Dict[str, np.ndarray]:
        """Run one classification pass over every live flow; returns
        {model_name: labels[n] int32} (class indices).  With
        ``confidence=True`` the pass also leaves {model_name: float32[n]} in
        ``self.confidence`` for the models that support it.  With
        ``ensemble=`` both carry the vote's under the key "ensemble", and
        with ``smooth=`` the smoothed verdict's under "smoothed"."""
        n = len(table)
        t0 = time.perf_counter()
        if self.smoother is not None:
            self._smooth_begin(table, n)
        if n > self.capacity:
            return self._classify_unbounded(table)
        if self.smoother is not None or self._traffic_key is not None:
            self._h_nlive_np[0] = n
            self.d_nlive.copy_(self.h_nlive, non_blocking=True)
        cur, prev, times = table.counters_snapshot()
        self.h_cur[:n] = torch.from_numpy(cur)
        self.h_prev[:n] = torch.from_numpy(prev)
        self.h_times[:n] = torch.from_numpy(times)
        if self.device.type == "cuda":
            self.d_cur.copy_(self.h_cur, non_blocking=True)
            self.d_prev.copy_(self.h_prev, non_blocking=True)
            self.d_times.copy_(self.h_times, non_blocking=True)
            if self.use_graph:
                if self._graph is None:
                    self._capture()
                self._graph.replay()
            else:
                self._compute()
            out = {}
            keys = list(self.models) + self._vote_keys
            for name in keys:
                self.h_labels[name].copy_(self.d_labels[name], non_blocking=True)
            for name in self._conf_keys:
                self.h_conf[name].copy_(self.d_conf[name], non_blocking=True)
            if self._traffic_key is not None:
                self._h_traffic.copy_(self._d_traffic, non_blocking=True)
            if self._top_k is not None:
                for key in self.h_top:
                    self.h_top[key].copy_(self.d_top[key], non_blocking=True)
            if self._novelty is not None:
                for key in self.h_nov:
                    self.h_nov[key].copy_(self.d_nov[key], non_blocking=True)
            if self._explain is not None:
                for key in self.h_exp:
                    self.h_exp[key].copy_(self.d_exp[key], non_blocking=True)
            torch.cuda.synchronize()
            for name in keys:
                out[name] = self.h_labels[name][:n].numpy().copy()
            self.confidence = {
                name: self.h_conf[name][:n].numpy().copy() for name in self._conf_keys
            }
            if self._traffic_key is not None:
                self.traffic = self._h_traffic.numpy().copy()
            if self._top_k is not None:
                self.top_flows = self.h_top["rows"].numpy().copy()
                self.top_flow_rates = self.h_top["rates"].numpy().copy()
            if self._novelty is not None:
                self._publish_novelty(self.h_nov["score"][:n], self.h_nov["flags"][:n])
            if self._explain is not None:
                self._publish_explain(self.h_exp, n)
        else:
            self.d_cur.copy_(self.h_cur)
            self.d_prev.copy_(self.h_prev)
            self.d_times.copy_(self.h_times)
            self._compute()
            out = {name: self.d_labels[name][:n].numpy().copy() for name in self.d_labels}
            self.confidence = {
                name: self.d_conf[name][:n].numpy().copy() for name in self._conf_keys
            }
            if self._traffic_key is not None:
                self.traffic = self._d_traffic.numpy().copy()
            if self._top_k is not None:
                self.top_flows = self.d_top["rows"].numpy().copy()
                self.top_flow_rates = self.d_top["rates"].numpy().copy()
            if self._novelty is not None:
                self._publish_novelty(self.d_nov["score"][:n], self.d_nov["flags"][:n])
            if self._explain is not None:
                self._publish_explain(self.d_exp, n)
        self.last_latency_s = time.perf_counter() - t0
        return out

    def _publish_novelty(self, score: torch.Tensor, flags: torch.Tensor) -> None:
        self.novelty_score = score.cpu().numpy().copy()
        self.novel = flags.cpu().numpy().astype(bool)

    def _classify_unbounded(self, table: FlowTable) -> Dict[str, np.ndarray]:
        from . import ops

        t0 = time.perf_counter()
        if self.smoother is not None and self.smoother.ensure_capacity(len(table)):
            self._graph = None  # it holds the buffers that were just replaced
        cur, prev, times = table.counters_snapshot()
        to = lambda a: torch.from_numpy(a).to(self.device)
        X = ops.flow_features(to(cur), to(prev), to(times))
        out = {}
        self.confidence = {}
        if self._novelty is not None and self._traffic_key is None:
            self._publish_novelty(*self._novelty_pass(X, None)[:2])
        for name, labels, conf in self._predict_all(X):
            if conf is not None:
                self.confidence[name] = conf.cpu().numpy()
            out[name] = labels.cpu().numpy()
            if name == self._explain:
                self._publish_explain(self._explain_pass(X, labels), len(table))
            if name == self._traffic_key:  # every row of X is a live flow
                if self._novelty is not None:
                    score, flags, labels = self._novelty_pass(X, labels)
                    self._publish_novelty(score, flags)
                self.traffic = self._account(X, labels, conf, None).cpu().numpy()
                if self._top_k is not None:
                    rows, rates = self._rank(X, labels, conf, None)
                    self.top_flows = rows.cpu().numpy()
                    self.top_flow_rates = rates.cpu().numpy()
        self.last_latency_s = time.perf_counter() - t0
        return out
