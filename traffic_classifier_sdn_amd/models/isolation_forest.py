"""Isolation forest: a per-flow novelty score (Liu, Ting & Zhou, ICDM 2008).

Every classifier here is closed-set: a flow that belongs to none of the
training classes still gets one of their names, often with a high class
confidence.  An isolation forest scores how UNLIKE the training rows a row
is: random axis-parallel splits isolate an unusual row after few of them, so
a short average path through the trees means "novel".  It is scale-free on
heavy-tailed rate features, fits in milliseconds on the host, and its score
is a traversal of packed 8-byte nodes (csrc/iforest_kernels.hip).

The detector is NOT a classifier: it has no classes, no ``predict_index``
and no probabilities, and the ensemble, the serve engine and the CLI refuse
it in those roles.  It rides along with a classifier (``novelty=`` of
GpuServeEngine and RealtimeClassifier) and turns flagged flows to "unknown".

score = 2^(-mean_t h_t(x) / c(psi)) in (0, 1], higher meaning more anomalous
(sklearn's ``-score_samples``), with h the depth of the leaf a row reaches
plus c(rows in that leaf), c(n) the average path length of an unsuccessful
binary-search-tree lookup among n rows, and psi the rows per tree.
"""

from __future__ import annotations

import math
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from .. import ops
from .base import ArrayLike, Estimator, as_tensor

_TREE_KEYS = ("left", "right", "feature", "threshold", "n_node_samples")


def _build_isolation_tree(X: np.ndarray, rng: np.random.Generator, max_depth: int) -> Dict[str, np.ndarray]:
    """One isolation tree over the rows of X (f64), nodes in depth-first
    order with left == index + 1.  A node picks a feature uniformly among
    those not constant in it and a threshold uniform in the open interval
    (min, max); it stops at one row, at all-rows-identical, or at max_depth."""
    left: List[int] = []
    right: List[int] = []
    feature: List[int] = []
    threshold: List[float] = []
    nns: List[int] = []

    def build(rows: np.ndarray, depth: int) -> int:
        node = len(left)
        left.append(-1)
        right.append(-1)
        feature.append(-1)
        threshold.append(0.0)
        nns.append(int(rows.shape[0]))
        if rows.shape[0] <= 1 or depth >= max_depth:
            return node
        Xn = X[rows]
        lo, hi = Xn.min(axis=0), Xn.max(axis=0)
        varying = np.nonzero(hi > lo)[0]
        if varying.size == 0:
            return node
        f = int(varying[rng.integers(varying.size)])
        thr = float(rng.uniform(lo[f], hi[f]))
        while not lo[f] < thr < hi[f]:  # uniform() draws from [lo, hi)
            thr = float(rng.uniform(lo[f], hi[f]))
        goes_left = Xn[:, f] <= thr
        feature[node] = f
        threshold[node] = thr
        left[node] = build(rows[goes_left], depth + 1)
        right[node] = build(rows[~goes_left], depth + 1)
        return node

    build(np.arange(X.shape[0]), 0)
    return {
        "left": np.asarray(left, dtype=np.int32),
        "right": np.asarray(right, dtype=np.int32),
        "feature": np.asarray(feature, dtype=np.int32),
        "threshold": np.asarray(threshold, dtype=np.float64),
        "n_node_samples": np.asarray(nns, dtype=np.int32),
    }


class IsolationForest(Estimator):
    kind = "isolation_forest"

    def __init__(
        self,
        n_estimators: int = 100,
        max_samples: int = 256,
        contamination: float = 0.01,
        random_state: int = 0,
        device: Optional[str] = None,
    ):
        super().__init__(device)
        if int(n_estimators) < 1:
            raise ValueError(f"n_estimators must be >= 1, got {n_estimators}")
        if int(max_samples) < 2:
            raise ValueError(f"max_samples must be >= 2, got {max_samples}")
        if not 0.0 < float(contamination) < 1.0:
            raise ValueError(f"contamination must be inside (0, 1), got {contamination}")
        self.n_estimators = int(n_estimators)
        self.max_samples = int(max_samples)
        self.contamination = float(contamination)
        self.random_state = int(random_state)
        self.classes_ = None
        self.trees_: Optional[List[Dict[str, np.ndarray]]] = None
        self.max_samples_: Optional[int] = None  # psi: rows each tree was grown on
        self.threshold_: Optional[float] = None  # a score above it is novel
        self._forest = None  # flattened SoA (lazy)

    # -- fit -------------------------------------------------------------
    def fit(self, X: ArrayLike, y: Optional[ArrayLike] = None):
        """Host numpy builds the trees on the rows as the kernels see them
        (rounded to f32).  Tree t is seeded from (random_state, t) alone, so
        it does not depend on how many trees there are."""
        Xn = as_tensor(X, torch.device("cpu"), torch.float32).numpy().astype(np.float64)
        n = Xn.shape[0]
        psi = min(self.max_samples, n)
        if psi < 2:
            raise ValueError(f"an isolation forest needs at least 2 rows, got {n}")
        max_depth = int(math.ceil(math.log2(psi)))
        trees = []
        for t in range(self.n_estimators):
            rng = np.random.default_rng([self.random_state, t])
            rows = rng.choice(n, size=psi, replace=False)
            trees.append(_build_isolation_tree(Xn[rows], rng, max_depth))
        self.trees_ = trees
        self.max_samples_ = psi
        self._forest = None
        # the 1 - contamination quantile of the training scores, taken from
        # the exact path-length sums so that it is the same on every device
        psum = self._run(X, None, None, want_sum=True)[3].cpu().numpy()
        scores = np.exp2(-psum * ops.iforest_consts(self.forest)[2])
        self.threshold_ = float(np.quantile(scores, 1.0 - self.contamination))
        return self

    @classmethod
    def from_sklearn(cls, skl, device: Optional[str] = None) -> "IsolationForest":
        """Take over a fitted sklearn.ensemble.IsolationForest in memory: its
        trees, psi and threshold (``-offset_``)."""
        if float(skl.max_features) != 1.0:
            raise ValueError(
                f"from_sklearn takes max_features == 1.0 (every tree sees every feature), "
                f"got {skl.max_features}"
            )
        m = cls(
            n_estimators=len(skl.estimators_), max_samples=int(skl.max_samples_),
            random_state=0, device=device,
        )
        m.trees_ = []
        for est in skl.estimators_:
            t = est.tree_
            m.trees_.append(
                {
                    "left": np.asarray(t.children_left, dtype=np.int32),
                    "right": np.asarray(t.children_right, dtype=np.int32),
                    "feature": np.asarray(t.feature, dtype=np.int32),
                    "threshold": np.asarray(t.threshold, dtype=np.float64),
                    "n_node_samples": np.asarray(t.n_node_samples, dtype=np.int32),
                }
            )
        m.max_samples_ = int(skl.max_samples_)
        m.threshold_ = float(-skl.offset_)
        return m

    # -- scoring ---------------------------------------------------------
    @property
    def forest(self):
        if self._forest is None:
            if self.trees_ is None:
                raise ValueError("this IsolationForest is not fitted")
            flat = ops.cpu.iforest_flatten(self.trees_, self.max_samples_)
            ops.iforest_consts(flat)  # read psi while it is on the host
            self._forest = {
                k: (v.to(self.device) if isinstance(v, torch.Tensor) else v)
                for k, v in flat.items()
            }
        return self._forest

    def to(self, device: str):
        super().to(device)
        self._forest = None
        return self

    def _run(self, X, labels, threshold, want_sum=False):
        Xt = as_tensor(X, self.device, torch.float32).contiguous()
        return ops.iforest_score(Xt, self.forest, threshold, labels, want_sum)

    def novelty_device(self, X: ArrayLike, labels: Optional[torch.Tensor] = None,
                       threshold: Optional[float] = None):
        """(score f32 [n], flags u8 [n], labels_out int32 [n] | None) device
        tensors from one pass: labels_out is ``labels`` with -1 in the
        flagged rows.  ``threshold=None`` takes ``threshold_``."""
        thr = self.threshold_ if threshold is None else threshold
        return self._run(X, labels, thr)[:3]

    def score_device(self, X: ArrayLike) -> torch.Tensor:
        """f32 [n] device tensor of scores in (0, 1]."""
        return self._run(X, None, None)[0]

    def score_samples(self, X: ArrayLike) -> np.ndarray:
        """f32 [n] in (0, 1], higher meaning more anomalous: sklearn's
        ``-score_samples``."""
        return self.score_device(X).cpu().numpy()

    def predict_novel(self, X: ArrayLike, threshold: Optional[float] = None) -> np.ndarray:
        """bool [n]: score above the threshold (``threshold_`` by default),
        decided on the exact path-length sum."""
        return self.novelty_device(X, None, threshold)[1].cpu().numpy().astype(bool)

    def predict_index(self, X: ArrayLike) -> torch.Tensor:
        raise ValueError(
            "IsolationForest is a novelty detector, not a classifier: it has no class "
            "index to predict (use score_samples or predict_novel)"
        )

    # -- checkpointing -------------------------------------------------
    def to_params(self) -> Dict[str, Any]:
        return {
            "kind": self.kind,
            "trees": self.trees_,
            "max_samples": int(self.max_samples_),
            "threshold": float(self.threshold_),
            "contamination": self.contamination,
            "random_state": self.random_state,
        }

    @classmethod
    def from_params(cls, params: Dict[str, Any], device: Optional[str] = None):
        m = cls(
            n_estimators=len(params["trees"]), max_samples=int(params["max_samples"]),
            contamination=float(params.get("contamination", 0.01)),
            random_state=int(params.get("random_state", 0)), device=device,
        )
        m.trees_ = [{k: np.asarray(t[k]) for k in _TREE_KEYS} for t in params["trees"]]
        m.max_samples_ = int(params["max_samples"])
        m.threshold_ = float(params["threshold"])
        return m
