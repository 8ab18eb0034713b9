"""RBF-kernel support-vector classifier (reference estimator N2).

predict: fused RBF-Gram + one-vs-one vote op on the libsvm checkpoint layout
(support vectors grouped by class, ``dual_coef`` (C-1, nSV), 15 OVO
intercepts — SURVEY.md §2.3).

fit: one-vs-one SMO (libsvm WSS-1 working-set selection, analytic pair
update) with on-the-fly fused kernel rows — no Gram matrix is materialised,
so the fit scales to the BASELINE 1M-row config; rows shard across ranks
with one candidate all-gather per iteration (models/svc_fit.py).

probabilities: ``CalibratedSVC`` (end of this file) adds Platt sigmoids per
class pair and libsvm's pairwise coupling, as sklearn's
``SVC(probability=True)``; the plain ``SVC`` has no probability methods.
"""

from __future__ import annotations

from typing import Any, Dict, Optional

import numpy as np
import torch

from .. import ops
from ..parallel import dist
from .base import ArrayLike, Estimator, as_tensor, encode_labels
from .svc_fit import smo_fit_pair


class SVC(Estimator):
    kind = "svc"

    def __init__(
        self,
        C: float = 1.0,
        gamma: str | float = "scale",
        tol: float = 1e-3,
        max_iter: int = 200_000,
        device: Optional[str] = None,
        probability: bool = False,
        random_state: int = 0,
    ):
        super().__init__(device)
        self.C = C
        self.gamma = gamma
        self.tol = tol
        self.max_iter = max_iter
        # probability=True: fit() also fits the Platt sigmoids and returns a
        # CalibratedSVC; random_state seeds the folds of that fit
        self.probability = probability
        self.random_state = random_state
        self.support_vectors_: Optional[torch.Tensor] = None
        self.dual_coef_: Optional[torch.Tensor] = None
        self.intercept_: Optional[torch.Tensor] = None
        self.n_support_: Optional[torch.Tensor] = None
        self.gamma_: float = 0.0

    def fit(self, X: ArrayLike, y: ArrayLike, sharded: bool = False):
        """One-vs-one SMO fit (models/svc_fit.py: fused on-the-fly kernel
        rows, HIP kernels on GPU, row-sharded across ranks when ``sharded``
        with one candidate all-gather per iteration).  With
        ``probability=True`` the fit goes on to the Platt sigmoids
        (``_fit_probability``) and returns self as a CalibratedSVC."""
        if self.probability and sharded:
            raise NotImplementedError(
                "SVC(probability=True) has no sharded fit: the cross-validated "
                "sigmoids are fitted on one device"
            )
        Xt = as_tensor(X, self.device, torch.float32)
        n, F = Xt.shape
        if sharded and dist.is_initialized():
            classes_local = np.unique(np.asarray(y).ravel())
            all_classes = [None] * dist.world_size()
            torch.distributed.all_gather_object(all_classes, list(classes_local))
            self.classes_ = np.unique(
                np.concatenate([np.asarray(c) for c in all_classes])
            ).astype(object)
            lut = {c: i for i, c in enumerate(self.classes_)}
            y_idx = torch.tensor([lut[v] for v in np.asarray(y).ravel()], dtype=torch.int64)
        else:
            self.classes_, y_idx = encode_labels(y)
        y_t = y_idx.to(self.device)
        C_cls = len(self.classes_)

        if self.gamma == "scale":
            # sklearn: 1 / (F * Var(all elements of X)); global when sharded
            # device tensor: NCCL collectives reject CPU tensors
            st = torch.tensor(
                [float(Xt.numel()), float(Xt.double().sum()), float((Xt.double() ** 2).sum())],
                dtype=torch.float64, device=self.device,
            )
            dist.allreduce_(st)
            xv = float(st[2] / st[0] - (st[1] / st[0]) ** 2)
            self.gamma_ = 1.0 / (F * xv) if xv > 0 else 1.0
        elif self.gamma == "auto":
            self.gamma_ = 1.0 / F
        else:
            self.gamma_ = float(self.gamma)

        n_pairs = C_cls * (C_cls - 1) // 2
        pair_alpha = torch.zeros(n, n_pairs, dtype=torch.float64)  # signed, local rows
        intercepts = []
        p = 0
        self.n_iter_ = []
        for i in range(C_cls):
            for j in range(i + 1, C_cls):
                sel = (y_t == i) | (y_t == j)
                idx = torch.nonzero(sel, as_tuple=False).squeeze(1)
                Xp = Xt[idx].contiguous()
                yp = torch.where(y_t[idx] == i, 1.0, -1.0).to(torch.float32)
                alpha, b, iters = smo_fit_pair(
                    Xp, yp, C=self.C, gamma=self.gamma_, tol=self.tol, max_iter=self.max_iter
                )
                pair_alpha[idx.cpu(), p] = (alpha.cpu() * yp.double().cpu())
                intercepts.append(b)
                self.n_iter_.append(iters)
                p += 1

        # assemble the libsvm layout (SVs grouped by class); gather shards
        sv_mask = pair_alpha.abs().sum(dim=1) > 1e-12
        Xsv_l = Xt[sv_mask.to(self.device)].double().cpu().numpy()
        ysv_l = y_t[sv_mask.to(self.device)].cpu().numpy()
        asv_l = pair_alpha[sv_mask].numpy()
        if sharded and dist.is_initialized():
            parts = [None] * dist.world_size()
            torch.distributed.all_gather_object(parts, (Xsv_l, ysv_l, asv_l))
            Xsv = np.concatenate([q[0] for q in parts])
            ysv = np.concatenate([q[1] for q in parts])
            asv = np.concatenate([q[2] for q in parts])
        else:
            Xsv, ysv, asv = Xsv_l, ysv_l, asv_l
        order = np.argsort(ysv, kind="stable")
        Xsv, ysv, asv = Xsv[order], ysv[order], asv[order]
        nSV = Xsv.shape[0]
        n_support = np.bincount(ysv, minlength=C_cls)
        dual = np.zeros((C_cls - 1, nSV), dtype=np.float64)
        p = 0
        for i in range(C_cls):
            for j in range(i + 1, C_cls):
                col = asv[:, p]
                for c, other in ((i, j), (j, i)):
                    row = other if other < c else other - 1
                    mask = ysv == c
                    dual[row, mask] = col[mask]
                p += 1
        self.support_vectors_ = torch.as_tensor(Xsv).to(self.device)
        self.dual_coef_ = torch.as_tensor(dual).to(self.device)
        self.intercept_ = torch.tensor(intercepts, dtype=torch.float64, device=self.device)
        self.n_support_ = torch.as_tensor(n_support, dtype=torch.int64).to(self.device)
        self.support_ = torch.nonzero(sv_mask, as_tuple=False).squeeze(1)
        if self.probability:
            self._fit_probability(Xt, y_t)
        return self

    # -- Platt scaling ---------------------------------------------------
    def _fit_probability(self, Xt: torch.Tensor, y_t: torch.Tensor) -> None:
        """libsvm's svm_binary_svc_probability per class pair: decision
        values of every row of the pair from a 5-fold cross-validation (five
        extra pair fits, each scoring its held-out fold), then the sigmoid
        fitted on them.  The folds come from one CPU permutation stream
        seeded with ``random_state``, so a CPU and a GPU fit fold alike.
        Turns self into a CalibratedSVC."""
        C_cls = len(self.classes_)
        rng = np.random.RandomState(self.random_state)
        n_fold = 5
        A, B = [], []
        for i in range(C_cls):
            for j in range(i + 1, C_cls):
                idx = torch.nonzero((y_t == i) | (y_t == j), as_tuple=False).squeeze(1)
                Xp = Xt[idx].contiguous()
                yp = torch.where(y_t[idx] == i, 1.0, -1.0).to(torch.float32)
                m = Xp.shape[0]
                perm = torch.from_numpy(rng.permutation(m))
                dec = torch.zeros(m, dtype=torch.float64)
                for f in range(n_fold):
                    held = perm[f * m // n_fold:(f + 1) * m // n_fold]
                    train = torch.cat([perm[:f * m // n_fold], perm[(f + 1) * m // n_fold:]])
                    if held.numel() == 0:
                        continue
                    ytr = yp[train.to(yp.device)]
                    n_pos, n_neg = int((ytr > 0).sum()), int((ytr < 0).sum())
                    if n_pos == 0 or n_neg == 0:
                        # one class (or nothing) to train on: libsvm's +1, -1, 0
                        dec[held] = float(n_pos > 0) - float(n_neg > 0)
                        continue
                    Xtr = Xp[train.to(Xp.device)].contiguous()
                    alpha, b, _ = smo_fit_pair(
                        Xtr, ytr, C=self.C, gamma=self.gamma_, tol=self.tol, max_iter=self.max_iter
                    )
                    dec[held] = _pair_decision(
                        Xtr, ytr, alpha, b, Xp[held.to(Xp.device)].contiguous(), self.gamma_
                    ).cpu()
                a, b = ops.platt_fit(dec, yp.cpu() > 0)
                A.append(a)
                B.append(b)
        self.probA_ = torch.tensor(A, dtype=torch.float64, device=self.device)
        self.probB_ = torch.tensor(B, dtype=torch.float64, device=self.device)
        self.__class__ = CalibratedSVC

    def calibrate(self, X: ArrayLike, y: ArrayLike) -> "CalibratedSVC":
        """A CalibratedSVC of this model: one Platt sigmoid per class pair,
        fitted on this model's own decision values for the rows of ``X``
        whose label ``y`` is one of the pair's two classes.  Nothing is
        refitted and the support vectors are shared, not copied.  Rows the
        model was trained on make the sigmoids too sharp; use other rows."""
        lut = {str(c): k for k, c in enumerate(self.classes_)}
        y_arr = np.asarray(y).ravel()
        unknown = sorted({str(v) for v in y_arr} - set(lut))
        if unknown:
            raise ValueError(f"labels {unknown} are not classes of this model")
        y_idx = torch.tensor([lut[str(v)] for v in y_arr], dtype=torch.int64)
        m = CalibratedSVC.__new__(CalibratedSVC)
        m.__dict__.update(self.__dict__)
        dec = m.decision_function(X).cpu()
        if dec.shape[0] != y_idx.numel():
            raise ValueError("X and y differ in their row count")
        A, B = [], []
        C_cls = len(self.classes_)
        p = 0
        for i in range(C_cls):
            for j in range(i + 1, C_cls):
                first, second = y_idx == i, y_idx == j
                if not bool(first.any()) or not bool(second.any()):
                    raise ValueError(
                        f"no row of one class of the pair ({self.classes_[i]}, "
                        f"{self.classes_[j]}) to fit its sigmoid on"
                    )
                rows = first | second
                a, b = ops.platt_fit(dec[rows, p], first[rows])
                A.append(a)
                B.append(b)
                p += 1
        m.probA_ = torch.tensor(A, dtype=torch.float64, device=self.device)
        m.probB_ = torch.tensor(B, dtype=torch.float64, device=self.device)
        m.probability = True
        return m

    def predict_index(self, X: ArrayLike) -> torch.Tensor:
        Xt = as_tensor(X, self.device, torch.float32)
        sc = getattr(self, "_svclass", None)
        if sc is None or sc.device != Xt.device:
            # SV -> class byte map; precomputed so the hipGraph-captured
            # serve path never runs repeat_interleave inside capture
            sc = torch.repeat_interleave(
                torch.arange(self.n_support_.numel(), device=Xt.device),
                self.n_support_.to(Xt.device),
            ).to(torch.uint8).contiguous()
            self._svclass = sc
        # raw (f64) params: the op layer caches the f32 copies so the
        # hipGraph serve path replays no conversion kernels
        return ops.svc_predict(
            Xt,
            self.support_vectors_,
            self.dual_coef_,
            self.intercept_,
            self.n_support_,
            self.gamma_,
            svclass=sc,
        )

    def decision_function_ovo(self, X: ArrayLike) -> torch.Tensor:
        Xt = as_tensor(X, self.device, torch.float64)
        K = ops.rbf_kernel(Xt, self.support_vectors_.to(Xt.dtype), self.gamma_)
        return ops.svc_ovo_decision(
            K, self.dual_coef_.double(), self.intercept_.double(), self.n_support_
        )

    # -- checkpointing -------------------------------------------------
    def to_params(self) -> Dict[str, Any]:
        return {
            "kind": self.kind,
            "classes": np.asarray(self.classes_, dtype=object),
            "support_vectors": self.support_vectors_.double().cpu().numpy(),
            "dual_coef": self.dual_coef_.double().cpu().numpy(),
            "intercept": self.intercept_.double().cpu().numpy(),
            "n_support": self.n_support_.cpu().numpy(),
            "gamma": float(self.gamma_),
            "support": getattr(self, "support_", torch.zeros(0, dtype=torch.int64)).cpu().numpy(),
        }

    @classmethod
    def from_params(cls, params: Dict[str, Any], device: Optional[str] = None):
        calibrated = np.size(params.get("probA", ())) > 0 and np.size(params.get("probB", ())) > 0
        if calibrated and not issubclass(cls, CalibratedSVC):
            cls = CalibratedSVC
        elif not calibrated and issubclass(cls, CalibratedSVC):
            raise ValueError("these SVC params hold no probA/probB: load them as an SVC")
        m = cls(device=device)
        if calibrated:
            m.probability = True
            m.probA_ = torch.as_tensor(np.asarray(params["probA"], dtype=np.float64).ravel()).to(m.device)
            m.probB_ = torch.as_tensor(np.asarray(params["probB"], dtype=np.float64).ravel()).to(m.device)
        m.classes_ = np.asarray([str(c) for c in params["classes"]], dtype=object)
        m.support_vectors_ = torch.as_tensor(np.asarray(params["support_vectors"], dtype=np.float64)).to(m.device)
        m.dual_coef_ = torch.as_tensor(np.asarray(params["dual_coef"], dtype=np.float64)).to(m.device)
        m.intercept_ = torch.as_tensor(np.asarray(params["intercept"], dtype=np.float64)).to(m.device)
        m.n_support_ = torch.as_tensor(np.asarray(params["n_support"], dtype=np.int64)).to(m.device)
        m.gamma_ = float(params["gamma"])
        return m


def _pair_decision(
    Xtr: torch.Tensor, y_pm: torch.Tensor, alpha: torch.Tensor, b: float,
    Xq: torch.Tensor, gamma: float,
) -> torch.Tensor:
    """f64 decision values of one fitted pair (``smo_fit_pair``'s alpha and
    b) on the rows ``Xq``: the pair as a two-class model in the libsvm
    layout, through ``ops.svc_decision``.  Positive votes for y = +1."""
    ay = (alpha * y_pm.double()).to(Xtr.device)
    sv = alpha.to(Xtr.device).abs() > 1e-12
    pos, neg = sv & (y_pm > 0), sv & (y_pm < 0)
    SV = torch.cat([Xtr[pos], Xtr[neg]]).float().contiguous()
    # f32 already: one-off fold models must not fill the op layer's caches
    dual = torch.cat([ay[pos], ay[neg]]).float().unsqueeze(0).contiguous()
    n_support = torch.tensor([int(pos.sum()), int(neg.sum())], dtype=torch.int64, device=Xtr.device)
    intercept = torch.tensor([b], dtype=torch.float32, device=Xtr.device)
    return ops.svc_decision(Xq, SV, dual, intercept, n_support, gamma)[:, 0]


class CalibratedSVC(SVC):
    """An SVC with class probabilities, as sklearn's SVC(probability=True):
    a Platt sigmoid per class pair (``probA_``, ``probB_``, in the pair order
    of the decision values) and libsvm's pairwise coupling.  It comes from
    ``SVC.calibrate``, from ``SVC(probability=True).fit`` or from a
    checkpoint that holds the sigmoids; the plain SVC has none of these
    methods, which is how the CLI, the serve engine and the ensemble tell
    the two apart.

    ``predict`` and ``predict_index`` are the parent's one-vs-one vote,
    unchanged.  The vote and the largest coupled probability are different
    rules and disagree on some rows (7.9 % of 800 held-out rows of the
    shipped model), as they do in sklearn; the confidence reported here is
    the coupled probability of the VOTED class, never the row maximum, so a
    label does not change when a confidence is asked for.
    """

    def _sv_classes(self, device: torch.device) -> torch.Tensor:
        sc = getattr(self, "_svclass", None)
        if sc is None or sc.device != device:
            # as in predict_index: made once, outside any graph capture
            sc = torch.repeat_interleave(
                torch.arange(self.n_support_.numel(), device=device),
                self.n_support_.to(device),
            ).to(torch.uint8).contiguous()
            self._svclass = sc
        return sc

    def decision_function(self, X: ArrayLike) -> torch.Tensor:
        """f64 [n, C(C-1)/2] one-vs-one decision values, pairs (0,1), (0,2),
        ... (the ``ovo`` shape).  On the GPU they are accumulated exactly as
        the label kernel accumulates them; on the CPU they are the f64
        decision function of f64 rows."""
        dtype = torch.float32 if self.device.type == "cuda" else torch.float64
        Xt = as_tensor(X, self.device, dtype)
        return ops.svc_decision(
            Xt,
            self.support_vectors_,
            self.dual_coef_,
            self.intercept_,
            self.n_support_,
            self.gamma_,
            svclass=self._sv_classes(Xt.device),
        )

    def _couple(self, X: ArrayLike):
        return ops.svc_couple(
            self.decision_function(X), self.probA_, self.probB_, len(self.n_support_)
        )

    def predict_scores(self, X: ArrayLike):
        """(proba f32[n,C], idx int32[n], conf float32[n]) device tensors
        from ONE walk over the support vectors and one coupling pass: idx is
        the one-vs-one vote, conf the coupled probability of that class."""
        proba, idx, conf = self._couple(X)
        return proba.to(torch.float32), idx, conf.to(torch.float32)

    def predict_proba(self, X: ArrayLike) -> np.ndarray:
        """Coupled class probabilities (sklearn SVC(probability=True) API):
        f64 on the CPU, the kernel's f32 on the GPU."""
        return self._couple(X)[0].cpu().numpy()

    def predict_proba_device(self, X: ArrayLike) -> torch.Tensor:
        """predict_proba as an f32 [n,C] tensor on the model's device (the
        soft-vote ensemble's input)."""
        return self.predict_scores(X)[0]

    def predict_index_conf(self, X: ArrayLike):
        """(idx int32[n], conf float32[n]) device tensors: the voted class
        and its coupled probability."""
        _, idx, conf = self.predict_scores(X)
        return idx, conf

    def predict_with_confidence(self, X: ArrayLike):
        """(labels, conf): ``predict(X)`` and the coupled probability of
        that label, which is not always the row's largest probability."""
        idx = self.predict_index(X).cpu().numpy()
        proba = self.predict_scores(X)[0].cpu().numpy()
        labels = idx if self.classes_ is None else self.classes_[idx]
        return labels, proba[np.arange(len(idx)), idx].astype(np.float32)

    def to_params(self) -> Dict[str, Any]:
        params = super().to_params()
        params["probA"] = self.probA_.double().cpu().numpy()
        params["probB"] = self.probB_.double().cpu().numpy()
        return params
