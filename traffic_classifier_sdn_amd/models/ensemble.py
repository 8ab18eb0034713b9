"""Soft-vote ensemble: one verdict and one confidence from several models.

Each member contributes its class probabilities (``predict_proba_device``,
an f32 tensor on the device); the vote is their weighted average over the
sorted union of the members' classes, taken by one kernel
(csrc/ensemble_kernels.hip, ops.ensemble_vote).  A class a member does not
know gets nothing from that member, so a member trained on fewer classes
simply has no say about the others.

The vote adds no accuracy over its best member on the shipped data; what it
adds is a single label with a confidence to reject on (README).
"""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from .base import ArrayLike, Estimator, as_tensor


class SoftVoteEnsemble(Estimator):
    kind = "soft_vote"

    def __init__(self, members: Dict[str, Estimator], weights: Optional[Sequence[float]] = None):
        members = dict(members)
        if not 1 <= len(members) <= 8:
            raise ValueError(f"a soft-vote ensemble takes 1..8 members, got {len(members)}")
        for name, m in members.items():
            if getattr(m, "kind", "") == "isolation_forest":
                raise ValueError(
                    f"ensemble member {name!r} is an IsolationForest, a novelty detector "
                    "with no class probabilities: it cannot vote"
                )
            if not hasattr(m, "predict_proba_device") or getattr(m, "classes_", None) is None:
                raise ValueError(
                    f"ensemble member {name!r} ({type(m).__name__}) has no class probabilities"
                )
        first = next(iter(members.values()))
        super().__init__(str(first.device))
        self.members = members
        self.classes_ = np.unique(
            np.concatenate([np.asarray(m.classes_, dtype=object).astype(str) for m in members.values()])
        ).astype(object)
        if not 2 <= len(self.classes_) <= 8:
            raise ValueError(f"a soft-vote ensemble covers 2..8 classes, got {len(self.classes_)}")
        col = {c: i for i, c in enumerate(self.classes_)}
        self.colmaps: List[List[int]] = [
            [col[str(c)] for c in m.classes_] for m in members.values()
        ]
        # normalised f32 weights, in member order
        self.weights: List[float] = ops.ensemble_weights(weights, len(members))

    # -- the vote --------------------------------------------------------
    def member_probas(self, X: ArrayLike) -> List[torch.Tensor]:
        Xt = as_tensor(X, self.device, torch.float32)
        return [m.predict_proba_device(Xt) for m in self.members.values()]

    def vote(self, probas: Sequence[torch.Tensor], want_proba: bool = False):
        """(avg | None, idx int32[n], conf float32[n]) from the members'
        probabilities, given in member order."""
        return ops.ensemble_vote(
            list(probas), self.colmaps, self.weights, len(self.classes_), want_proba=want_proba
        )

    def predict_index(self, X: ArrayLike) -> torch.Tensor:
        return self.vote(self.member_probas(X))[1]

    def predict_proba(self, X: ArrayLike) -> torch.Tensor:
        return self.vote(self.member_probas(X), want_proba=True)[0]

    def predict_index_conf(self, X: ArrayLike):
        """(idx int32[n], conf float32[n]) device tensors: the voted class
        and its averaged probability."""
        _, idx, conf = self.vote(self.member_probas(X))
        return idx, conf

    def predict_with_confidence(self, X: ArrayLike):
        idx, conf = self.predict_index_conf(X)
        return self.classes_[idx.cpu().numpy()], conf.cpu().numpy().astype(np.float32)

    def to(self, device: str):
        self.device = torch.device(device)
        for m in self.members.values():
            m.to(device)
        return self

    # -- no checkpoint format: an ensemble is its members ------------------
    def to_params(self) -> Dict[str, Any]:
        raise NotImplementedError("a SoftVoteEnsemble has no checkpoint format: save its members")
