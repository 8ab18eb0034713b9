"""Stable per-flow verdicts: class probabilities smoothed across polls.

A model judges every poll alone, so a flow's label flips as its
instantaneous rates move.  ``FlowSmoother`` keeps, per flow slot, an
exponential moving average of the flow's probability row and the label it
last reported, and changes that label only when another class leads the
average by more than a margin (ops.proba_smooth; the kernel is in
csrc/ensemble_kernels.hip).  The flow table is append-only and a flow keeps
its slot for life (flow/state.py), so the slot index is the flow's identity.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import ops


class FlowSmoother:
    def __init__(
        self,
        n_classes: int,
        capacity: int,
        alpha: float,
        switch_margin: float = 0.0,
        device=None,
    ) -> None:
        if not 2 <= int(n_classes) <= 8:
            raise ValueError(f"a FlowSmoother covers 2..8 classes, got {n_classes}")
        if int(capacity) < 1:
            raise ValueError(f"a FlowSmoother needs a capacity of at least 1, got {capacity}")
        self.n_classes = int(n_classes)
        self.alpha = float(alpha)
        self.switch_margin = float(switch_margin)
        self.device = torch.device(device if device is not None else "cpu")
        self.state = torch.zeros(int(capacity), self.n_classes, dtype=torch.float32, device=self.device)
        self.held = torch.full((int(capacity),), -1, dtype=torch.int32, device=self.device)
        # alpha and the margin are refused here as the op refuses them
        ops.proba_smooth_check(
            self.state[:0], self.state, self.held, self.alpha, self.switch_margin, None
        )

    @property
    def capacity(self) -> int:
        return self.state.shape[0]

    def update(
        self, proba: torch.Tensor, n_live: Optional[torch.Tensor] = None
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(labels int32[n], conf float32[n]) for the rows of ``proba``
        [n, C], row r being slot r; ``state`` and ``held`` move on.  Rows at
        or past ``n_live[0]`` (an int32 [1] tensor on the device; None: all
        are live) are reset instead and get their own argmax."""
        return ops.proba_smooth(
            proba, self.state, self.held, self.alpha, self.switch_margin, n_live
        )

    def reset(self) -> None:
        """Forget every flow; the buffers stay where they are."""
        self.held.fill_(-1)
        self.state.zero_()

    def ensure_capacity(self, n: int) -> bool:
        """Room for ``n`` slots: True when the buffers were reallocated (the
        history of the slots so far is copied over)."""
        cap = self.capacity
        if n <= cap:
            return False
        new_cap = max(int(n), 2 * cap)
        state = torch.zeros(new_cap, self.n_classes, dtype=torch.float32, device=self.device)
        held = torch.full((new_cap,), -1, dtype=torch.int32, device=self.device)
        state[:cap] = self.state
        held[:cap] = self.held
        self.state, self.held = state, held
        return True
