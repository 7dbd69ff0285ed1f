"""Worker-side momentum (arXiv:2012.10333): every local logical worker keeps a private
fp32 state row and sends its momentum instead of its gradient.  The adversary
injection acts on the sent row only, so every slot keeps an HONEST state: the schedule
picks different Byzantine workers every step.
"""
from __future__ import annotations

import os

import torch

from .. import ops
from ..utils.checkpoint import _flat_to_params, _params_to_flat


class WorkerMomentum:
    def __init__(self, space, L: int, beta: float):
        self.beta = float(beta)
        self.L = L
        self.state = space.alloc_payload(L)  # (L, d_pad)
        self.first = [True] * L  # slot has sent nothing yet: its next step sets m = g

    def apply(self, payload: torch.Tensor, row: int, lo: int, hi: int) -> None:
        """In place on the final [lo, hi) of payload row `row`, before any injection."""
        ops.worker_momentum_(payload[row, lo:hi], self.state[row, lo:hi], self.beta,
                             self.first[row])

    def row_sent(self, row: int) -> None:
        """The WHOLE row has shipped (in the bucketed path: its last bucket)."""
        self.first[row] = False

    @staticmethod
    def path(train_dir: str, step: int, rank: int) -> str:
        # rank-local sidecar of the checkpoint.  The name must not match model_step_*,
        # which evaluate.py globs and parses.
        return os.path.join(train_dir, f"worker_momentum_step_{step}.rank{rank}")

    def save(self, path: str, space, step: int, world: int) -> None:
        # the state is rank-local (P rows over all ranks), so every rank writes its
        # own rows; per parameter, like the optimizer buffers (layout-independent)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        state = {
            "step": step,
            "beta": self.beta,
            "world": world,
            "L": self.L,
            "first": list(self.first),
            "rows": [_flat_to_params(space, self.state[l]) for l in range(self.L)],
        }
        tmp = path + ".tmp"
        torch.save(state, tmp)
        os.replace(tmp, path)

    def load(self, path: str, space, step: int, world: int, logger) -> None:
        state = None
        if os.path.exists(path):
            state = torch.load(path, map_location="cpu", weights_only=False)
            if state.get("world") != world or state.get("L") != self.L:
                state = None  # rows of another worker layout are not this rank's workers
        self.state.zero_()
        if state is None:
            # every slot starts over with m = g on its next step
            self.first = [True] * self.L
            logger.log({"step": step, "event": "worker_momentum_restart", "path": path})
            return
        for l in range(self.L):
            _params_to_flat(space, state["rows"][l], self.state[l])
        self.first = [bool(f) for f in state["first"]]
