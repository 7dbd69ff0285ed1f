"""Nearest-neighbour mixing (NNM): a stateless pre-aggregation step in front of any
baseline rule (Allouah, Farhadkhani, Guerraoui, Gupta, Pinot, Stephan, "Fixing by
Mixing", AISTATS 2023, arXiv:2302.01772).  Every row of the exchanged block is replaced
by the mean of its P-f nearest rows in L2, itself included; the unchanged rule then runs
on the mixed rows.
"""
from __future__ import annotations

import torch

from .. import ops
from .aggregators import selection_distances
from .comm import Communicator

MAX_WORKERS = 32  # one 32x32 matrix tile in ops.mix_rows_, and the Gram kernel's limit


def nnm_weights(gram: torch.Tensor, f: int):
    """(P, P) allreduced Gram -> (W, bad), on gram's device with no host read.

    W (P, P) fp64: row i holds 1/(P-f) at the P-f rows nearest to row i and 0 elsewhere.
    Distances are selection_distances' (fp64, non-finite counted as +inf, exactly
    symmetric) with the self-distance set to 0, so a finite row is its own nearest
    neighbour; ties go to the lower index (stable sort).  bad (P,) bool marks the rows
    whose Gram diagonal is not finite (any NaN/Inf element, or a squared norm that
    overflows fp32): their COLUMNS of W are zero and their ROWS are NaN."""
    P = gram.shape[0]
    d2 = selection_distances(gram.unsqueeze(0))[0]
    d2.fill_diagonal_(0.0)
    near = torch.sort(d2, dim=1, stable=True).indices[:, : P - f]
    w = torch.zeros(P, P, dtype=torch.float64, device=gram.device)
    w.scatter_(1, near, 1.0 / (P - f))
    bad = ~torch.isfinite(gram.diagonal())
    w = torch.where(bad.unsqueeze(0), torch.zeros_like(w), w)
    w = torch.where(bad.unsqueeze(1), torch.full_like(w, float("nan")), w)
    return w, bad


class NearestNeighborMixing:
    """Called on the exchanged (P, shard) block, in place: row i <- mean of the P-f rows
    nearest to row i over the WHOLE gradient (the paper's distance, not per layer).

    Shape: ops.segment_gram over one segment on the local shard, ONE allreduce of P^2
    floats, the selection in fp64 on device (nnm_weights), ONE kernel over the block
    (ops.mix_rows_: Y = W X on the matrix unit, in place, no second (P, shard) buffer).
    P is taken per call; 2f < P <= 32 is checked at construction (when num_workers is
    given) and per call.  last_weights keeps W (fp32, on device) of the latest call.

    The one host round-trip.  A row whose Gram diagonal is not finite is EXCLUDED: its
    column of W is zero, and because a zero weight times a NaN is a NaN, it must also
    not be loaded, which ops.mix_rows_ takes as a host-side row set.  Which rows those
    are is known on the device only, so the set is read back from the allreduced
    diagonal, packed into one 8-byte word (one synchronising readback per call, as the
    cyclic decode has one).  W itself never depends on that read.

    Guarantee and its limits.  With at most f corrupted rows, every honest mixed row is a
    mean of P-f rows of which at least P-2f are honest.  With at most f non-finite rows
    no honest row has one among its neighbours (an honest row has P-f finite distances,
    its own included).  An excluded row's own mixed row is all NaN, so the rule behind
    sees at most as many bad rows as before.  With more than f non-finite rows there is
    no guarantee: an honest row's neighbour set then reaches into the excluded rows and
    its weights sum to less than 1.  The pad tail stays zero in every non-excluded row.
    What mixing did in front of five rules in one recorded run is in
    profiles/convergence_nnm.md; nothing more is claimed about convergence.
    """

    def __init__(self, comm: Communicator, f: int, num_workers: int | None = None):
        self.comm = comm
        self.f = int(f)
        self.last_weights = None
        self._seg = None
        self._seg_key = None
        if self.f < 0:
            raise ValueError(f"nnm needs f >= 0, got {f}")
        if num_workers is not None:
            self._check(num_workers)

    def _check(self, P: int) -> None:
        if P > MAX_WORKERS:
            raise ValueError(f"nnm supports at most {MAX_WORKERS} workers (got {P}): the "
                             "row-mix HIP kernel holds W as one 32x32 matrix tile")
        if P <= 2 * self.f:
            raise ValueError(f"nnm with f={self.f} needs more than {2 * self.f} workers, got {P}")

    def __call__(self, recv: torch.Tensor) -> torch.Tensor:
        P, shard = recv.shape
        self._check(P)
        if self._seg_key != (shard, recv.device):
            self._seg_key = (shard, recv.device)
            self._seg = torch.tensor([0, shard], dtype=torch.int64, device=recv.device)
        gram = ops.segment_gram(recv, self._seg)[0]  # (P, P)
        self.comm.all_reduce(gram)
        w, bad = nnm_weights(gram, self.f)
        self.last_weights = w.float()
        bits = (bad.to(torch.int64) << torch.arange(P, device=bad.device)).sum()
        mask = int(bits.item())  # the one host read
        ops.mix_rows_(recv, self.last_weights, [k for k in range(P) if (mask >> k) & 1])
        return recv
