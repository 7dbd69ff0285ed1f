"""Sharded robust-aggregation policies.

Each policy turns the per-rank payload (the local logical workers' flat gradients)
into the decoded global gradient, replicated on every rank.  All of them follow the
same xGMI-friendly shape: one all_to_all of d/world shards, decode on the local shard
(HIP kernels via draco_amd.ops), tiny allreduces for cross-shard decisions, one
all_gather of the decoded shard.  Reference semantics per policy:

  mean         baseline_master.py:202-207,267-269   (plain averaging)
  maj_vote     rep_master.py:141-168                (group-wise Boyer-Moore vote)
  geo_median   baseline_master.py:271-276           (per-layer Weiszfeld)
  krum         baseline_master.py:278-296           (per-layer Krum selection)
  multi_krum   (not in the reference) arXiv:1703.02757  (per-layer mean of the P-f best Krum scores)
  bulyan       (not in the reference) arXiv:1802.07927  (per-layer iterated Krum, then mean around median)
  median       (not in the reference) arXiv:1803.01498  (coordinate-wise median)
  trimmed_mean (not in the reference) arXiv:1803.01498  (coordinate-wise b-trimmed mean)
  meamed       (not in the reference) arXiv:1802.10116  (mean of the P-b values nearest the median)
  phocas       (not in the reference) arXiv:1805.09682  (mean of the P-b values nearest the b-trimmed mean)
  centered_clip (not in the reference) arXiv:2012.10333 (iterated clipped steps from the previous aggregate)
  cyclic       cyclic_master.py:103-188             (DFT-code algebraic decode)
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..coding import COLLUDING_MODES, CyclicCode
from .comm import Communicator
from .flat import FlatSpace


def inject_encoded_(enc: torch.Tensor, mode: str) -> None:
    """The adversary of the cyclic approach, in place on a (2, n) view of a worker's
    encoded (re, im) planes: the whole planes, or the [lo, hi) columns of one bucket.
    The reference injects on the encoded complex combination with cyclic=True
    (additive error, cyclic_worker.py:181-183 / model_ops/utils.py:8-11).  Every mode
    but gauss is per element, so slices compose to the whole; gauss scales its noise by
    the mean magnitude of the view it is given."""
    if mode == "rev_grad":
        enc.add_(enc, alpha=ops.fallback.ADVERSARY_)
    elif mode == "constant":
        enc[0].add_(ops.fallback.ADVERSARY_)
    elif mode in ("random", "none", ""):
        pass
    elif mode == "gauss":
        enc.add_(torch.randn_like(enc) * enc.abs().mean().clamp(min=1e-12) * 100.0)
    else:
        raise ValueError(mode)


class Aggregator:
    """Base: owns comm + space, provides the exchange/allgather plumbing.

    Overlap: the trainer may call start_row(payload, r) as soon as payload row r is
    final (backward done + adversary injected) — the all_to_all for that row then
    runs on the communication stream while the next logical worker's backward
    computes.  aggregate() exchanges any not-yet-started rows and waits.
    """

    name = "base"
    # coding.collusion.Collusion or None: colluding adversaries (alie / ipm) see the
    # honest rows only after the exchange, so they act inside exchanged().  The trainer
    # sets collusion.rows from the host-side schedule before every aggregate().
    collusion = None
    # the most rows the rule's HIP kernel holds (None: no limit) and why; _check_rows
    # is the CPU-side config check, so a bad count fails at construction and not at
    # the first kernel launch on the GPU
    MAX_WORKERS = None
    MAX_WORKERS_WHY = ""

    def __init__(self, comm: Communicator, space: FlatSpace, comm_dtype=torch.float32):
        self.comm = comm
        self.space = space
        self.comm_dtype = comm_dtype  # bf16 = K12 wire compression (all_to_all paths)
        self._out = torch.zeros(space.d_pad, dtype=torch.float32, device=space.device)
        self._shard_out = torch.zeros(space.shard, dtype=torch.float32, device=space.device)
        self.local_seg = space.local_seg_bounds(comm.rank).to(space.device)
        self._recv = None
        self._send = None
        self._recv32 = None
        self._works: list = []
        self._started: set = set()
        self._pending_copies: list = []  # (tmp2d, row, slo, shi) from bucket exchanges

    # ---------------------------------------------------------- row exchange
    def _ensure_recv(self, rows: int, device) -> None:
        if self._recv is None or self._recv.shape[0] != rows:
            # zeros, not empty: the bucketed path never transmits the [d, d_pad)
            # padding tail (payload padding is always zero), so recv must start zero
            self._recv = torch.zeros(rows, self.comm.world, self.space.shard,
                                     dtype=self.comm_dtype, device=device)
            if self.comm_dtype != torch.float32:
                self._send = torch.empty(rows, self.space.d_pad,
                                         dtype=self.comm_dtype, device=device)
                self._recv32 = torch.empty(rows, self.comm.world, self.space.shard,
                                           dtype=torch.float32, device=device)

    def start_row(self, payload: torch.Tensor, row: int) -> None:
        if not self.comm.distributed:
            return
        self._ensure_recv(payload.shape[0], payload.device)
        if self.comm_dtype != torch.float32:
            self._send[row].copy_(payload[row])  # fp32 -> bf16 cast on device
            send_row = self._send[row]
        else:
            send_row = payload[row]
        w = self.comm.all_to_all_row(send_row, self._recv[row], async_op=True)
        if w is not None:
            self._works.append(w)
        self._started.add(row)

    def start_bucket(self, payload: torch.Tensor, row: int, lo: int, hi: int) -> None:
        """Exchange just the [lo, hi) flat range of one payload row (posted from a
        post-accumulate-grad hook while the rest of backward still computes — the
        per-layer comm/compute overlap, reference lenet.py:114-218 interleaved
        isends).  Same wire format as start_row, delivered into the same recv slots;
        the trainer calls mark_row_started(row) once every bucket of the row is
        posted."""
        if not self.comm.distributed:
            return
        self._ensure_recv(payload.shape[0], payload.device)
        world, shard, rank = self.comm.world, self.space.shard, self.comm.rank
        if self.comm_dtype != torch.float32:
            self._send[row, lo:hi].copy_(payload[row, lo:hi])
            src = self._send[row, lo:hi]
        else:
            src = payload[row, lo:hi]
        in_splits = [max(0, min(hi, (j + 1) * shard) - max(lo, j * shard)) for j in range(world)]
        mlo, mhi = max(lo, rank * shard), min(hi, (rank + 1) * shard)
        m = max(0, mhi - mlo)
        tmp = torch.empty(world * m, dtype=self.comm_dtype, device=payload.device)
        w = self.comm.all_to_all_bucket(src, tmp, in_splits, m)
        if w is not None:
            self._works.append(w)
        if m > 0:
            self._pending_copies.append((tmp.view(world, m), row, mlo - rank * shard, mhi - rank * shard))

    def mark_row_started(self, row: int) -> None:
        self._started.add(row)

    def exchanged(self, payload: torch.Tensor) -> torch.Tensor:
        """(rows, d_pad) payload -> (rows*world, shard) in l-major row order.  With a
        collusion attached, the step's Byzantine rows of that block are overwritten
        (ops.collude_) before the rule reads it."""
        recv = self._exchange(payload)
        col = self.collusion
        if col is not None and col.rows:
            # baseline approach: recv row l*world + src IS logical worker l*world + src
            ops.collude_(recv, col.rows, col.a, col.b)
        return recv

    def _check_rows(self, P: int) -> None:
        if self.MAX_WORKERS is not None and P > self.MAX_WORKERS:
            raise ValueError(f"{self.name} supports at most {self.MAX_WORKERS} workers "
                             f"(got {P}): {self.MAX_WORKERS_WHY}")

    def _start_rest(self, payload: torch.Tensor) -> None:
        for r in range(payload.shape[0]):
            if r not in self._started:
                self.start_row(payload, r)

    def _drain(self) -> None:
        for w in self._works:
            w.wait()
        self._works = []
        self._started = set()

    def _exchange(self, payload: torch.Tensor) -> torch.Tensor:
        rows = payload.shape[0]
        if not self.comm.distributed:
            return payload.view(rows, self.space.shard)
        self._start_rest(payload)
        self._drain()
        for tmp2d, row, slo, shi in self._pending_copies:
            self._recv[row, :, slo:shi].copy_(tmp2d)
        self._pending_copies = []
        if self.comm_dtype != torch.float32:
            self._recv32.copy_(self._recv)  # upcast once; decode kernels stay fp32
            return self._recv32.view(rows * self.comm.world, self.space.shard)
        return self._recv.view(rows * self.comm.world, self.space.shard)

    def aggregate(self, payload: torch.Tensor, step: int) -> torch.Tensor:
        raise NotImplementedError

    def state(self):
        """The (d_pad,) flat tensor a checkpoint must carry for this rule to resume
        exactly, or None: every rule but centered clipping is memoryless."""
        return None


class MeanAggregator(Aggregator):
    """Plain averaging over all P = L*world logical workers.

    Mean commutes with sharding, so no all_to_all is needed: start_row posts an
    async per-row reduce_scatter (the sum happens in-flight on the wire), which
    both gives the baseline path the same backward/comm overlap as the coded
    paths and ships each byte exactly once (round-1 bug: the base-class
    all_to_all was posted but never awaited — dead traffic + unbounded _works)."""

    name = "mean"

    def __init__(self, comm, space, num_workers: int):
        super().__init__(comm, space)
        self.num_workers = num_workers
        self._rs_shards = None  # (rows, shard) per-row reduce_scatter outputs
        self._bucketed = False

    def start_row(self, payload: torch.Tensor, row: int) -> None:
        if not self.comm.distributed:
            return
        if self._rs_shards is None or self._rs_shards.shape[0] != payload.shape[0]:
            self._rs_shards = torch.empty(payload.shape[0], self.space.shard,
                                          dtype=torch.float32, device=payload.device)
        w = self.comm.reduce_scatter_row(payload[row], self._rs_shards[row], async_op=True)
        if w is not None:
            self._works.append(w)
        self._started.add(row)

    def start_bucket(self, payload: torch.Tensor, row: int, lo: int, hi: int) -> None:
        """Mean commutes with summing in-flight: the bucket is an in-place async
        all_reduce of the payload slice (the hook guarantees autograd is done with
        the range), so aggregate() just rescales the row."""
        if not self.comm.distributed:
            return
        w = self.comm.all_reduce(payload[row, lo:hi], async_op=True)
        if w is not None:
            self._works.append(w)
        self._bucketed = True

    def aggregate(self, payload: torch.Tensor, step: int) -> torch.Tensor:
        if not self.comm.distributed:
            ops.sum_rows(payload, self._out)
            self._out /= float(self.num_workers)
            return self._out
        if self._bucketed:
            self._drain()
            self._bucketed = False
            ops.sum_rows(payload, self._out)  # rows now hold cross-rank sums
            self._out /= float(self.num_workers)
            return self._out
        self._start_rest(payload)
        self._drain()
        torch.sum(self._rs_shards, dim=0, out=self._shard_out)
        self._shard_out /= float(self.num_workers)
        self.comm.all_gather_shard(self._shard_out, self._out)
        return self._out


class VoteAggregator(Aggregator):
    """Repetition-code decode: per-group majority vote, then mean of winners.

    Colocated layout: G = world groups of size r; member i of group g is local worker
    slot i of rank (g+i) % world, so received row of member (g, i) is
    src*L + l with src = (g+i) % world, l = i.

    Equality rule: members a, b are equal iff max|a-b| <= atol + rtol*max(|a|inf,|b|inf)
    over the FULL gradient (per-shard maxima combined by a tiny MAX allreduce).
    atol=rtol=0 reproduces the reference's bitwise np.array_equal vote
    (rep_master.py:154-168) — usable on CPU, where autograd is reproducible.  On GPU,
    MIOpen conv backward is not bitwise-reproducible (measured: enabling
    cudnn.deterministic neither fixes it nor is affordable — 15x on conv backward), so
    honest replicas differ by fp-reorder noise and the DEFAULT GPU rule is the
    tolerance vote.  This is a deliberate, MEASURED relaxation of the adversary
    model (tests/test_vote_security.py): a within-ball adversary that wins its
    group's tie-break shifts that group's contribution by at most the ball radius
    (atol + rtol*max|g|) — so the aggregate over G groups by at most s/G of it —
    and training under a persistent within-ball attack still tracks the clean
    curve; anything outside the ball loses the vote.  granularity="segment"
    tightens the ball to per parameter tensor (atol + rtol*max|g_seg| on EVERY
    segment; honest noise margin measured in profiles/segnoise_r02.txt).

    Non-finite members: a member with ANY NaN, +Inf or -Inf value is outside every
    ball.  The vote statistics report +inf for a pair (or segment) that touches a
    non-finite element, and a pair is equal only if its statistic is finite — without
    that, rtol > 0 gives thresh = atol + rtol*inf = inf and "inf <= inf" would admit
    the member.  The test stays on device (no host read).
    """

    name = "maj_vote"

    def __init__(self, comm, space, group_size: int, atol: float = 0.0,
                 rtol: float = 0.0, member_rows=None, comm_dtype=torch.float32,
                 member_mask=None, granularity: str = "row"):
        super().__init__(comm, space, comm_dtype)
        self.atol = atol
        self.rtol = rtol
        # granularity="segment": the tolerance ball is PER PARAMETER TENSOR
        # (max|a-b| <= atol + rtol*max(segmax_a, segmax_b) must hold on EVERY
        # segment).  This shrinks a within-tolerance adversary's reach from
        # rtol*max|g| over the whole gradient to rtol*max|g_seg| per tensor —
        # orders of magnitude tighter for late/small layers — at the cost of a
        # slightly larger (still tiny) stats allreduce.
        assert granularity in ("row", "segment"), granularity
        self.granularity = granularity
        if member_rows is None:
            # colocated layout: G = world groups; member i of group g is local slot i
            # of rank (g+i)%world = row i*world + (g+i)%world (l-major convention of
            # comm.all_to_all_rows)
            member_rows = np.asarray(
                [[i * comm.world + (g + i) % comm.world for i in range(group_size)]
                 for g in range(max(comm.world, 1))]
            )
        self.member_rows = np.asarray(member_rows)  # (G, r)
        self.G, self.r = self.member_rows.shape
        # member_mask[g, i] False = forfeited member (its host rank died; the vote
        # proceeds over the remaining members — the repetition code's erasure form)
        if member_mask is None:
            member_mask = np.ones((self.G, self.r), dtype=bool)
        self.member_mask = np.asarray(member_mask, dtype=bool)
        pairs_a, pairs_b, pg, pi, pj = [], [], [], [], []
        for g, rows in enumerate(self.member_rows):
            for i in range(self.r):
                for j in range(i + 1, self.r):
                    if self.member_mask[g, i] and self.member_mask[g, j]:
                        pairs_a.append(rows[i])
                        pairs_b.append(rows[j])
                        pg.append(g)
                        pi.append(i)
                        pj.append(j)
        self.pairs_a = torch.tensor(pairs_a, dtype=torch.int64, device=space.device)
        self.pairs_b = torch.tensor(pairs_b, dtype=torch.int64, device=space.device)
        # device-side winner selection state (no host round-trip in aggregate():
        # at N=8 a per-step .to("cpu") serialises all ranks on one readback)
        dev = space.device
        self._pg = torch.tensor(pg, dtype=torch.int64, device=dev)
        self._pi = torch.tensor(pi, dtype=torch.int64, device=dev)
        self._pj = torch.tensor(pj, dtype=torch.int64, device=dev)
        eye = torch.eye(self.r, device=dev).expand(self.G, self.r, self.r).clone()
        maskt = torch.tensor(self.member_mask, device=dev)
        eye *= maskt[:, :, None].float()  # forfeited members have empty classes
        self._eye = eye
        self._eqm = torch.empty_like(self._eye)
        # forfeited members can never win the argmax
        self._class_bias = torch.where(maskt, 0.0, -1e9)
        self._alive_count = maskt.sum(dim=1).float()  # (G,)
        self._member_rows_t = torch.tensor(self.member_rows, dtype=torch.int64, device=dev)
        # telemetry: steps where some group saw NO equal pair (tolerance too tight /
        # replicas diverged -> the vote degenerates to an arbitrary pick, which an
        # adversary can exploit).  Accumulated ON DEVICE; read via degenerate_steps.
        self._deg_counter = torch.zeros((), dtype=torch.int64, device=dev)

    @property
    def degenerate_steps(self) -> int:
        return int(self._deg_counter.item())

    @classmethod
    def from_member_rows(cls, comm, space, member_rows, atol: float = 0.0, rtol: float = 0.0):
        return cls(comm, space, group_size=member_rows.shape[1], atol=atol, rtol=rtol,
                   member_rows=member_rows)

    def aggregate(self, payload: torch.Tensor, step: int) -> torch.Tensor:
        recv = self.exchanged(payload)  # (r*world, shard)
        if self.rtol > 0.0 and self.granularity == "segment":
            npairs = self.pairs_a.numel()
            segdiff = ops.segment_pair_maxdiff(recv, self.pairs_a, self.pairs_b,
                                               self.local_seg)  # (n_pairs, L)
            segmax = ops.segment_absmax(recv, self.local_seg)  # (rows, L)
            stats = torch.cat([segdiff.reshape(-1), segmax.reshape(-1)])
            self.comm.all_reduce(stats, op="max")  # per-segment global maxima
            segdiff = stats[: segdiff.numel()].view(npairs, -1)
            segmax = stats[segdiff.numel():].view(recv.shape[0], -1)
            thresh = self.atol + self.rtol * torch.maximum(segmax[self.pairs_a],
                                                           segmax[self.pairs_b])
            eq = (segdiff <= thresh).all(dim=1) & torch.isfinite(segdiff).all(dim=1)
        elif self.rtol > 0.0:
            maxdiff = ops.pair_maxdiff(recv, self.pairs_a, self.pairs_b)  # (n_pairs,)
            rowmax = ops.row_absmax(recv)  # (world*r,)
            stats = torch.cat([maxdiff, rowmax])
            self.comm.all_reduce(stats, op="max")  # full-gradient maxima
            maxdiff, rowmax = stats[: len(maxdiff)], stats[len(maxdiff):]
            thresh = self.atol + self.rtol * torch.maximum(rowmax[self.pairs_a], rowmax[self.pairs_b])
            eq = (maxdiff <= thresh) & torch.isfinite(maxdiff)
        else:
            maxdiff = ops.pair_maxdiff(recv, self.pairs_a, self.pairs_b)
            self.comm.all_reduce(maxdiff, op="max")
            eq = (maxdiff <= self.atol) & torch.isfinite(maxdiff)
        # winner selection ON DEVICE (every rank computes the identical winners from
        # the identical allreduced bits — zero host round-trips in the decode):
        # the winner of group g is a member of its largest equality class.  When a
        # true majority class exists (the coded guarantee: > r/2 honest members)
        # this is exactly the reference's Boyer-Moore result (rep_master.py:154-168);
        # with no majority both picks are arbitrary (the reference takes the last
        # surviving candidate, we take the plurality class — strictly no worse).
        eqf = eq.float()
        eqm = self._eqm
        eqm.copy_(self._eye)
        eqm[self._pg, self._pi, self._pj] = eqf
        eqm[self._pg, self._pj, self._pi] = eqf
        class_size = eqm.sum(dim=2)  # (G, r); forfeited members contribute/score 0
        winner_member = (class_size + self._class_bias).argmax(dim=1)  # deterministic tie-break
        winners = self._member_rows_t.gather(1, winner_member.unsqueeze(1)).squeeze(1)
        if self.r > 1:
            # degenerate: a group with >= 2 alive members and NO equal pair
            deg = (self._alive_count >= 2) & (class_size.max(dim=1).values <= 1.5)
            self._deg_counter += deg.any().to(torch.int64)
        ops.mean_rows(recv, winners, self._shard_out)
        self.comm.all_gather_shard(self._shard_out, self._out)
        return self._out


class GeoMedianAggregator(Aggregator):
    """Per-layer geometric median (Weiszfeld), sharded over d.

    Each iteration: per-(worker, layer) partial squared distances on the local shard,
    one (P, L) allreduce, then the reweighted mean on the shard.  Every rank sees the
    identical allreduced distances, so the iterates stay consistent without any
    further synchronisation.
    """

    name = "geo_median"

    def __init__(self, comm, space, num_workers: int, max_iter: int = 80, tol: float = 1e-7,
                 gpu_iters: int = 24):
        super().__init__(comm, space)
        self.num_workers = num_workers
        self.max_iter = max_iter
        self.tol = tol
        # On GPU: a FIXED iteration count with no convergence readback — each
        # early-exit check is a full host round-trip that serialises all ranks
        # (Weiszfeld converges geometrically; 24 iterations measured ample for
        # P <= 64 points, and the CPU early-exit lane cross-checks the fixpoint).
        self.gpu_iters = gpu_iters

    def aggregate(self, payload: torch.Tensor, step: int) -> torch.Tensor:
        recv = self.exchanged(payload)  # (P, shard)
        P = recv.shape[0]
        on_gpu = recv.is_cuda
        n_iter = self.gpu_iters if on_gpu else self.max_iter
        z = recv.mean(dim=0)  # init at the mean (hdmedians does the same)
        # zeros, not empty: the pad tail past the last segment is never written by
        # segment_weighted_mean, and garbage there (inf) poisons the delta criterion
        z_new = torch.zeros_like(z)
        for it in range(n_iter):
            part = ops.segment_sqdist(recv, z, self.local_seg)  # (P, L)
            self.comm.all_reduce(part)
            dist = part.clamp_min(1e-24).sqrt()
            w = 1.0 / dist
            w = w / w.sum(dim=0, keepdim=True)
            ops.segment_weighted_mean(recv, w, self.local_seg, z_new)
            z, z_new = z_new, z
            # convergence check every 8 iterations (CPU lane only: one fused 2-word
            # allreduce + host sync instead of three per iteration)
            if not on_gpu and ((it & 7) == 7 or it == n_iter - 1):
                stats = torch.stack([(z - z_new).pow(2).sum(), z.pow(2).sum()])
                self.comm.all_reduce(stats)
                d_val, s_val = float(stats[0]), float(stats[1])
                if np.isfinite(d_val) and d_val <= self.tol * self.tol * max(s_val, 1e-12):
                    break
        self.comm.all_gather_shard(z, self._out)
        return self._out


# ------------------------------------------------------------------ Krum-family scoring
# Shared by KrumAggregator, MultiKrumAggregator and BulyanAggregator.  Everything works
# on the allreduced (L, P, P) Gram in fp64 ON DEVICE with no host read (CDNA4 fp64 is
# strong and the matrices are tiny); every rank holds the identical allreduced bits,
# so every rank arrives at the identical selection.
def gram_sq_distances(gram: torch.Tensor) -> torch.Tensor:
    """(L, P, P) Gram -> (L, P, P) fp64 squared distances |x_a|^2 + |x_b|^2 - 2<x_a, x_b>,
    clamped at 0, +inf on the diagonal (a row is not its own neighbour)."""
    g = gram.double()
    P = g.shape[1]
    diag = g.diagonal(dim1=1, dim2=2)  # (L, P)
    d2 = (diag.unsqueeze(2) + diag.unsqueeze(1) - 2.0 * g).clamp_(min=0.0)
    eye = torch.eye(P, dtype=torch.bool, device=d2.device)
    d2.masked_fill_(eye, float("inf"))
    return d2


def krum_scores(d2: torch.Tensor, keep: int) -> torch.Tensor:
    """(L, P) Krum scores: per row, the sum of its `keep` smallest distances."""
    vals, _ = torch.sort(d2, dim=2)
    return vals[:, :, :keep].sum(dim=2)


def selection_distances(gram: torch.Tensor) -> torch.Tensor:
    """gram_sq_distances with every non-finite distance counted as +inf: a row with a
    NaN/Inf element (or one whose squared norm overflows fp32) has a non-finite Gram
    row, and argmin over a NaN score would PICK that row.  (KrumAggregator keeps the
    plain distances: its results are not this change's to alter.)  The result is made
    exactly symmetric (the HIP Gram is by construction, a BLAS one need not be): at
    keep = 1 two rows that are each other's nearest neighbour then tie exactly, and the
    lower index wins on every device."""
    inf = float("inf")
    d2 = torch.nan_to_num(gram_sq_distances(gram), nan=inf, posinf=inf, neginf=inf)
    return torch.minimum(d2, d2.transpose(1, 2))


def select_multi_krum(gram: torch.Tensor, f: int, m: int) -> torch.Tensor:
    """One-shot selection (arXiv:1703.02757 §4): (L, m) int64, per segment the m rows
    of lowest Krum score (sum of the max(P-f-2, 1) smallest distances to the others),
    ties to the lower row index, in score order."""
    d2 = selection_distances(gram)
    P = d2.shape[1]
    scores = krum_scores(d2, max(P - f - 2, 1))
    _, order = torch.sort(scores, dim=1, stable=True)
    return order[:, :m].contiguous()


def select_bulyan(gram: torch.Tensor, f: int, theta: int) -> torch.Tensor:
    """Iterative selection (arXiv:1802.07927): (L, theta) int64 distinct rows per
    segment.  theta times: among the n' rows remaining, score = sum of the
    max(n'-f-2, 1) smallest distances to the other REMAINING rows; the lowest score
    wins (lower index on ties) and leaves the pool.  A removed row is never chosen
    again, even when every remaining score is +inf (f = 0 on the last pick)."""
    d2 = selection_distances(gram)
    L, P = d2.shape[0], d2.shape[1]
    inf = float("inf")
    remaining = torch.ones(L, P, dtype=torch.bool, device=d2.device)
    rows = torch.arange(L, device=d2.device)
    picks = []
    for t in range(theta):
        n_rem = P - t
        pair = remaining.unsqueeze(2) & remaining.unsqueeze(1)
        scores = krum_scores(d2.masked_fill(~pair, inf), max(n_rem - f - 2, 1))
        scores = scores.masked_fill(~remaining, inf)
        best = scores.min(dim=1, keepdim=True).values
        # first remaining row at the best score (argmax of a 0/1 tensor: first maximum)
        pick = (remaining & (scores == best)).to(torch.int32).argmax(dim=1)
        picks.append(pick)
        remaining[rows, pick] = False
    return torch.stack(picks, dim=1)


class KrumAggregator(Aggregator):
    """Per-layer Krum selection (arXiv:1703.02757), sharded over d.

    Pairwise squared distances come from per-segment Gram matrices (one allreduce of
    (L, P, P)); selection score per layer = sum of the P-s-2 smallest distances to the
    other workers, argmin wins (exactly baseline_master.py:279-291).
    """

    name = "krum"
    MAX_WORKERS = 32  # the k_seg_gram LDS tile (draco_kernels.hip GRAM_CHUNK layout)
    MAX_WORKERS_WHY = "the segment-Gram HIP kernel stages a (P, chunk) LDS tile sized for P <= 32"

    def __init__(self, comm, space, num_workers: int, s: int):
        super().__init__(comm, space)
        self.num_workers = num_workers
        self.s = s
        self._check_rows(num_workers)
        # per-column segment id of the local shard (for device-side winner assembly:
        # out[c] = recv[winner[seg_of(c)], c]); zero-length padding tail maps to 0
        # and is zeroed after the gather
        seg = self.local_seg
        lengths = (seg[1:] - seg[:-1]).clamp(min=0)
        dev = space.device
        self._col_seg = torch.repeat_interleave(
            torch.arange(len(lengths), dtype=torch.int64, device=dev), lengths.to(dev))
        self._tail = int(seg[-1])

    def aggregate(self, payload: torch.Tensor, step: int) -> torch.Tensor:
        recv = self.exchanged(payload)  # (P, shard)
        gram = ops.segment_gram(recv, self.local_seg)  # (L, P, P)
        self.comm.all_reduce(gram)
        # selection entirely ON DEVICE (fp64 — CDNA4 fp64 is strong and the matrix
        # is tiny; identical allreduced Gram -> identical winners on every rank)
        d2 = gram_sq_distances(gram)
        scores = krum_scores(d2, max(self.num_workers - self.s - 2, 1))  # (L, P)
        winners = scores.argmin(dim=1)  # (L,)
        out = self._shard_out
        if self._tail > 0:
            col_rows = winners[self._col_seg]  # (tail,)
            torch.gather(recv, 0, col_rows.unsqueeze(0), out=out[: self._tail].unsqueeze(0))
        if self._tail < out.shape[0]:
            out[self._tail:] = 0.0
        self.comm.all_gather_shard(out, self._out)
        return self._out


class _KrumSelectAggregator(Aggregator):
    """Shared pipeline of Multi-Krum and Bulyan: all_to_all, per-segment Gram on the
    local shard, ONE (L, P, P) allreduce, on-device selection of T rows per segment
    (no host read), ONE kernel (ops.segment_mean_around gathers each column's rows
    through the per-segment index table), all_gather.  last_sel keeps the (L, T)
    selection of the latest call, on device."""

    MAX_WORKERS = KrumAggregator.MAX_WORKERS
    MAX_WORKERS_WHY = KrumAggregator.MAX_WORKERS_WHY

    def __init__(self, comm, space, num_workers: int, f: int):
        super().__init__(comm, space)
        self.num_workers = num_workers
        self.f = f
        self.last_sel = None
        self._plan(num_workers)  # config check: fail at construction

    def _plan(self, P: int):
        raise NotImplementedError

    def _check_workers(self, P: int, need: int, why: str) -> None:
        if self.f < 0:
            raise ValueError(f"f must be >= 0, got {self.f}")
        self._check_rows(P)
        if P < need:
            raise ValueError(
                f"{self.name} with f={self.f} needs at least {why} = {need} workers, got {P}")

    def aggregate(self, payload: torch.Tensor, step: int) -> torch.Tensor:
        recv = self.exchanged(payload)  # (P, shard)
        select, keep, clo, chi = self._plan(recv.shape[0])
        gram = ops.segment_gram(recv, self.local_seg)  # (L, P, P)
        self.comm.all_reduce(gram)
        sel = select(gram)  # (L, T)
        self.last_sel = sel
        # writes the whole shard, the zero pad tail past the last segment included
        ops.segment_mean_around(recv, sel, self.local_seg, keep, clo, chi, self._shard_out)
        self.comm.all_gather_shard(self._shard_out, self._out)
        return self._out


class MultiKrumAggregator(_KrumSelectAggregator):
    """Per-layer Multi-Krum (arXiv:1703.02757 §4), sharded over d: the plain mean of the
    m workers of lowest Krum score (default m = P - f), where Krum returns the single
    best one and so gives up the variance reduction of averaging.

    Score of a worker = sum of its max(P-f-2, 1) smallest squared distances to the
    others, from the allreduced per-segment Gram; the m lowest win, ties to the lower
    index.  Needs P >= 2f + 3 and 1 <= m <= P - f; P <= 32 (the Gram kernel's limit).
    Bounds are recomputed per call from the received row count (survivor world).

    Guarantee and its limits.  With at most f non-finite rows (any NaN/Inf element, or a
    squared norm that overflows fp32), no non-finite row is ever selected: every distance
    that touches such a row counts as +inf, an honest row still has at least
    P-1-f >= max(P-f-2, 1) finite distances and so a finite score, there are at least
    P-f >= m honest rows, and a non-finite row scores +inf.  An unselected row is never
    read by the kernel, so its NaNs cannot reach the output (0/1 weights could not
    promise that).  Against FINITE adversaries Multi-Krum inherits Krum's (alpha,
    f)-resilience only in the norm sense: a selected adversarial row that sits close to
    the honest cloud in L2 can still carry one crafted coordinate into the mean (the
    hole Bulyan closes), and the m selected rows are averaged unweighted.
    """

    name = "multi_krum"

    def __init__(self, comm, space, num_workers: int, f: int, m: int | None = None):
        self.m = m
        super().__init__(comm, space, num_workers, f)

    def _plan(self, P: int):
        self._check_workers(P, 2 * self.f + 3, "2f + 3")
        m = P - self.f if self.m is None else self.m
        if not 1 <= m <= P - self.f:
            raise ValueError(f"multi_krum needs 1 <= m <= P - f = {P - self.f}, got m={m}")
        f = self.f
        return (lambda gram: select_multi_krum(gram, f, m)), m, 0, m


class BulyanAggregator(_KrumSelectAggregator):
    """Per-layer Bulyan (arXiv:1802.07927), sharded over d: Krum iteratively selects
    theta = P - 2f workers; then, per coordinate, the mean of the beta = theta - 2f
    selected values nearest their median (ops.column_mean_around's rule over the
    selected rows, median centre).

    Needs P >= 4f + 3 (so beta >= 3); P <= 32 (the Gram kernel's limit).  Bounds are
    recomputed per call from the received row count (survivor world).

    Guarantee and its limits.  With at most f non-finite rows (any NaN/Inf element, or a
    squared norm that overflows fp32), no non-finite row is ever selected: at every pick,
    with n' >= 2f + 1 rows remaining, an honest row has at least n'-1-f >=
    max(n'-f-2, 1) finite distances to the other remaining rows and so a finite score,
    at least n'-f >= 1 honest rows remain, and a non-finite row scores +inf.  FINITE
    corrupted rows can be selected — f >= 2 identical ones win the late picks, where
    max(n'-f-2, 1) = 1 and the score is the distance to the nearest remaining row —
    which is what the second stage is for.  With at
    most f corrupted rows of any kind, at most f of the theta selected rows are
    corrupted and theta > 2f, so per coordinate the median c of the selected values lies
    inside the selected honest rows' [min, max] and |out - c| <= max over selected
    honest h of |h - c| (column_mean_around's radius guarantee with b = 2f >= f): one
    crafted coordinate that slipped through Krum's L2 test moves the output by at most
    the honest spread.  As for mean-around-median, the output itself is NOT confined to
    the honest [min, max].  Selection is per layer, so the guarantee is per layer; it
    is the paper's only for f < (P-3)/4 corrupted workers, not beyond.
    """

    name = "bulyan"

    def _plan(self, P: int):
        self._check_workers(P, 4 * self.f + 3, "4f + 3")
        f = self.f
        theta = P - 2 * f
        beta = theta - 2 * f
        return ((lambda gram: select_bulyan(gram, f, theta)), beta, (theta - 1) // 2,
                theta // 2 + 1)


class TrimmedMeanAggregator(Aggregator):
    """Coordinate-wise median / beta-trimmed mean (arXiv:1803.01498), sharded over d.

    Purely per-coordinate, so the rule commutes with sharding exactly: all_to_all,
    ONE kernel on the local shard (per-column sort of the P received values, mean of
    the kept ranks), all_gather — no cross-shard allreduce, no host read.

    trim=None is the median (mean of the two middle values for even P); trim=b drops
    the b smallest and b largest values of every coordinate.  With at most b
    corrupted workers every output coordinate lies inside the honest workers'
    [min, max], whatever the adversary sends: a NaN sorts as +inf and is trimmed like
    any other extreme.  (More non-finite rows than trim can still yield inf/NaN —
    the trainer's nan-guard then skips the update.)
    """

    MAX_WORKERS = 64  # padded to <= 64 rows
    MAX_WORKERS_WHY = "the column-sort HIP kernel holds a column in registers"

    def __init__(self, comm, space, num_workers: int, trim: int | None = None):
        super().__init__(comm, space)
        self.num_workers = num_workers
        self.trim = trim
        self.name = "median" if trim is None else "trimmed_mean"
        self._check_rows(num_workers)
        if trim is not None and trim < 0:
            raise ValueError(f"trim must be >= 0, got {trim}")
        self._bounds(num_workers)

    def _bounds(self, P: int):
        """Kept rank range [lo, hi) for P received rows (computed per call: the
        survivor world after a rank failure has fewer rows)."""
        if self.trim is None:
            return (P - 1) // 2, P // 2 + 1
        if 2 * self.trim >= P:
            raise ValueError(
                f"trimmed mean with trim={self.trim} per end needs more than "
                f"{2 * self.trim} workers, got {P}")
        return self.trim, P - self.trim

    def aggregate(self, payload: torch.Tensor, step: int) -> torch.Tensor:
        recv = self.exchanged(payload)  # (P, shard)
        lo, hi = self._bounds(recv.shape[0])
        ops.column_trimmed_mean(recv, lo, hi, self._shard_out)
        self.comm.all_gather_shard(self._shard_out, self._out)
        return self._out


class MeanAroundAggregator(Aggregator):
    """Mean around median ("MeaMed", arXiv:1802.10116) and Phocas (arXiv:1805.09682),
    sharded over d: per coordinate, the mean of the P-b values nearest to a robust
    centre c — the median (center="median") or the b-trimmed mean
    (center="trimmed_mean").

    Same shape as TrimmedMeanAggregator: all_to_all, ONE kernel on the local shard
    (ops.column_mean_around: per-column sort, centre, window, mean), all_gather — no
    cross-shard allreduce, no host read.

    Only the b values farthest from c are dropped, on whichever side they lie, so a
    one-sided adversary costs no honest value on the quiet side (trimmed mean drops b
    per end regardless).  Guarantee, with at most b corrupted workers and P > 2b: c
    lies inside the honest workers' [min, max] and |out - c| <= max over honest h of
    |h - c| (the radius guarantee), NaN/Inf inputs included — a NaN sorts as +inf and
    at most b non-finite values never enter the window.  Unlike the median and the
    trimmed mean, the output is NOT confined to the honest [min, max] per coordinate:
    a corrupted value just outside that range can be nearer to c than a far honest
    one.  (More than b non-finite rows can yield inf/NaN — the trainer's nan-guard
    then skips the update.)
    """

    MAX_WORKERS = TrimmedMeanAggregator.MAX_WORKERS
    MAX_WORKERS_WHY = TrimmedMeanAggregator.MAX_WORKERS_WHY

    def __init__(self, comm, space, num_workers: int, b: int, center: str = "median"):
        super().__init__(comm, space)
        if center not in ("median", "trimmed_mean"):
            raise ValueError(f"center must be 'median' or 'trimmed_mean', got {center!r}")
        self.num_workers = num_workers
        self.b = b
        self.center = center
        self.name = "meamed" if center == "median" else "phocas"
        self._check_rows(num_workers)
        self._bounds(num_workers)

    def _bounds(self, P: int):
        """(keep, clo, chi) for P received rows (computed per call: the survivor world
        after a rank failure has fewer rows)."""
        if self.b < 0:
            raise ValueError(f"b must be >= 0, got {self.b}")
        if 2 * self.b >= P:
            raise ValueError(
                f"{self.name} with b={self.b} needs more than {2 * self.b} workers, got {P}")
        if self.center == "median":
            return P - self.b, (P - 1) // 2, P // 2 + 1
        return P - self.b, self.b, P - self.b

    def aggregate(self, payload: torch.Tensor, step: int) -> torch.Tensor:
        recv = self.exchanged(payload)  # (P, shard)
        keep, clo, chi = self._bounds(recv.shape[0])
        ops.column_mean_around(recv, keep, clo, chi, self._shard_out)
        self.comm.all_gather_shard(self._shard_out, self._out)
        return self._out


class CenteredClipAggregator(Aggregator):
    """Centered clipping (Karimireddy, He, Jaggi, "Learning from History for Byzantine
    Robust Optimization", ICML 2021, arXiv:2012.10333), sharded over d: starting from
    the PREVIOUS aggregate v, `iters` times

        v <- v + (1/P) sum_i min(1, tau / |x_i - v|) (x_i - v).

    The only stateful rule here: v is the previous output, which after the all_gather is
    already replicated in self._out, and a rank's v is its own slice of it, so the state
    costs no buffer and no communication.  It is zero before the first step, and again
    in the aggregator rebuilt for a survivor world (KNOWN_ISSUES).

    Shape: all_to_all, then iters + 1 passes of ONE kernel over the local shard
    (ops.clip_step_ applies a clipped step and returns every row's squared distance to
    the new centre; the first pass has zero weights and only measures) with one
    allreduce of P floats between them, all_gather.  The P-element clip arithmetic is
    fp64 torch on device; nothing is read on the host.  last_weights keeps the last
    iteration's clip factors c_i in [0, 1], on device.

    tau > 0 is the paper's fixed radius.  tau <= 0 or NaN selects AUTO, which is this
    project's own choice and not the paper's: the lower median (the (P+1)//2-th
    smallest) of the P distances |x_i - v_0| of the step's first pass, non-finite ones
    counted as +inf, computed once per step.

    Guarantee and its limits.  A row with a non-finite distance (any NaN/Inf element, or
    a squared distance that overflows fp32) gets c = 0: it is excluded rather than
    clipped and, never being read by the update, moves v by nothing.  Every other row
    moves v by at most tau/P in L2 per iteration.  With at most f < P/2 corrupted rows,
    auto tau is at most the largest honest distance, so the corrupted rows together
    move v by at most iters * f/P of it per step.  With a fixed tau the first steps from
    v = 0 move at most iters * tau per step (the paper's behaviour).  The norm is over
    the whole gradient (the paper's), not per layer; the pad tail is zero in x and v
    and stays zero.  The paper pairs the rule with worker-side momentum: that is
    --worker-momentum (Config.worker_momentum, ops.worker_momentum_, applied by the
    trainer before the rows reach any rule; off by default).  It shrinks the variance
    among honest rows, which is what time-coupled attacks hide in; what it did in one
    recorded run is in profiles/convergence_worker_momentum.md.
    """

    name = "centered_clip"
    MAX_WORKERS = 64
    MAX_WORKERS_WHY = "the clip-step HIP kernel holds a column in registers"

    def __init__(self, comm, space, num_workers: int, tau: float = 0.0, iters: int = 3):
        super().__init__(comm, space)
        self._check_rows(num_workers)
        if iters < 1:
            raise ValueError(f"centered_clip needs iters >= 1, got {iters}")
        self.num_workers = num_workers
        tau = float(tau)
        self.tau = tau if tau > 0.0 else None  # None = auto (tau <= 0 or NaN)
        self.iters = int(iters)
        self.last_weights = None

    def state(self) -> torch.Tensor:
        return self._out

    def aggregate(self, payload: torch.Tensor, step: int) -> torch.Tensor:
        recv = self.exchanged(payload)  # (P, shard)
        P = recv.shape[0]  # per call: the survivor world is rebuilt, but this reaches the kernel
        self._check_rows(P)
        v = self._shard_out
        v.copy_(self.space.shard_of(self._out, self.comm.rank))
        inf = float("inf")
        d2 = ops.clip_step_(recv, v, torch.zeros(P, dtype=torch.float32, device=recv.device))
        tau = self.tau
        for it in range(1, self.iters + 1):
            self.comm.all_reduce(d2)
            d = d2.double()
            d = torch.where(torch.isfinite(d), d.sqrt(), torch.full_like(d, inf))
            if tau is None:
                tau = torch.kthvalue(d, (P + 1) // 2).values
            # min(1, tau / d) without the 0/0 and inf/inf of the quotient
            c = torch.where(d <= tau, torch.ones_like(d), tau / d)
            c = torch.where(torch.isfinite(d), c, torch.zeros_like(d))
            d2 = ops.clip_step_(recv, v, (c / P).float(), dist=it < self.iters)
        self.last_weights = c
        self.comm.all_gather_shard(v, self._out)
        return self._out


class CyclicAggregator(Aggregator):
    """Cyclic-code algebraic decode, sharded over d.

    The payload rows here are the ENCODED complex gradients as (2, d) fp32 planes —
    (L*2, d_pad) per rank.  Decode: random projection proj = R @ z (partial per shard,
    one (n, 2) allreduce), host error-location + recombination-vector solve (tiny,
    cached per healthy-set), then out = Re(v @ R)/n on the shard.
    """

    name = "cyclic"

    def __init__(self, comm, space, code: CyclicCode, workers_per_rank: int,
                 comm_dtype=torch.float32, world0: int | None = None, alive=None):
        super().__init__(comm, space, comm_dtype)
        self.code = code
        self.L = workers_per_rank
        self.n = code.n
        # Logical worker w = l*world0 + src0 where world0 is the ORIGINAL world size
        # (the code is built for n = L*world0 and never changes).  `alive` lists the
        # surviving original ranks; workers hosted on dead ranks are permanent
        # ERASURES — known-bad rows the decode removes (<= s of them total with the
        # step's adversaries).  Recv rows are in survivor-world coordinates:
        # worker w's (re, im) payload rows (2l, 2l+1) land at (2l+p)*W' + pos(src0).
        world0 = world0 if world0 is not None else max(comm.world, 1)
        alive = list(alive) if alive is not None else list(range(world0))
        pos = {rk: i for i, rk in enumerate(alive)}
        Wp = max(len(alive), 1)
        w_ids = np.arange(self.n)
        l, src = w_ids // world0, w_ids % world0
        self.alive_w = np.array([int(s) in pos for s in src])
        posv = np.array([pos.get(int(s), 0) for s in src])
        self.rows_re = (2 * l) * Wp + posv
        self.rows_im = (2 * l + 1) * Wp + posv
        self.erased = frozenset(int(w) for w in w_ids[~self.alive_w])
        aw = w_ids[self.alive_w]
        self._alive_rows = torch.tensor(
            np.concatenate([self.rows_re[aw], self.rows_im[aw]]),
            dtype=torch.int64, device=space.device)
        self._alive_idx = aw
        self._z = None
        self._zgen = None

    def aggregate(self, payload_planes: torch.Tensor, step: int,
                  erasures: frozenset = frozenset()) -> torch.Tensor:
        recv = self.exchanged(payload_planes)  # (2L*world', shard)
        # random projection generated ON DEVICE (a shard-sized CPU randn + H2D copy
        # costs ~30 ms at d=11M — it dominated the whole decode); per-rank streams
        # may legitimately use different z (partial projections are summed)
        if self._z is None:
            self._z = torch.empty(self.space.shard, dtype=torch.float32, device=self.space.device)
            self._zgen = torch.Generator(device=self.space.device)
        self._zgen.manual_seed(0x5EED ^ (step * 1000003) ^ self.comm.rank)
        z = self._z.normal_(mean=1.0, std=1.0, generator=self._zgen)
        proj = ops.cyclic_project(recv, z)  # (2L*world',) per-row partial dots
        self.comm.all_reduce(proj)
        pa = proj.to("cpu").numpy().astype(np.float64)
        proj_complex = np.where(self.alive_w, pa[self.rows_re] + 1j * pa[self.rows_im], 0.0)
        known_bad = frozenset(erasures) | self.erased
        syndrome = self.code.W_perp @ proj_complex
        scale = float(np.abs(proj_complex).max())
        if not known_bad and float(np.abs(syndrome).max()) <= 1e-7 * max(scale, 1e-30):
            healthy = np.arange(self.n)
        else:
            healthy = self.code.locate_errors(syndrome, known_bad=known_bad)
        v = self.code.recombination_vector(healthy)
        # Re(v @ R) = sum_w vre[w]*re_row[w] - vim[w]*im_row[w]: one combine kernel
        # over the ALIVE workers' rows (v is zero on erased/adversarial rows anyway)
        va = v[self._alive_idx]
        w = torch.tensor(np.concatenate([np.real(va), -np.imag(va)]) / self.n,
                         dtype=torch.float32, device=recv.device)
        ops.combine_rows(recv, self._alive_rows, w, self._shard_out)
        self.comm.all_gather_shard(self._shard_out, self._out)
        return self._out


# ------------------------------------------------------------------ baseline rule table
# mode -> (class, cfg -> rule arguments), shared by Trainer and the PS master.  The
# count a rule tolerates (Krum's s, the trim per end, b, f) is cfg.worker_fail.
_BASELINE_RULES = {
    "normal": (MeanAggregator, lambda cfg: {}),
    "geometric_median": (GeoMedianAggregator, lambda cfg: {}),
    "krum": (KrumAggregator, lambda cfg: {"s": cfg.worker_fail}),
    "median": (TrimmedMeanAggregator, lambda cfg: {}),
    "trimmed_mean": (TrimmedMeanAggregator, lambda cfg: {"trim": cfg.worker_fail}),
    "meamed": (MeanAroundAggregator, lambda cfg: {"b": cfg.worker_fail, "center": "median"}),
    "phocas": (MeanAroundAggregator,
               lambda cfg: {"b": cfg.worker_fail, "center": "trimmed_mean"}),
    "multi_krum": (MultiKrumAggregator, lambda cfg: {"f": cfg.worker_fail}),
    "bulyan": (BulyanAggregator, lambda cfg: {"f": cfg.worker_fail}),
    "centered_clip": (CenteredClipAggregator,
                      lambda cfg: {"tau": cfg.clip_tau, "iters": cfg.clip_iters}),
}
BASELINE_MODES = "/".join(_BASELINE_RULES)


def build_baseline_aggregator(cfg, comm, space, num_workers: int) -> Aggregator:
    """The baseline approach's rule for cfg.mode over num_workers logical workers."""
    if cfg.mode not in _BASELINE_RULES:
        raise ValueError(f"baseline approach supports modes {BASELINE_MODES}, got {cfg.mode!r}")
    cls, args = _BASELINE_RULES[cfg.mode]
    kwargs, name, hint = args(cfg), None, ""
    if cfg.mode == "normal" and cfg.err_mode in COLLUDING_MODES:
        # MeanAggregator sums inside the reduce-scatter: the honest rows are never
        # visible together.  Under a colluding adversary the plain mean goes over
        # the exchange path instead: the trimmed mean with nothing trimmed.
        cls, kwargs, name = TrimmedMeanAggregator, {"trim": 0}, "mean"
        hint = (f" (mode 'normal' under the colluding err mode {cfg.err_mode!r} is the "
                "trim=0 mean over the exchange path, so that kernel's limit of 64 workers "
                "applies)")
    elif cfg.mode in ("multi_krum", "bulyan"):
        # these two have a floor on the worker count (2f+3, 4f+3) that a default
        # one-worker-per-rank configuration misses: name the modes one can switch to
        hint = f" (baseline approach supports modes {BASELINE_MODES})"
    try:
        agg = cls(comm, space, num_workers=num_workers, **kwargs)
    except ValueError as e:
        raise ValueError(f"{e}{hint}") from None
    if name is not None:
        agg.name = name
    return agg
