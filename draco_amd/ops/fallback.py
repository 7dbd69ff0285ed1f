"""Pure-PyTorch implementations of every Draco op.

These are (a) the CPU execution path for tests/gloo lanes and (b) the numerics oracle
the HIP kernels (ops/csrc/) are tested against.  Semantics mirror the reference:
  - fused_sgd_step:  /root/reference/src/optim/sgd_modified.py:53-89
  - fused_adam_step: /root/reference/src/optim/adam_modified.py:32-93
  - inject_:         /root/reference/src/model_ops/utils.py:6-23
  - rows_equal / mean_rows: the majority-vote decode, rep_master.py:154-168
  - encode/proj/recombine:  cyclic code hot GEMVs, cyclic_worker.py:165-194 and
    cyclic_master.py:146-173
"""
from __future__ import annotations

import torch

ADVERSARY_ = -100.0  # reference: model_ops/utils.py:3


# --------------------------------------------------------------------- optimizers
@torch.no_grad()
def fused_sgd_step(
    param: torch.Tensor,
    grad: torch.Tensor,
    momentum_buf: torch.Tensor | None,
    *,
    lr: float,
    momentum: float,
    dampening: float,
    weight_decay: float,
    nesterov: bool,
    first_step: bool,
    guard: torch.Tensor | None = None,
) -> None:
    if guard is not None and not bool(guard):
        return  # nan-guard skip (host read is fine on the CPU path)
    d_p = grad
    if weight_decay != 0.0:
        d_p = d_p.add(param, alpha=weight_decay)
    if momentum != 0.0:
        assert momentum_buf is not None
        if first_step:
            # reference quirk kept deliberately: the very first momentum update has no
            # (1 - dampening) factor (sgd_modified.py:80-82)
            momentum_buf.mul_(momentum).add_(d_p)
        else:
            momentum_buf.mul_(momentum).add_(d_p, alpha=1.0 - dampening)
        if nesterov:
            d_p = d_p.add(momentum_buf, alpha=momentum)
        else:
            d_p = momentum_buf
    param.add_(d_p, alpha=-lr)


@torch.no_grad()
def fused_adam_step(
    param: torch.Tensor,
    grad: torch.Tensor,
    exp_avg: torch.Tensor,
    exp_avg_sq: torch.Tensor,
    max_exp_avg_sq: torch.Tensor | None,
    *,
    step: int,
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
    amsgrad: bool,
    guard: torch.Tensor | None = None,
) -> None:
    if guard is not None and not bool(guard):
        return  # nan-guard skip
    if weight_decay != 0.0:
        grad = grad.add(param, alpha=weight_decay)
    exp_avg.mul_(beta1).add_(grad, alpha=1.0 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1.0 - beta2)
    bias_c1 = 1.0 - beta1**step
    bias_c2 = 1.0 - beta2**step
    if amsgrad:
        assert max_exp_avg_sq is not None
        torch.maximum(max_exp_avg_sq, exp_avg_sq, out=max_exp_avg_sq)
        denom = max_exp_avg_sq.sqrt().add_(eps)
    else:
        denom = exp_avg_sq.sqrt().add_(eps)
    step_size = lr * (bias_c2**0.5) / bias_c1
    param.addcdiv_(exp_avg, denom, value=-step_size)


# --------------------------------------------------------------------- adversary
@torch.no_grad()
def inject_(grad: torch.Tensor, mode: str, cyclic: bool = False) -> None:
    """Byzantine fault injection at the send boundary, in place.

    reference err_simulation: rev_grad -> -100*g (replace), constant -> -100 fill,
    random -> passthrough (left TODO upstream; kept as passthrough for parity, with
    'gauss' provided as a real randomising mode).  cyclic=True adds the error to the
    gradient instead of replacing it (model_ops/utils.py:8-20).
    """
    if mode == "rev_grad":
        err = grad * ADVERSARY_
    elif mode == "constant":
        err = torch.full_like(grad, ADVERSARY_)
    elif mode == "random":
        return  # reference passthrough (model_ops/utils.py:21-23 TODO)
    elif mode == "gauss":
        err = torch.randn_like(grad) * grad.abs().mean().clamp(min=1e-12) * 100.0
    elif mode in ("none", ""):
        return
    elif mode in ("alie", "ipm"):
        raise ValueError(
            f"err mode {mode!r} is a colluding adversary: it needs every honest worker's "
            "values and is applied to the exchanged (P, shard) block by collude_, not to "
            "one worker's gradient")
    else:
        raise ValueError(f"unknown err mode {mode!r}")
    if cyclic:
        grad.add_(err)
    else:
        grad.copy_(err)


@torch.no_grad()
def collude_(x: torch.Tensor, rows, a: float, b: float) -> None:
    """Colluding adversaries that see the honest gradients, in place: every row of x
    listed in `rows` becomes a*mu + b*sigma per column, mu and sigma being the mean and
    the population standard deviation (divide by h) of the h rows NOT listed.  ALIE
    (arXiv:1902.06156) is (a, b) = (1, -z); inner-product manipulation
    (arXiv:1903.03936) is (-eps, 0).

    x: (P, n) fp32 contiguous, 2 <= P <= 64, n % 4 == 0; rows: distinct ints in [0, P),
    at least one row left honest; empty rows (or n == 0) is a no-op.  Honest rows are
    never written.  Per column, in fp32: the honest values are added one at a time in
    ascending row order and divided by float32(h); then, unless b == 0, the squared
    deviations from that mean are added in the same order, divided by float32(h), and
    rooted (two passes: the one-pass E[x^2] - mu^2 form cancels and can go negative).
    The HIP kernel does the same in the same order, up to FMA contraction: it agrees
    within the rounding bound, not bit for bit.  Non-finite inputs propagate by
    ordinary IEEE arithmetic.
    """
    if x.dtype != torch.float32:
        raise ValueError(f"collude_: x must be fp32, got {x.dtype}")
    if x.dim() != 2:
        raise ValueError(f"collude_: x must be 2D, got {x.dim()}D")
    if not x.is_contiguous():
        raise ValueError("collude_: x must be contiguous")
    P, n = x.shape
    if not 2 <= P <= 64:
        raise ValueError(f"collude_ supports 2 <= P <= 64, got {P}")
    if n % 4 != 0:
        raise ValueError(f"collude_: row length must be a multiple of 4, got {n}")
    rows = [int(r) for r in rows]
    for r in rows:
        if not 0 <= r < P:
            raise ValueError(f"collude_: row {r} outside [0, {P})")
    if len(set(rows)) != len(rows):
        raise ValueError(f"collude_: rows must be distinct, got {rows}")
    byz = set(rows)
    honest = [p for p in range(P) if p not in byz]
    if not honest:
        raise ValueError(f"collude_: all {P} rows are Byzantine, need at least one honest row")
    if not rows or n == 0:
        return
    cnt = torch.full((n,), float(len(honest)), dtype=torch.float32, device=x.device)
    acc = x[honest[0]].clone()
    for p in honest[1:]:
        acc = acc + x[p]
    # tensor divisor: an elementwise IEEE division (never a multiply by 1/h)
    mu = torch.div(acc, cnt)
    val = mu * float(a)
    if float(b) != 0.0:
        ss = torch.zeros_like(mu)
        for p in honest:
            dev = x[p] - mu
            ss = ss + dev * dev
        val = val + torch.sqrt(torch.div(ss, cnt)) * float(b)
    for r in rows:
        x[r] = val


@torch.no_grad()
def clip_step_(x: torch.Tensor, v: torch.Tensor, w: torch.Tensor, dist: bool = True):
    """One centered-clipping iteration (arXiv:2012.10333) with the clip weights given:
    in place, v_j += sum over the rows with w_i != 0 of w_i * (x_ij - v_j); returns
    d2 (P,) with d2_i = sum_j (x_ij - v_j_new)^2 over EVERY row (dist=True), else None.

    x: (P, n) fp32 contiguous, 1 <= P <= 64, n % 4 == 0; v: (n,) fp32; w: (P,) fp32,
    w_i >= 0, on x's device.  Per column, in fp32: the terms w_i * (x_ij - v_j) are
    added one at a time in ascending row order, starting from 0, and the sum is then
    added to v_j.  A row with w_i == 0 is skipped, not multiplied by 0, so a NaN in it
    cannot reach v; with every w_i == 0, v is not written.  d2 is summed in fp32 in
    torch's order.  Non-finite values propagate by ordinary IEEE arithmetic.  The HIP
    kernel does the same in the same row order, up to FMA contraction and the order of
    the d2 sum: it agrees within the rounding bound, not bit for bit.
    """
    if x.dtype != torch.float32 or v.dtype != torch.float32 or w.dtype != torch.float32:
        raise ValueError(f"clip_step_: x, v and w must be fp32, got {x.dtype}, {v.dtype}, "
                         f"{w.dtype}")
    if x.dim() != 2:
        raise ValueError(f"clip_step_: x must be 2D, got {x.dim()}D")
    if not x.is_contiguous() or not v.is_contiguous():
        raise ValueError("clip_step_: x and v must be contiguous")
    P, n = x.shape
    if not 1 <= P <= 64:
        raise ValueError(f"clip_step_ supports 1 <= P <= 64, got {P}")
    if n % 4 != 0:
        raise ValueError(f"clip_step_: row length must be a multiple of 4, got {n}")
    if v.shape != (n,):
        raise ValueError(f"clip_step_: v must have shape ({n},), got {tuple(v.shape)}")
    if w.shape != (P,):
        raise ValueError(f"clip_step_: w must have shape ({P},), got {tuple(w.shape)}")
    if v.device != x.device or w.device != x.device:
        raise ValueError("clip_step_: v and w must be on x's device")
    used = [p for p in range(P) if float(w[p]) != 0.0]
    if used and n > 0:
        delta = torch.zeros_like(v)
        for p in used:
            delta = delta + (x[p] - v) * w[p]
        v += delta
    if not dist:
        return None
    dev = x - v
    return (dev * dev).sum(dim=1)


# --------------------------------------------------------------------- worker momentum
@torch.no_grad()
def worker_momentum_(g: torch.Tensor, m: torch.Tensor, beta: float, first: bool) -> None:
    """Worker-side momentum (arXiv:2012.10333), in place on one worker's gradient g and
    its private state m: the worker sends its momentum instead of its gradient.

    g, m: 1-D fp32 contiguous, equal length, length % 4 == 0 (a [lo, hi) slice of a
    payload row and the same slice of the state row qualify); 0 <= beta < 1.  Per
    element, in fp32:
      first (the worker's first step):  m = g bit for bit, g is sent as it is.  This is
          the project's choice, the same as FlatSGD's first step (buf = grad): the
          paper's m_0 = 0 would scale the first sent row by (1 - beta).
      later steps:  m = beta*m + (1-beta)*g, then g = m.  (1-beta) is formed in double
          and then cast, as in fused_adam_step.
      non-finite g (NaN, +-Inf), any step:  m keeps its value (0 on the first step) and
          g is sent as it is, so the rule and the nan-guard see the non-finite value in
          this step and the state stays clean for the next.
    The HIP kernel contracts the update into one FMA; here it is two products and an
    add.  They agree within the rounding bound (tests/worker_momentum_util.py), not
    bit for bit; the first step and the non-finite branches agree bit for bit.
    """
    if g.dtype != torch.float32 or m.dtype != torch.float32:
        raise ValueError(f"worker_momentum_: g and m must be fp32, got {g.dtype}, {m.dtype}")
    if not g.is_contiguous() or not m.is_contiguous():
        raise ValueError("worker_momentum_: g and m must be contiguous")
    if g.device != m.device:
        raise ValueError("worker_momentum_: m must be on g's device")
    if m.numel() != g.numel():
        raise ValueError(f"worker_momentum_: m must have g's length, got {m.numel()} "
                         f"and {g.numel()}")
    if g.numel() % 4 != 0:
        raise ValueError(f"worker_momentum_: length must be a multiple of 4, got {g.numel()}")
    beta = float(beta)
    if not 0.0 <= beta < 1.0:
        raise ValueError(f"worker_momentum_: beta must be in [0, 1), got {beta}")
    if g.numel() == 0:
        return
    g1, m1 = g.view(-1), m.view(-1)
    fin = torch.isfinite(g1)
    if first:
        m1.copy_(torch.where(fin, g1, torch.zeros_like(g1)))
        return
    # two rounded products and a rounded add, never an axpy: whether add_(alpha=) fuses
    # differs between the vector body and the tail of a CPU loop, and a slice of a row
    # must give the bits the whole row gives (bucketed == whole-row)
    upd = (m1 * beta).add_(g1 * (1.0 - beta))
    m1.copy_(torch.where(fin, upd, m1))
    g1.copy_(torch.where(fin, upd, g1))


# --------------------------------------------------------------------- vote
@torch.no_grad()
def rows_equal(x: torch.Tensor, a_idx: torch.Tensor, b_idx: torch.Tensor, atol: float) -> torch.Tensor:
    """Per-pair equality of rows of x over the local shard.

    x: (m, d) fp32; a_idx/b_idx: (k,) int64.  Returns (k,) uint8 — 1 iff
    max|x[a]-x[b]| <= atol over d (atol=0 -> bitwise-identical semantics of the
    reference's np.array_equal vote).
    """
    if x.shape[1] == 0:
        return torch.ones(len(a_idx), dtype=torch.uint8, device=x.device)
    diff = (x[a_idx] - x[b_idx]).abs().amax(dim=1)
    return (diff <= atol).to(torch.uint8)


def _absmax_nonfinite_inf(v: torch.Tensor, dim: int) -> torch.Tensor:
    """max|v| along dim under the vote statistics' non-finite rule: any NaN, +Inf or
    -Inf element (Inf - Inf = NaN included) makes the result exactly +inf, so a
    non-finite member is never "equal" to anyone and the value survives a cross-rank
    MAX allreduce (NaN ordering there is unspecified; +inf's is not)."""
    a = v.abs()
    a = torch.where(torch.isnan(a), torch.full_like(a, float("inf")), a)
    return a.amax(dim=dim).float()


@torch.no_grad()
def pair_maxdiff(x: torch.Tensor, a_idx: torch.Tensor, b_idx: torch.Tensor) -> torch.Tensor:
    """Per-pair max|x[a]-x[b]| over the local shard.  (k,) fp32; +inf if any element
    of the difference is non-finite."""
    if x.shape[1] == 0:
        return torch.zeros(len(a_idx), dtype=torch.float32, device=x.device)
    return _absmax_nonfinite_inf(x[a_idx] - x[b_idx], 1)


@torch.no_grad()
def row_absmax(x: torch.Tensor) -> torch.Tensor:
    """Per-row max|x| over the local shard.  (m,) fp32; +inf if any element is
    non-finite."""
    if x.shape[1] == 0:
        return torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
    return _absmax_nonfinite_inf(x, 1)


@torch.no_grad()
def mean_rows(x: torch.Tensor, idx: torch.Tensor, out: torch.Tensor) -> None:
    """out = mean over selected rows of x.  x: (m, d), idx: (k,), out: (d,)."""
    torch.mean(x[idx], dim=0, out=out)


@torch.no_grad()
def sum_rows(x: torch.Tensor, out: torch.Tensor) -> None:
    torch.sum(x, dim=0, out=out)


# --------------------------------------------------------------------- cyclic code
@torch.no_grad()
def cyclic_encode(grads: torch.Tensor, w_re: torch.Tensor, w_im: torch.Tensor, out: torch.Tensor) -> None:
    """out[0] = sum_k w_re[k]*grads[k];  out[1] = sum_k w_im[k]*grads[k].

    grads: (k, d) fp32 (the 2s+1 sub-batch gradients, band order); w_*: (k,);
    out: (2, d) fp32 planes of the encoded complex gradient.
    """
    torch.sum(grads * w_re[:, None], dim=0, out=out[0])
    torch.sum(grads * w_im[:, None], dim=0, out=out[1])


@torch.no_grad()
def cyclic_project(rows: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """Partial per-row projection proj_r = sum_d rows[r, d] * z[d] over the shard.

    rows: (m, d_shard) fp32; z: (d_shard,) fp32 -> (m,) fp32 partials
    (to be summed across ranks).
    """
    if rows.shape[1] == 0:
        return torch.zeros(rows.shape[0], dtype=torch.float32, device=rows.device)
    return rows @ z


@torch.no_grad()
def combine_rows(x: torch.Tensor, rows: torch.Tensor, w: torch.Tensor, out: torch.Tensor) -> None:
    """out = sum_i w[i] * x[rows[i]] — the generic weighted row combination behind
    winner-mean, cyclic encode/recombine and plain summing."""
    if x.shape[1] == 0:
        out.zero_()
        return
    out.copy_((w @ x[rows]).reshape(-1))


@torch.no_grad()
def combine_rows_slice(x: torch.Tensor, rows: torch.Tensor, w: torch.Tensor,
                       out: torch.Tensor, col_off: int) -> None:
    """Column-range variant for the bucketed cyclic encode: identical per-element
    arithmetic to combine_rows restricted to [col_off, col_off + len(out))."""
    n = out.numel()
    if n == 0:
        return
    out.copy_((w @ x[rows][:, col_off : col_off + n]).reshape(-1))


@torch.no_grad()
def cyclic_recombine(r_planes: torch.Tensor, v_re: torch.Tensor, v_im: torch.Tensor, out: torch.Tensor) -> None:
    """out = Re( v @ R ) over the local shard.

    Re(v_i * (re + i*im)) = v_re*re - v_im*im summed over rows i.
    r_planes: (n, 2, d_shard); v_*: (n,); out: (d_shard,).
    """
    re = torch.einsum("nd,n->d", r_planes[:, 0, :], v_re)
    im = torch.einsum("nd,n->d", r_planes[:, 1, :], v_im)
    torch.sub(re, im, out=out)


# --------------------------------------------------------------------- geo-median
@torch.no_grad()
def segment_absmax(x: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
    """(rows, d), (L+1,) bounds -> (rows, L) per-segment max|x| (segment vote); a
    cell is +inf if its segment holds any non-finite element."""
    L = seg.numel() - 1
    out = torch.zeros(x.shape[0], L, dtype=torch.float32, device=x.device)
    for l in range(L):
        lo, hi = int(seg[l]), int(seg[l + 1])
        if hi > lo:
            out[:, l] = _absmax_nonfinite_inf(x[:, lo:hi], 1)
    return out


def segment_pair_maxdiff(x: torch.Tensor, a_idx: torch.Tensor, b_idx: torch.Tensor,
                         seg: torch.Tensor) -> torch.Tensor:
    """(pairs, L) per-segment max|x[a]-x[b]| (segment-granular tolerance vote)."""
    return segment_absmax(x[a_idx] - x[b_idx], seg)


def segment_sqdist(x: torch.Tensor, z: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
    """Per-(row, segment) partial squared distance ||x[p, seg_l] - z[seg_l]||^2.

    x: (P, d_shard), z: (d_shard,), seg: (L+1,) int64 local segment bounds.
    Returns (P, L) fp32 partials.
    """
    P = x.shape[0]
    L = len(seg) - 1
    out = torch.zeros(P, L, dtype=torch.float32, device=x.device)
    d2 = (x - z[None, :]).pow(2)
    for l in range(L):
        lo, hi = int(seg[l]), int(seg[l + 1])
        if hi > lo:
            out[:, l] = d2[:, lo:hi].sum(dim=1)
    return out


@torch.no_grad()
def segment_weighted_mean(x: torch.Tensor, w: torch.Tensor, seg: torch.Tensor, out: torch.Tensor) -> None:
    """out[seg_l] = sum_p w[p, l] * x[p, seg_l]  (weights pre-normalised per segment).

    x: (P, d_shard); w: (P, L); seg: (L+1,); out: (d_shard,).
    """
    L = len(seg) - 1
    for l in range(L):
        lo, hi = int(seg[l]), int(seg[l + 1])
        if hi > lo:
            out[lo:hi] = w[:, l] @ x[:, lo:hi]


@torch.no_grad()
def segment_gram(x: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
    """Per-segment Gram matrices G[l] = X_l @ X_l^T (for Krum's distance matrix).

    x: (P, d_shard); seg: (L+1,).  Returns (L, P, P) fp32 partials.
    """
    P = x.shape[0]
    L = len(seg) - 1
    out = torch.zeros(L, P, P, dtype=torch.float32, device=x.device)
    for l in range(L):
        lo, hi = int(seg[l]), int(seg[l + 1])
        if hi > lo:
            xs = x[:, lo:hi]
            out[l] = xs @ xs.T
    return out


# --------------------------------------------------------------------- trimmed mean
@torch.no_grad()
def column_trimmed_mean(x: torch.Tensor, lo: int, hi: int, out: torch.Tensor) -> None:
    """out[j] = mean of ranks [lo, hi) of column j of x (coordinate-wise median /
    beta-trimmed mean, arXiv:1803.01498).

    x: (P, d) fp32; out: (d,); 0 <= lo < hi <= P.  Per column: NaN -> +inf (the vote
    statistics' rule: a NaN is an extreme value that gets trimmed), ascending sort,
    then the kept ranks are added ONE AT A TIME in ascending order and divided by
    float32(hi - lo).  The HIP kernel performs the same fp32 operations in the same
    order, so the two agree bit for bit (torch.sum/mean have an unspecified order).
    """
    P = x.shape[0]
    if not 0 <= lo < hi <= P:
        raise ValueError(f"column_trimmed_mean needs 0 <= lo < hi <= P, got lo={lo} hi={hi} P={P}")
    if out.numel() != x.shape[1]:
        raise ValueError("column_trimmed_mean: out must have the length of a row of x")
    if x.shape[1] == 0:
        return
    a = torch.where(torch.isnan(x), torch.full_like(x, float("inf")), x)
    s, _ = torch.sort(a, dim=0)
    acc = s[lo].clone()
    for k in range(lo + 1, hi):
        acc = acc + s[k]
    # tensor divisor: an elementwise IEEE division (never a multiply by 1/k)
    torch.div(acc, torch.full_like(acc, float(hi - lo)), out=out)


# --------------------------------------------------------------------- mean around
@torch.no_grad()
def mean_around_window(x: torch.Tensor, keep: int, clo: int, chi: int):
    """Steps 1-3 of column_mean_around: (s, c, w) = the sorted columns, the centre and
    the start of the kept window of every column (exposed so tests can see which
    windows a data set exercises)."""
    P = x.shape[0]
    if not 1 <= keep <= P:
        raise ValueError(f"column_mean_around needs 1 <= keep <= P, got keep={keep} P={P}")
    if not 0 <= clo < chi <= P:
        raise ValueError(
            f"column_mean_around needs 0 <= clo < chi <= P, got clo={clo} chi={chi} P={P}")
    a = torch.where(torch.isnan(x), torch.full_like(x, float("inf")), x)
    s, _ = torch.sort(a, dim=0)
    c = s[clo].clone()
    for k in range(clo + 1, chi):
        c = c + s[k]
    # tensor divisor: an elementwise IEEE division (never a multiply by 1/k)
    c = torch.div(c, torch.full_like(c, float(chi - clo)))
    b = P - keep
    if b > 0:
        w = ((c - s[:b]) > (s[keep:] - c)).sum(dim=0)
    else:
        w = torch.zeros(x.shape[1], dtype=torch.long, device=x.device)
    return s, c, w


@torch.no_grad()
def column_mean_around(x: torch.Tensor, keep: int, clo: int, chi: int,
                       out: torch.Tensor) -> None:
    """out[j] = mean of the `keep` values of column j nearest to a robust centre c
    (mean around median, arXiv:1802.10116; Phocas, arXiv:1805.09682).

    x: (P, d) fp32; out: (d,); 1 <= keep <= P; 0 <= clo < chi <= P; b = P - keep.
    Per column:
      1. NaN -> +inf, ascending sort into s[0..P)            (column_trimmed_mean's step)
      2. c = column_trimmed_mean(x, clo, chi): ranks [clo, chi) added one at a time,
         divided by float32(chi - clo).  Median: ((P-1)//2, P//2+1); trimmed mean: (b, P-b)
      3. w = #{ j in [0, b) : (c - s[j]) > (s[j + keep] - c) } -- plain fp32, strict >,
         a NaN comparison is false.  The predicate is monotone in j, and w is where
         dropping, b times, whichever end is farther from c (a tie drops the top)
         arrives: s[w, w+keep) holds the keep smallest distances to c
      4. out = ranks [w, w+keep) added one at a time ascending / float32(keep)
    The HIP kernel performs the same fp32 operations in the same order: bit-identical.

    With at most b corrupted rows and P > 2b, c lies inside the honest [min, max] and
    |out - c| <= max over honest h of |h - c| (the radius guarantee).  The output itself
    is NOT confined to the honest [min, max]: a corrupted value just outside it can be
    nearer to c than a far honest one.  With at most b non-finite rows the window holds
    finite values only; with more the result may be inf/NaN.
    """
    s, _, w = mean_around_window(x, keep, clo, chi)
    if out.numel() != x.shape[1]:
        raise ValueError("column_mean_around: out must have the length of a row of x")
    if x.shape[1] == 0:
        return
    idx = w.unsqueeze(0) + torch.arange(keep, device=x.device).unsqueeze(1)
    win = torch.gather(s, 0, idx)
    acc = win[0].clone()
    for k in range(1, keep):
        acc = acc + win[k]
    torch.div(acc, torch.full_like(acc, float(keep)), out=out)


# --------------------------------------------------------------------- segment mean around
@torch.no_grad()
def segment_mean_around(x: torch.Tensor, sel: torch.Tensor, seg: torch.Tensor, keep: int,
                        clo: int, chi: int, out: torch.Tensor) -> None:
    """column_mean_around over a per-segment row selection (Multi-Krum / Bulyan decode).

    x: (P, d) fp32; sel: (L, T) int64 row indices into x, distinct within a row;
    seg: (L+1,) non-decreasing local segment bounds (zero-length segments, seg[0] > 0
    and seg[L] < d are legal); out: (d,).  1 <= T <= P; keep, clo, chi relative to T.
    For column j of segment l, out[j] = column_mean_around of the T values
    x[sel[l, k], j] (the order of sel[l] cannot matter: they are sorted); columns
    outside [seg[0], seg[L]) get +0.0, so every element of out is written.  A row that
    is not selected for a segment is never read there: a NaN in it cannot reach out.
    Indices are clamped into [0, P), as in the HIP kernel, which performs the same fp32
    operations in the same order: bit-identical.
    """
    P, d = x.shape
    L = seg.numel() - 1
    if sel.dim() != 2 or sel.shape[0] != L:
        raise ValueError(f"segment_mean_around: sel must be (L, T) with L={L}, "
                         f"got {tuple(sel.shape)}")
    T = sel.shape[1]
    if not 1 <= T <= P:
        raise ValueError(f"segment_mean_around needs 1 <= T <= P, got T={T} P={P}")
    if not 1 <= keep <= T:
        raise ValueError(f"segment_mean_around needs 1 <= keep <= T, got keep={keep} T={T}")
    if not 0 <= clo < chi <= T:
        raise ValueError(
            f"segment_mean_around needs 0 <= clo < chi <= T, got clo={clo} chi={chi} T={T}")
    if out.numel() != d:
        raise ValueError("segment_mean_around: out must have the length of a row of x")
    if d == 0:
        return
    out.zero_()
    rows = sel.clamp(0, P - 1)
    for l in range(L):
        lo, hi = int(seg[l]), int(seg[l + 1])
        if hi > lo:
            column_mean_around(x[rows[l]][:, lo:hi], keep, clo, chi, out[lo:hi])


# --------------------------------------------------------------------- dtype cast
@torch.no_grad()
def cast_to_bf16(x: torch.Tensor, out: torch.Tensor) -> None:
    out.copy_(x)


@torch.no_grad()
def cast_from_bf16(x: torch.Tensor, out: torch.Tensor) -> None:
    out.copy_(x)
