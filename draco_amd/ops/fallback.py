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


# --------------------------------------------------------------------- row mixing
@torch.no_grad()
def mix_rows_(x: torch.Tensor, w: torch.Tensor, skip=()) -> None:
    """Y = W X in place on the (P, n) block with the rows in `skip` left out of the sum:
    y[i, c] = sum over k not in skip of w[i, k] * x[k, c].  The heavy half of
    nearest-neighbour mixing (arXiv:2302.01772; parallel/mixing.py builds W).

    x: (P, n) fp32 contiguous, P <= 32, n % 4 == 0; w: (P, P) fp32 contiguous on x's
    device, dense (not assumed 0/1 or symmetric), never read on the host; skip: distinct
    ints in [0, P).  A skipped row is removed by selection, not multiplied by zero: its
    NaN/Inf values reach no output, whatever w holds in its column.  It is still WRITTEN
    like every other row.  With every row skipped the result is zero.  Other non-finite
    values propagate by ordinary IEEE arithmetic (a NaN row of w gives a NaN row of y).
    The HIP kernel sums in the matrix unit's order: it agrees within the rounding bound
    2*(P+4)*2^-24 * sum_k |w[i,k] x[k,c]|, not bit for bit.
    """
    if x.dtype != torch.float32 or w.dtype != torch.float32:
        raise ValueError(f"mix_rows_: x and w must be fp32, got {x.dtype}, {w.dtype}")
    if x.dim() != 2:
        raise ValueError(f"mix_rows_: x must be 2D, got {x.dim()}D")
    if not x.is_contiguous() or not w.is_contiguous():
        raise ValueError("mix_rows_: x and w must be contiguous")
    P, n = x.shape
    if P > 32:
        raise ValueError(f"mix_rows_ supports P <= 32, got {P}")
    if n % 4 != 0:
        raise ValueError(f"mix_rows_: row length must be a multiple of 4, got {n}")
    if w.shape != (P, P):
        raise ValueError(f"mix_rows_: w must have shape ({P}, {P}), got {tuple(w.shape)}")
    if w.device != x.device:
        raise ValueError("mix_rows_: w must be on x's device")
    skip = [int(r) for r in skip]
    for r in skip:
        if not 0 <= r < P:
            raise ValueError(f"mix_rows_: skip row {r} outside [0, {P})")
    if len(set(skip)) != len(skip):
        raise ValueError(f"mix_rows_: skip rows must be distinct, got {skip}")
    if P == 0 or n == 0:
        return
    keep = [k for k in range(P) if k not in set(skip)]
    if not keep:
        x.zero_()
        return
    x.copy_(torch.mm(w[:, keep], x[keep]))


# --------------------------------------------------------------------- sign majority
def _check_sign(op: str, vals: torch.Tensor, bits: torch.Tensor, n: int) -> None:
    if vals.dtype != torch.float32:
        raise ValueError(f"{op}: values must be fp32, got {vals.dtype}")
    if bits.dtype != torch.int32:
        raise ValueError(f"{op}: packed signs must be int32, got {bits.dtype}")
    if not vals.is_contiguous() or not bits.is_contiguous():
        raise ValueError(f"{op}: tensors must be contiguous")
    if vals.device != bits.device:
        raise ValueError(f"{op}: tensors must be on one device")
    if vals.dim() != 1 or n % 64 != 0:
        raise ValueError(f"{op}: values must be 1D with a length that is a multiple of 64, "
                         f"got shape {tuple(vals.shape)}")


@torch.no_grad()
def sign_pack(g: torch.Tensor, out: torch.Tensor) -> None:
    """The signSGD wire format (arXiv:1810.05291): out = the votes of g, two bits each.

    g: (n,) fp32 contiguous, n % 64 == 0; out: (n/16,) int32 on g's device.  The vote of a
    value is +1 (g > 0), -1 (g < 0) or 0 (+0.0, -0.0 and NaN abstain); +-Inf and
    subnormals vote their sign.  It is read off the bit pattern, so no float compare can
    flush a subnormal.  Elements [64r, 64r + 64) form record r = words 4r..4r+3:
    (neg bits 0..31, neg bits 32..63, pos bits 0..31, pos bits 32..63), element 4l + c of
    the record (l < 16, c < 4) at bit 16c + l of its plane: the layout documented above
    k_sign_pack in draco_kernels.hip, which writes the same bytes.  A 64-aligned slice of
    g packs to the matching slice of out.
    """
    n = g.numel()
    _check_sign("sign_pack", g, out, n)
    if out.dim() != 1 or out.numel() != n // 16:
        raise ValueError(f"sign_pack: out must be 1D of length {n // 16}, got "
                         f"{tuple(out.shape)}")
    if n == 0:
        return
    u = g.view(torch.int32)
    a = u & 0x7FFFFFFF
    votes = (a != 0) & (a <= 0x7F800000)
    planes = torch.stack([votes & (u < 0), votes & (u >= 0)])  # (neg, pos) x (n,)
    # (plane, R, l, c) -> (R, plane, c, l): bit 16c + l, 32 bits per word
    bits = planes.view(2, -1, 16, 4).permute(1, 0, 3, 2).reshape(-1, 32).to(torch.int64)
    words = (bits << torch.arange(32, device=g.device)).sum(dim=1)
    out.copy_(torch.where(words >= 2 ** 31, words - 2 ** 32, words))


@torch.no_grad()
def sign_majority(packed: torch.Tensor, out: torch.Tensor) -> None:
    """out[j] = sign(#pos_j - #neg_j) over the P packed rows: +1.0, -1.0 or +0.0 (ties,
    all-abstain columns and the zero pad tail), always finite.

    packed: (P, n/16) int32 contiguous, rows in sign_pack's format, P <= 64; out: (n,)
    fp32 on its device, n % 64 == 0.  A row counts at most once per coordinate whatever
    its bits are: one with both bits of an element set adds one to each side and so
    abstains.  n == 0 or P == 0 returns at once (with P == 0, out is left as it is).
    """
    n = out.numel()
    _check_sign("sign_majority", out, packed, n)
    if packed.dim() != 2 or packed.shape[1] != n // 16:
        raise ValueError(f"sign_majority: packed must be (P, {n // 16}), got "
                         f"{tuple(packed.shape)}")
    P = packed.shape[0]
    if P > 64:
        raise ValueError(f"sign_majority supports P <= 64, got {P}")
    if n == 0 or P == 0:
        return
    shifts = torch.arange(32, device=packed.device, dtype=torch.int32)
    bits = (packed.view(P, -1, 2, 2, 1) >> shifts) & 1  # (P, R, plane, word, bit)
    # bit 16c + l of a plane -> element 4l + c of the record
    count = bits.view(P, -1, 2, 4, 16).sum(dim=0, dtype=torch.int32)  # (R, plane, c, l)
    diff = (count[:, 1] - count[:, 0]).transpose(1, 2).reshape(-1)  # (R, l, c) -> (n,)
    out.copy_(torch.sign(diff))


# --------------------------------------------------------------------- mx8 wire
def mx8_chunk_bytes(chunk: int) -> int:
    """Bytes of one packed record: chunk codes, chunk/32 scales, zero padding to 16."""
    return chunk + (chunk // 32 + 15) // 16 * 16


def _check_mx8(op: str, vals: torch.Tensor, data: torch.Tensor, chunk: int, records: int,
               chunk_bytes=mx8_chunk_bytes) -> None:
    if vals.dtype != torch.float32:
        raise ValueError(f"{op}: values must be fp32, got {vals.dtype}")
    if data.dtype != torch.uint8:
        raise ValueError(f"{op}: packed data must be uint8, got {data.dtype}")
    if not vals.is_contiguous() or not data.is_contiguous():
        raise ValueError(f"{op}: tensors must be contiguous")
    if vals.device != data.device:
        raise ValueError(f"{op}: tensors must be on one device")
    if chunk < 0 or chunk % 64 != 0:
        raise ValueError(f"{op}: chunk must be a multiple of 64, got {chunk}")
    if vals.numel() != records * chunk:
        raise ValueError(f"{op}: values must hold {records} x {chunk} elements, got "
                         f"{vals.numel()}")
    if data.numel() != records * chunk_bytes(chunk):
        raise ValueError(f"{op}: packed data must hold {records} records of "
                         f"{chunk_bytes(chunk)} bytes, got {data.numel()}")


@torch.no_grad()
def mx8_pack(g: torch.Tensor, out: torch.Tensor, chunk: int) -> None:
    """The MXFP8 wire (E4M3 codes, one E8M0 scale per 32 elements): out = the n / chunk
    packed records of g.  g: (n,) fp32, n % chunk == 0, chunk % 64 == 0; out:
    (n / chunk * mx8_chunk_bytes(chunk),) uint8.  The format is described once, above
    k_mx8_pack in draco_kernels.hip; this is its executable definition, in integer
    arithmetic on the fp32 bit patterns, and the kernel writes the same bytes."""
    n = g.numel()
    if g.dim() != 1 or out.dim() != 1:
        raise ValueError("mx8_pack: g and out must be 1D")
    if (n % chunk != 0) if chunk > 0 else (n != 0):
        raise ValueError(f"mx8_pack: length {n} is not a multiple of chunk {chunk}")
    records = n // chunk if chunk > 0 else 0
    _check_mx8("mx8_pack", g, out, chunk, records)
    if n == 0:
        return
    u = g.view(torch.int32).to(torch.int64)
    a, sign = u & 0x7FFFFFFF, (u >> 24) & 0x80
    fin = a < 0x7F800000
    amax = torch.where(fin, a, torch.zeros_like(a)).view(-1, 32).amax(dim=1)
    # s = e + 127 with e = exponent(amax) - 8, plus 1 past 1.75 * 2^exponent; e >= -117
    s = ((amax >> 23) - 8 + ((amax & 0x7FFFFF) > 0x600000)).clamp_(min=10)
    ex, m = a >> 23, a & 0x7FFFFF
    m = torch.where(ex > 0, m | 0x800000, m)  # the 24-bit significand; subnormals have ex = 1
    q = ex.clamp(min=1) - s.repeat_interleave(32)  # exponent of x / 2^e
    # normal codes keep 4 significand bits (drop 20); below 2^-6 the codes step by 2^-9
    sh = (20 + (-6 - q).clamp(min=0)).clamp(max=31)
    r = (m + (torch.ones_like(sh) << (sh - 1)) - 1 + ((m >> sh) & 1)) >> sh  # nearest, ties to even
    code = ((q + 6).clamp(min=0) << 3) + r  # r = 16 carries into the exponent field
    code = torch.where(fin, code, torch.full_like(code, 0x7F)) | sign
    rec = out.view(records, -1)
    rec[:, :chunk] = code.view(records, chunk).to(torch.uint8)
    rec[:, chunk: chunk + chunk // 32] = s.view(records, -1).to(torch.uint8)
    rec[:, chunk + chunk // 32:] = 0


@torch.no_grad()
def mx8_unpack(packed: torch.Tensor, out: torch.Tensor) -> None:
    """out (P, chunk) fp32 = the decoded rows of packed (P, mx8_chunk_bytes(chunk)) uint8 in
    mx8_pack's format.  Any bytes decode: a scale byte below 10 counts as 10, 0xFF makes the
    block NaN, an overflowing product is +-Inf.  P == 0 or chunk == 0 returns at once."""
    if packed.dim() != 2 or out.dim() != 2 or packed.shape[0] != out.shape[0]:
        raise ValueError("mx8_unpack: packed must be (P, chunk_bytes) and out (P, chunk)")
    P, chunk = out.shape
    _check_mx8("mx8_unpack", out, packed, chunk, P)
    if P == 0 or chunk == 0:
        return
    c = torch.arange(256, device=out.device)
    e, m = (c >> 3) & 15, (c & 7).float()
    table = torch.where(e > 0, torch.ldexp(1.0 + m / 8.0, e - 7), m * 2.0 ** -9)
    table = torch.where((c & 0x7F) == 0x7F, torch.full_like(table, float("nan")), table)
    table = torch.where(c >= 128, -table, table)
    s = packed[:, chunk: chunk + chunk // 32].to(torch.int32)
    scale = (s.clamp(min=10) << 23).view(torch.float32)  # 2^(s-127), a normal fp32 number
    scale = torch.where(s == 0xFF, torch.full_like(scale, float("nan")), scale)
    out.copy_(table[packed[:, :chunk].long()] * scale.repeat_interleave(32, dim=1))


# --------------------------------------------------------------------- mx4 wire
def mx4_chunk_bytes(chunk: int) -> int:
    """Bytes of one packed record: chunk/2 code bytes, chunk/32 scales, zero padding to 16."""
    return chunk // 2 + (chunk // 32 + 15) // 16 * 16


def _mx4_hash(a: torch.Tensor) -> torch.Tensor:
    """h of the mx4 format on int64 tensors holding 32-bit values (products wrap mod 2^64,
    which keeps the low 32 bits)."""
    a = a ^ (a >> 16)
    a = (a * 0x7FEB352D) & 0xFFFFFFFF
    a = a ^ (a >> 15)
    a = (a * 0x846CA68B) & 0xFFFFFFFF
    return a ^ (a >> 16)


@torch.no_grad()
def mx4_pack(g: torch.Tensor, out: torch.Tensor, chunk: int, seed=None) -> None:
    """The MXFP4 wire (E2M1 nibbles, one E8M0 scale per 32 elements): out = the n / chunk
    packed records of g.  g: (n,) fp32, n % chunk == 0, chunk % 64 == 0; out:
    (n / chunk * mx4_chunk_bytes(chunk),) uint8.  seed=None rounds to nearest (ties to the
    even code); an int seed rounds stochastically, unbiased per element, with the 24 random
    bits of element i a stateless hash of (seed mod 2^64, i).  The format is described once,
    above k_mx4_pack in draco_kernels.hip; this is its executable definition, in integer
    arithmetic on the fp32 bit patterns, and the kernel writes the same bytes."""
    n = g.numel()
    if g.dim() != 1 or out.dim() != 1:
        raise ValueError("mx4_pack: g and out must be 1D")
    if (n % chunk != 0) if chunk > 0 else (n != 0):
        raise ValueError(f"mx4_pack: length {n} is not a multiple of chunk {chunk}")
    records = n // chunk if chunk > 0 else 0
    _check_mx8("mx4_pack", g, out, chunk, records, mx4_chunk_bytes)
    if n == 0:
        return
    u = g.view(torch.int32).to(torch.int64)
    a, sign = u & 0x7FFFFFFF, (u >> 28) & 8
    fin = a < 0x7F800000
    a = torch.where(fin, a, torch.zeros_like(a))  # a non-finite element: code 0 with its sign
    amax = a.view(-1, 32).amax(dim=1)
    # s = e + 127 with e = exponent(amax) - 2, plus 1 past 1.5 * 2^exponent; e >= -125
    s = ((amax >> 23) - 2 + ((amax & 0x7FFFFF) > 0x400000)).clamp_(min=2)
    ex, m = a >> 23, a & 0x7FFFFF
    m = torch.where(ex > 0, m | 0x800000, m)  # the 24-bit significand M; subnormals have ex = 1
    q = ex.clamp(min=1) - s.repeat_interleave(32)  # t = M * 2^(q-23), q <= 2
    sh = 22 - q.clamp(max=0)  # t / step = M / 2^sh: step 0.5 below 2, then 1, then 2
    shc = sh.clamp(max=31)  # M < 2^24: past 24 the quotient is 0 and the remainder M
    frac = m & ((torch.ones_like(shc) << shc) - 1)
    code = (m >> shc) + 2 * q.clamp(min=0)  # lo's code; hi's is the next one
    if seed is None:
        half = torch.ones_like(shc) << (shc - 1)
        up = (frac > half) | ((frac == half) & ((code & 1) == 1))
    else:
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        hi_word = torch.tensor(((seed >> 32) + 0x9E3779B9) & 0xFFFFFFFF, device=g.device)
        key = _mx4_hash((seed & 0xFFFFFFFF) ^ _mx4_hash(hi_word))
        i = torch.arange(n, device=g.device) & 0xFFFFFFFF
        r = _mx4_hash(i ^ key) >> 8
        # up iff r < frac * 2^24 / 2^sh, in integers on either side of sh = 24
        d = (sh - 24).clamp(min=0, max=24)
        thr = torch.where(sh <= 24, frac << (24 - sh).clamp(min=0),
                          (frac + (torch.ones_like(d) << d) - 1) >> d)
        tiny = (sh > 125) & ((m >> (sh - 125).clamp(min=0, max=31)) == 0)  # t < 2^-126
        up = (r < thr) & ~tiny
    code = (code + up) | sign
    bad = (~fin).view(-1, 32).any(dim=1)
    s = torch.where(bad, torch.full_like(s, 0xFF), s)
    rec = out.view(records, -1)
    code = code.view(records, chunk // 2, 2)
    rec[:, : chunk // 2] = (code[:, :, 0] | (code[:, :, 1] << 4)).to(torch.uint8)
    rec[:, chunk // 2: chunk // 2 + chunk // 32] = s.view(records, -1).to(torch.uint8)
    rec[:, chunk // 2 + chunk // 32:] = 0


@torch.no_grad()
def mx4_unpack(packed: torch.Tensor, out: torch.Tensor) -> None:
    """out (P, chunk) fp32 = the decoded rows of packed (P, mx4_chunk_bytes(chunk)) uint8 in
    mx4_pack's format.  Any bytes decode: a scale byte below 2 counts as 2, 0xFF makes the
    block NaN, an overflowing product is +-Inf.  P == 0 or chunk == 0 returns at once."""
    if packed.dim() != 2 or out.dim() != 2 or packed.shape[0] != out.shape[0]:
        raise ValueError("mx4_unpack: packed must be (P, chunk_bytes) and out (P, chunk)")
    P, chunk = out.shape
    _check_mx8("mx4_unpack", out, packed, chunk, P, mx4_chunk_bytes)
    if P == 0 or chunk == 0:
        return
    table = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], device=out.device)
    table = torch.cat([table, -table])
    b = packed[:, : chunk // 2].long()
    codes = torch.stack([b & 15, b >> 4], dim=2).view(P, chunk)  # element 2k: the low nibble
    s = packed[:, chunk // 2: chunk // 2 + chunk // 32].to(torch.int32)
    scale = (s.clamp(min=2) << 23).view(torch.float32)  # 2^(s-127), a normal fp32 number
    scale = torch.where(s == 0xFF, torch.full_like(scale, float("nan")), scale)
    out.copy_(table[codes] * scale.repeat_interleave(32, dim=1))


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


# --------------------------------------------------------------------- mx8 column rules
def _mx8_decoded(op: str, packed: torch.Tensor, out: torch.Tensor, chunk_bytes=mx8_chunk_bytes,
                 unpack=mx8_unpack):
    """The checks of the ops below and the decoded (P, chunk) block.  The format is
    mx8_unpack's (mx4_unpack's for the mx4 ops): it has no second statement here."""
    if out.dtype != torch.float32:
        raise ValueError(f"{op}: out must be fp32, got {out.dtype}")
    if not out.is_contiguous():
        raise ValueError(f"{op}: out must be contiguous")
    chunk = out.numel()
    if packed.dim() != 2 or packed.shape[1] != chunk_bytes(chunk):
        raise ValueError(f"{op}: packed must be (P, {chunk_bytes(chunk)}) for chunk {chunk}")
    if not 1 <= packed.shape[0] <= 64:
        raise ValueError(f"{op} supports 1 <= P <= 64, got {packed.shape[0]}")
    x = torch.empty(packed.shape[0], chunk, dtype=torch.float32, device=out.device)
    unpack(packed, x)  # dtype, device, contiguity of packed, chunk % 64
    return x


@torch.no_grad()
def mx8_column_trimmed_mean(packed: torch.Tensor, lo: int, hi: int, out: torch.Tensor) -> None:
    """out (chunk,) = column_trimmed_mean of the decoded rows of packed (P,
    mx8_chunk_bytes(chunk)) uint8, 1 <= P <= 64: by definition mx8_unpack into a temporary,
    then column_trimmed_mean.  The HIP kernel gives the same bits from the packed bytes."""
    x = _mx8_decoded("mx8_column_trimmed_mean", packed, out)
    column_trimmed_mean(x, lo, hi, out.view(-1))


@torch.no_grad()
def mx8_column_mean_around(packed: torch.Tensor, keep: int, clo: int, chi: int,
                           out: torch.Tensor) -> None:
    """out (chunk,) = column_mean_around of the decoded rows of packed; as
    mx8_column_trimmed_mean."""
    x = _mx8_decoded("mx8_column_mean_around", packed, out)
    column_mean_around(x, keep, clo, chi, out.view(-1))


# --------------------------------------------------------------------- mx4 column rules
@torch.no_grad()
def mx4_column_trimmed_mean(packed: torch.Tensor, lo: int, hi: int, out: torch.Tensor) -> None:
    """out (chunk,) = column_trimmed_mean of the decoded rows of packed (P,
    mx4_chunk_bytes(chunk)) uint8, 1 <= P <= 64: by definition mx4_unpack into a temporary,
    then column_trimmed_mean.  The HIP kernel gives the same bits from the packed bytes."""
    x = _mx8_decoded("mx4_column_trimmed_mean", packed, out, mx4_chunk_bytes, mx4_unpack)
    column_trimmed_mean(x, lo, hi, out.view(-1))


@torch.no_grad()
def mx4_column_mean_around(packed: torch.Tensor, keep: int, clo: int, chi: int,
                           out: torch.Tensor) -> None:
    """out (chunk,) = column_mean_around of the decoded rows of packed; as
    mx4_column_trimmed_mean."""
    x = _mx8_decoded("mx4_column_mean_around", packed, out, mx4_chunk_bytes, mx4_unpack)
    column_mean_around(x, keep, clo, chi, out.view(-1))


# --------------------------------------------------------------------- mx8 iterative rules
@torch.no_grad()
def mx8_clip_step_(packed: torch.Tensor, v: torch.Tensor, w: torch.Tensor, dist: bool = True):
    """clip_step_ on the decoded rows of packed (P, mx8_chunk_bytes(chunk)) uint8, 1 <= P <=
    64, v (chunk,) fp32 in place: by definition mx8_unpack into a temporary, then clip_step_.
    The HIP kernel reads the records and gives clip_step's v bit for bit."""
    if v.dim() != 1:
        raise ValueError(f"mx8_clip_step_: v must be 1D, got {v.dim()}D")
    x = _mx8_decoded("mx8_clip_step_", packed, v)
    return clip_step_(x, v, w, dist)


@torch.no_grad()
def mx8_weiszfeld_step(packed: torch.Tensor, w, seg: torch.Tensor, z: torch.Tensor,
                       dist: bool = True):
    """One Weiszfeld iteration on the decoded rows of packed (P, mx8_chunk_bytes(chunk)) uint8,
    1 <= P <= 64: by definition mx8_unpack into a temporary, then segment_weighted_mean into z
    (chunk,) with the weights w (P, L) (w None: z is left as it is), then segment_sqdist at
    that z: (P, L), or None with dist=False."""
    if z.dim() != 1:
        raise ValueError(f"mx8_weiszfeld_step: z must be 1D, got {z.dim()}D")
    x = _mx8_decoded("mx8_weiszfeld_step", packed, z)
    P, L = x.shape[0], seg.numel() - 1
    if w is not None:
        if w.dtype != torch.float32 or tuple(w.shape) != (P, L):
            raise ValueError(f"mx8_weiszfeld_step: w must be fp32 of shape ({P}, {L}), got "
                             f"{w.dtype} {tuple(w.shape)}")
        segment_weighted_mean(x, w, seg, z)
    return segment_sqdist(x, z, seg) if dist else None


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


# --------------------------------------------------------------------- mx8 krum rules
def _mx8_chunk_of(op: str, cbytes: int) -> int:
    """The chunk whose packed record has `cbytes` bytes (mx8_chunk_bytes is increasing)."""
    c = max(0, cbytes * 32 // 33 // 64 * 64 - 64)
    while mx8_chunk_bytes(c) < cbytes:
        c += 64
    if mx8_chunk_bytes(c) != cbytes:
        raise ValueError(f"{op}: {cbytes} bytes are no mx8 record of a chunk that is a "
                         f"multiple of 64")
    return c


def _check_krum_rows(op: str, packed: torch.Tensor) -> None:
    if packed.dim() != 2 or not 1 <= packed.shape[0] <= 32:
        raise ValueError(f"{op} supports packed (P, chunk_bytes) with 1 <= P <= 32, got "
                         f"{tuple(packed.shape)}")


@torch.no_grad()
def mx8_segment_gram(packed: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
    """(L, P, P) fp32 = segment_gram of the decoded rows of packed (P, mx8_chunk_bytes(chunk))
    uint8, 1 <= P <= 32 (one 32x32 matrix tile in the HIP kernel): by definition mx8_unpack
    into a temporary, then segment_gram.  The HIP kernel multiplies the records themselves
    with the block-scaled FP8 matrix instruction: every product is exact, only the fp32
    accumulation order differs, and an entry that is non-finite here is non-finite there."""
    _check_krum_rows("mx8_segment_gram", packed)
    chunk = _mx8_chunk_of("mx8_segment_gram", packed.shape[1])
    x = torch.empty(packed.shape[0], chunk, dtype=torch.float32, device=packed.device)
    mx8_unpack(packed, x)
    return segment_gram(x, seg)


@torch.no_grad()
def mx8_segment_mean_around(packed: torch.Tensor, sel: torch.Tensor, seg: torch.Tensor,
                            keep: int, clo: int, chi: int, out: torch.Tensor) -> None:
    """out (chunk,) = segment_mean_around of the decoded rows of packed, 1 <= T <= P <= 32: by
    definition mx8_unpack into a temporary, then segment_mean_around.  The HIP kernel gives
    the same bits from the packed bytes."""
    _check_krum_rows("mx8_segment_mean_around", packed)
    x = _mx8_decoded("mx8_segment_mean_around", packed, out)
    segment_mean_around(x, sel, seg, keep, clo, chi, out.view(-1))


# --------------------------------------------------------------------- gradient sink
def flat_order(t: torch.Tensor, channels_last: bool = False) -> torch.Tensor:
    """The elements of t in the order of the flat space: NHWC for a 4-D tensor of a
    channels-last space, row-major otherwise."""
    if channels_last and t.dim() == 4:
        return t.permute(0, 2, 3, 1).reshape(-1)
    return t.reshape(-1)


def check_scatter_grads(srcs, offsets, out: torch.Tensor) -> None:
    """The host-side checks of scatter_grads_ (the HIP op makes the same ones)."""
    if out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous():
        raise ValueError("scatter_grads_: out must be a contiguous 1-D fp32 row")
    if len(srcs) != len(offsets):
        raise ValueError(f"scatter_grads_: {len(srcs)} sources, {len(offsets)} offsets")
    d, ranges = out.numel(), []
    for i, (s, o) in enumerate(zip(srcs, offsets)):
        if s.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"scatter_grads_: source {i} must be fp32 or bf16, got {s.dtype}")
        if s.device != out.device:
            raise ValueError(f"scatter_grads_: source {i} must be on out's device")
        o, n = int(o), s.numel()
        if o < 0 or o + n > d:
            raise ValueError(f"scatter_grads_: range [{o}, {o + n}) beyond out's {d} elements")
        if n:
            ranges.append((o, o + n))
    ranges.sort()
    for (_, hi), (lo, hi2) in zip(ranges, ranges[1:]):
        if lo < hi:
            raise ValueError(f"scatter_grads_: range [{lo}, {hi2}) overlaps the one before it")


@torch.no_grad()
def scatter_grads_(srcs, offsets, out: torch.Tensor, channels_last: bool = False) -> None:
    """The gradient sink: the gradients of one backward into a worker's flat payload row.

    srcs: tensors, each fp32 or bf16, on out's device; offsets: host ints; out: (d_pad,)
    fp32 contiguous.  out[o_i : o_i + n_i] = float(src_i), elements in the order of the
    flat space (flat_order: NHWC for 4-D tensors when channels_last, row-major otherwise);
    every element of out that no source covers becomes +0.0, the pad tail included.  The
    ranges must not overlap and must lie inside out.  bf16 -> fp32 is exact (NaN, +-Inf,
    -0.0 and subnormals are kept).  Every element of out is written; the caller clears
    nothing.
    """
    check_scatter_grads(srcs, offsets, out)
    out.zero_()
    for s, o in zip(srcs, offsets):
        out[int(o) : int(o) + s.numel()].copy_(flat_order(s, channels_last))


# --------------------------------------------------------------------- dtype cast
@torch.no_grad()
def cast_to_bf16(x: torch.Tensor, out: torch.Tensor) -> None:
    out.copy_(x)


@torch.no_grad()
def cast_from_bf16(x: torch.Tensor, out: torch.Tensor) -> None:
    out.copy_(x)
