"""Op dispatch: hand-written HIP/CDNA4 kernels on GPU, pure-torch on CPU.

Every op has identical semantics in both paths; the CPU path doubles as the
numerics oracle for the GPU kernels (tests/test_kernels_gpu.py).
"""
from __future__ import annotations

import torch

from . import fallback
from .fused_bn import fused_bn_act
from .native import available, get_extension, require_extension

__all__ = [
    "fused_sgd_step",
    "fused_adam_step",
    "inject_",
    "collude_",
    "clip_step_",
    "worker_momentum_",
    "mix_rows_",
    "sign_pack",
    "sign_majority",
    "mx8_pack",
    "mx8_unpack",
    "mx8_chunk_bytes",
    "mx8_column_trimmed_mean",
    "mx8_column_mean_around",
    "mx8_clip_step_",
    "mx8_weiszfeld_step",
    "mx8_segment_gram",
    "mx8_segment_mean_around",
    "mx4_pack",
    "mx4_unpack",
    "mx4_chunk_bytes",
    "mx4_column_trimmed_mean",
    "mx4_column_mean_around",
    "scatter_grads_",
    "rows_equal",
    "pair_maxdiff",
    "row_absmax",
    "mean_rows",
    "sum_rows",
    "cyclic_encode",
    "combine_rows",
    "cyclic_project",
    "cyclic_recombine",
    "segment_absmax",
    "segment_pair_maxdiff",
    "segment_sqdist",
    "segment_weighted_mean",
    "segment_gram",
    "column_trimmed_mean",
    "column_mean_around",
    "segment_mean_around",
    "fused_bn_act",
    "available",
]


def _native_for(t: torch.Tensor):
    """Return the HIP extension for CUDA tensors (or None -> fallback allowed)."""
    if t.is_cuda:
        return require_extension()
    return None


def fused_sgd_step(param, grad, momentum_buf, *, lr, momentum, dampening, weight_decay,
                   nesterov, first_step, guard=None):
    """guard: optional 0-dim bool tensor ON DEVICE; False -> the update is a no-op.
    Lets the nan_guard skip poisoned updates without a host round-trip."""
    ext = _native_for(param)
    if ext is not None:
        ext.fused_sgd_step(
            param, grad,
            momentum_buf if momentum_buf is not None else param.new_empty(0),
            lr, momentum, dampening, weight_decay, bool(nesterov), bool(first_step),
            guard if guard is not None else param.new_empty(0, dtype=torch.bool),
        )
        return
    fallback.fused_sgd_step(
        param, grad, momentum_buf,
        lr=lr, momentum=momentum, dampening=dampening,
        weight_decay=weight_decay, nesterov=nesterov, first_step=first_step, guard=guard,
    )


def fused_adam_step(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, *, step, lr, beta1,
                    beta2, eps, weight_decay, amsgrad, guard=None):
    ext = _native_for(param)
    if ext is not None:
        ext.fused_adam_step(
            param, grad, exp_avg, exp_avg_sq,
            max_exp_avg_sq if max_exp_avg_sq is not None else param.new_empty(0),
            int(step), lr, beta1, beta2, eps, weight_decay, bool(amsgrad),
            guard if guard is not None else param.new_empty(0, dtype=torch.bool),
        )
        return
    fallback.fused_adam_step(
        param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq,
        step=step, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
        weight_decay=weight_decay, amsgrad=amsgrad, guard=guard,
    )


def inject_(grad, mode, cyclic=False):
    ext = _native_for(grad)
    if mode in ("random", "none", ""):  # passthrough modes never touch memory
        return
    if ext is not None and mode in ("rev_grad", "constant"):
        ext.inject(grad, mode, bool(cyclic))
        return
    fallback.inject_(grad, mode, cyclic)


def collude_(x, rows, a, b):
    """In place on the exchanged (P, n) block: every row in `rows` (a host sequence of
    distinct ints) becomes a*mu + b*sigma per column, mu / sigma = mean / population
    standard deviation of the other rows.  ALIE: (1, -z); inner-product manipulation:
    (-eps, 0).  The row set reaches the kernel as a 64-bit mask by value: no device
    tensor, no copy.  Definition and checks: fallback.collude_."""
    ext = _native_for(x)
    if ext is not None:
        ext.collude(x, [int(r) for r in rows], float(a), float(b))
        return
    fallback.collude_(x, rows, a, b)


def clip_step_(x, v, w, dist=True):
    """One centered-clipping iteration on the exchanged (P, n) block with the clip
    weights w (P,) given, on x's device and never read on the host: in place,
    v += sum over rows with w_i != 0 of w_i * (x_i - v); returns d2 (P,), the squared
    distance of EVERY row to the new v (the next iteration's weights come from it), or
    None with dist=False.  One pass over x serves both halves, and d2 is reduced in a
    fixed order (no float atomics): two runs agree bit for bit.  Definition and checks:
    fallback.clip_step_."""
    ext = _native_for(x)
    if ext is not None:
        return ext.clip_step(x, v, w, bool(dist))
    return fallback.clip_step_(x, v, w, dist)


def worker_momentum_(g, m, beta, first):
    """Worker-side momentum, in place on a payload row (or a slice of it) g and the same
    span of the worker's state m: first -> m = g; else m = beta*m + (1-beta)*g and
    g = m.  A non-finite g element leaves m as it is and is sent unchanged.  One pass,
    current stream.  Definition and checks: fallback.worker_momentum_."""
    ext = _native_for(g)
    if ext is not None:
        ext.worker_momentum(g, m, float(beta), bool(first))
        return
    fallback.worker_momentum_(g, m, beta, first)


def mix_rows_(x, w, skip=()):
    """In place on the exchanged (P, n) block, P <= 32: y[i, c] = sum over k not in `skip`
    of w[i, k] * x[k, c], w a dense (P, P) fp32 tensor on x's device that is never read
    on the host.  `skip` (a host sequence of distinct ints) reaches the kernel as a
    64-bit mask by value; a skipped row is never loaded, so its NaNs reach no output, and
    is still written.  On the GPU this is the one kernel on the matrix unit (fp32 MFMA,
    W in registers, no second (P, n) buffer); two runs agree bit for bit.  Definition and
    checks: fallback.mix_rows_."""
    ext = _native_for(x)
    if ext is not None:
        ext.mix_rows(x, w, [int(r) for r in skip])
        return
    fallback.mix_rows_(x, w, skip)


def sign_pack(g, out):
    """The signSGD wire format: out (n/16,) int32 = the votes of g (n,) fp32, n % 64 == 0,
    two bits per element (+1: g > 0, -1: g < 0, abstain: +-0 and NaN), 16 bytes per 64
    elements; a 64-aligned slice of g packs to the matching slice of out.  The kernel
    (wave ballots) and the fallback write the same bytes.  Layout and checks:
    fallback.sign_pack."""
    ext = _native_for(g)
    if ext is not None:
        ext.sign_pack(g, out)
        return
    fallback.sign_pack(g, out)


def sign_majority(packed, out):
    """out (n,) fp32 = sign(#pos - #neg) per coordinate over the P <= 64 rows of packed
    (P, n/16) int32 in sign_pack's format: +1.0, -1.0 or +0.0, always finite.  On the GPU
    a bit-sliced vote (vertical counters, 64 coordinates per lane at once) in a fixed
    order: two runs agree bit for bit, and with the fallback.  Definition and checks:
    fallback.sign_majority."""
    ext = _native_for(packed)
    if ext is not None:
        ext.sign_majority(packed, out)
        return
    fallback.sign_majority(packed, out)


def mx8_chunk_bytes(chunk):
    """Bytes of one packed record of the mx8 wire: chunk + round_up(chunk / 32, 16)."""
    return fallback.mx8_chunk_bytes(int(chunk))


def mx8_pack(g, out, chunk):
    """The MXFP8 wire format: out (n / chunk * mx8_chunk_bytes(chunk),) uint8 = the packed
    records of g (n,) fp32, n % chunk == 0, chunk % 64 == 0: one E4M3 code per element and
    one E8M0 scale per 32 elements, NaN / Inf kept non-finite.  A record depends on its
    chunk alone.  The kernel (gfx950 scaled FP8 converts, block amax by DPP) and the
    fallback write the same bytes.  Format: above k_mx8_pack in draco_kernels.hip;
    definition and checks: fallback.mx8_pack."""
    ext = _native_for(g)
    if ext is not None:
        ext.mx8_pack(g, out, int(chunk))
        return
    fallback.mx8_pack(g, out, int(chunk))


def mx8_unpack(packed, out):
    """out (P, chunk) fp32 = the decoded rows of packed (P, mx8_chunk_bytes(chunk)) uint8.
    Every byte pattern decodes to an fp32 value, NaN or +-Inf; kernel and fallback agree
    bit for bit (NaNs as NaNs).  Definition and checks: fallback.mx8_unpack."""
    ext = _native_for(packed)
    if ext is not None:
        ext.mx8_unpack(packed, out)
        return
    fallback.mx8_unpack(packed, out)


def mx8_column_trimmed_mean(packed, lo, hi, out):
    """out (chunk,) fp32 = column_trimmed_mean(mx8_unpack(packed), lo, hi), bit for bit, for
    packed (P, mx8_chunk_bytes(chunk)) uint8, P <= 64, chunk % 64 == 0.  On the GPU one kernel
    reads the records themselves (a dword of codes is four columns of a lane) and the fp32
    block is never formed.  Definition and checks: fallback.mx8_column_trimmed_mean."""
    ext = _native_for(packed)
    if ext is not None:
        ext.mx8_column_trimmed_mean(packed, int(lo), int(hi), out)
        return
    fallback.mx8_column_trimmed_mean(packed, int(lo), int(hi), out)


def mx8_column_mean_around(packed, keep, clo, chi, out):
    """out (chunk,) fp32 = column_mean_around(mx8_unpack(packed), keep, clo, chi), bit for
    bit; shapes and kernel as mx8_column_trimmed_mean.  Definition and checks:
    fallback.mx8_column_mean_around."""
    ext = _native_for(packed)
    if ext is not None:
        ext.mx8_column_mean_around(packed, int(keep), int(clo), int(chi), out)
        return
    fallback.mx8_column_mean_around(packed, int(keep), int(clo), int(chi), out)


def mx8_clip_step_(packed, v, w, dist=True):
    """clip_step_(mx8_unpack(packed), v, w, dist) for packed (P, mx8_chunk_bytes(chunk)) uint8,
    1 <= P <= 64, v (chunk,) fp32 updated in place, w (P,) fp32, without the fp32 block: on
    the GPU one kernel reads the records (k_mx8_clip_step).  v is bit for bit clip_step_'s on
    the decoded block; d2 (P,), or None with dist=False, is within its rounding bound and
    repeatable bit for bit.  Definition and checks: fallback.mx8_clip_step_."""
    ext = _native_for(packed)
    if ext is not None:
        return ext.mx8_clip_step(packed, v, w, bool(dist))
    return fallback.mx8_clip_step_(packed, v, w, dist)


def mx8_weiszfeld_step(packed, w, seg, z, dist=True):
    """One Weiszfeld iteration on packed (P, mx8_chunk_bytes(chunk)) uint8, 1 <= P <= 64, in
    one pass: with w (P, L) fp32 given, z (chunk,) becomes segment_weighted_mean(
    mx8_unpack(packed), w, seg, z), bit for bit (columns outside every segment untouched);
    with w None z is only read.  Returns segment_sqdist(mx8_unpack(packed), z, seg) at the NEW
    z, (P, L) fp32, or None with dist=False.  seg: (L+1,) local bounds, searched on the device.
    The distances end in float atomics: their last bits may differ between two runs, z's do
    not.  Definition and checks: fallback.mx8_weiszfeld_step."""
    ext = _native_for(packed)
    if ext is not None:
        return ext.mx8_weiszfeld_step(packed, w, seg.to(packed.device), z, bool(dist))
    return fallback.mx8_weiszfeld_step(packed, w, seg, z, dist)


def mx8_segment_gram(packed, seg):
    """(L, P, P) fp32 = segment_gram(mx8_unpack(packed), seg) for packed (P,
    mx8_chunk_bytes(chunk)) uint8, 1 <= P <= 32, chunk % 64 == 0; seg: (L+1,) local bounds,
    never read on the host.  On the GPU the block-scaled FP8 matrix instruction multiplies the
    records themselves (a lane holds one MX block of one row as both operands): products are
    exact, the fp32 sums are added with float atomics (last bits may differ between runs), the
    result is exactly symmetric and non-finite wherever the definition's is.  Definition and
    checks: fallback.mx8_segment_gram."""
    ext = _native_for(packed)
    if ext is not None:
        return ext.mx8_segment_gram(packed, seg.to(packed.device))
    return fallback.mx8_segment_gram(packed, seg)


def mx8_segment_mean_around(packed, sel, seg, keep, clo, chi, out):
    """out (chunk,) fp32 = segment_mean_around(mx8_unpack(packed), sel, seg, keep, clo, chi),
    bit for bit, for packed (P, mx8_chunk_bytes(chunk)) uint8 and sel (L, T), 1 <= T <= P <= 32.
    On the GPU one kernel gathers a dword of codes (four columns) per selected row from the
    records; unselected rows are never read.  Definition and checks:
    fallback.mx8_segment_mean_around."""
    ext = _native_for(packed)
    if ext is not None:
        ext.mx8_segment_mean_around(packed, sel.to(packed.device), seg.to(packed.device),
                                    int(keep), int(clo), int(chi), out)
        return
    fallback.mx8_segment_mean_around(packed, sel, seg, int(keep), int(clo), int(chi), out)


def mx4_chunk_bytes(chunk):
    """Bytes of one packed record of the mx4 wire: chunk / 2 + round_up(chunk / 32, 16)."""
    return fallback.mx4_chunk_bytes(int(chunk))


def mx4_pack(g, out, chunk, seed=None):
    """The MXFP4 wire format: out (n / chunk * mx4_chunk_bytes(chunk),) uint8 = the packed
    records of g (n,) fp32, n % chunk == 0, chunk % 64 == 0: one E2M1 nibble per element and
    one E8M0 scale per 32 elements; a block with a NaN / Inf element decodes to 32 NaNs.
    seed=None rounds to nearest; an int seed (taken mod 2^64) rounds stochastically,
    unbiased per element, from a stateless hash of (seed, element index), so the bytes do not
    depend on the device or the launch.  The seed reaches the kernel by value.  The kernel
    (gfx950 scaled FP4 converts for nearest, integer VALU rounding for stochastic, block amax
    by DPP) and the fallback write the same bytes.  Format: above k_mx4_pack in
    draco_kernels.hip; definition and checks: fallback.mx4_pack."""
    ext = _native_for(g)
    if ext is not None:
        ext.mx4_pack(g, out, int(chunk), seed is not None,
                     0 if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF)
        return
    fallback.mx4_pack(g, out, int(chunk), seed)


def mx4_unpack(packed, out):
    """out (P, chunk) fp32 = the decoded rows of packed (P, mx4_chunk_bytes(chunk)) uint8.
    Every byte pattern decodes to an fp32 value, NaN or +-Inf; kernel and fallback agree
    bit for bit (NaNs as NaNs).  Definition and checks: fallback.mx4_unpack."""
    ext = _native_for(packed)
    if ext is not None:
        ext.mx4_unpack(packed, out)
        return
    fallback.mx4_unpack(packed, out)


def mx4_column_trimmed_mean(packed, lo, hi, out):
    """out (chunk,) fp32 = column_trimmed_mean(mx4_unpack(packed), lo, hi), bit for bit, for
    packed (P, mx4_chunk_bytes(chunk)) uint8, 1 <= P <= 64, chunk % 64 == 0.  On the GPU one
    kernel reads the records themselves (a dword of codes is eight columns of a lane) and the
    fp32 block is never formed.  Definition and checks: fallback.mx4_column_trimmed_mean."""
    ext = _native_for(packed)
    if ext is not None:
        ext.mx4_column_trimmed_mean(packed, int(lo), int(hi), out)
        return
    fallback.mx4_column_trimmed_mean(packed, int(lo), int(hi), out)


def mx4_column_mean_around(packed, keep, clo, chi, out):
    """out (chunk,) fp32 = column_mean_around(mx4_unpack(packed), keep, clo, chi), bit for
    bit; shapes and kernel as mx4_column_trimmed_mean.  Definition and checks:
    fallback.mx4_column_mean_around."""
    ext = _native_for(packed)
    if ext is not None:
        ext.mx4_column_mean_around(packed, int(keep), int(clo), int(chi), out)
        return
    fallback.mx4_column_mean_around(packed, int(keep), int(clo), int(chi), out)


def scatter_grads_(srcs, offsets, out, channels_last=False):
    """The gradient sink: out[o_i : o_i + n_i] = float(src_i) for the fp32 / bf16 tensors
    srcs at the host offsets, in the order of the flat space (NHWC for 4-D tensors when
    channels_last), and +0.0 everywhere else in the (d_pad,) fp32 row out, the pad tail
    included: every element is written exactly once and the caller clears nothing.  On the
    GPU one kernel (k_scatter_grads) whose tensor table travels by value in its arguments,
    64 ranges per launch: no device table, no copy, no synchronisation, so the call can be
    captured into a graph.  The kernel reads a source in storage order; a source that is
    not dense in the flat order (contiguous, or channels-last-contiguous for 4-D when
    channels_last) is written by a strided copy_ into its range instead.  Definition and
    checks: fallback.scatter_grads_."""
    ext = _native_for(out)
    if ext is None:
        fallback.scatter_grads_(srcs, offsets, out, channels_last)
        return
    fallback.check_scatter_grads(srcs, offsets, out)
    dense, dense_off, skip_off, skip_len = [], [], [], []
    for s, o in zip(srcs, offsets):
        o = int(o)
        cl = channels_last and s.dim() == 4
        if s.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format):
            dense.append(s)
            dense_off.append(o)
            continue
        dst = out[o : o + s.numel()]
        if cl:
            n, c, h, w = s.shape
            dst = dst.view(n, h, w, c).permute(0, 3, 1, 2)
        else:
            dst = dst.view(s.shape)
        with torch.no_grad():
            dst.copy_(s)
        skip_off.append(o)
        skip_len.append(s.numel())
    ext.scatter_grads(dense, dense_off, skip_off, skip_len, out)


def rows_equal(x, a_idx, b_idx, atol):
    ext = _native_for(x)
    if ext is not None:
        return ext.rows_equal(x, a_idx.to(x.device), b_idx.to(x.device), float(atol))
    return fallback.rows_equal(x, a_idx, b_idx, atol)


def pair_maxdiff(x, a_idx, b_idx):
    ext = _native_for(x)
    if ext is not None:
        return ext.pair_maxdiff(x, a_idx.to(x.device), b_idx.to(x.device))
    return fallback.pair_maxdiff(x, a_idx, b_idx)


def row_absmax(x):
    ext = _native_for(x)
    if ext is not None:
        return ext.row_absmax(x)
    return fallback.row_absmax(x)


def mean_rows(x, idx, out):
    ext = _native_for(x)
    if ext is not None:
        ext.mean_rows(x, idx.to(x.device), out)
        return
    fallback.mean_rows(x, idx, out)


def sum_rows(x, out):
    ext = _native_for(x)
    if ext is not None:
        ext.sum_rows(x, out)
        return
    fallback.sum_rows(x, out)


def cyclic_encode(grads, w_re, w_im, out):
    ext = _native_for(grads)
    if ext is not None:
        ext.cyclic_encode(grads, w_re.to(grads.device), w_im.to(grads.device), out)
        return
    fallback.cyclic_encode(grads, w_re, w_im, out)


def cyclic_project(rows, z):
    ext = _native_for(rows)
    if ext is not None:
        return ext.cyclic_project(rows, z)
    return fallback.cyclic_project(rows, z)


def combine_rows(x, rows, w, out):
    ext = _native_for(x)
    if ext is not None:
        ext.combine_rows(x, rows.to(x.device), w.to(x.device), out)
        return
    fallback.combine_rows(x, rows, w, out)


def combine_rows_slice(x, rows, w, out, col_off):
    """out = sum_i w[i] * x[rows[i], col_off : col_off + len(out)] (bucketed encode)."""
    ext = _native_for(x)
    if ext is not None:
        ext.combine_rows_slice(x, rows.to(x.device), w.to(x.device), out, int(col_off))
        return
    fallback.combine_rows_slice(x, rows, w, out, col_off)


def cyclic_recombine(r_planes, v_re, v_im, out):
    ext = _native_for(r_planes)
    if ext is not None:
        ext.cyclic_recombine(r_planes, v_re.to(r_planes.device), v_im.to(r_planes.device), out)
        return
    fallback.cyclic_recombine(r_planes, v_re, v_im, out)


def segment_absmax(x, seg):
    ext = _native_for(x)
    if ext is not None:
        return ext.segment_absmax(x, seg.to(x.device))
    return fallback.segment_absmax(x, seg)


def segment_pair_maxdiff(x, a_idx, b_idx, seg):
    ext = _native_for(x)
    if ext is not None:
        return ext.segment_pair_maxdiff(x, a_idx.to(x.device), b_idx.to(x.device), seg.to(x.device))
    return fallback.segment_pair_maxdiff(x, a_idx, b_idx, seg)


def segment_sqdist(x, z, seg):
    ext = _native_for(x)
    if ext is not None:
        return ext.segment_sqdist(x, z, seg.to(x.device))
    return fallback.segment_sqdist(x, z, seg)


def segment_weighted_mean(x, w, seg, out):
    ext = _native_for(x)
    if ext is not None:
        ext.segment_weighted_mean(x, w, seg.to(x.device), out)
        return
    fallback.segment_weighted_mean(x, w, seg, out)


def segment_gram(x, seg):
    ext = _native_for(x)
    if ext is not None:
        return ext.segment_gram(x, seg.to(x.device))
    return fallback.segment_gram(x, seg)


def column_trimmed_mean(x, lo, hi, out):
    """out[j] = mean of sorted ranks [lo, hi) of column j (NaN sorts as +inf):
    coordinate-wise median (lo=(P-1)//2, hi=P//2+1) and trimmed mean (lo=b, hi=P-b)."""
    ext = _native_for(x)
    if ext is not None:
        ext.column_trimmed_mean(x, int(lo), int(hi), out)
        return
    fallback.column_trimmed_mean(x, int(lo), int(hi), out)


def column_mean_around(x, keep, clo, chi, out):
    """out[j] = mean of the `keep` values of column j nearest to the centre c = mean of
    sorted ranks [clo, chi) (NaN sorts as +inf): mean around median (clo=(P-1)//2,
    chi=P//2+1) and Phocas (clo=b, chi=P-b), keep = P-b.  Definition, the radius
    guarantee and the missing envelope guarantee: fallback.column_mean_around."""
    ext = _native_for(x)
    if ext is not None:
        ext.column_mean_around(x, int(keep), int(clo), int(chi), out)
        return
    fallback.column_mean_around(x, int(keep), int(clo), int(chi), out)


def segment_mean_around(x, sel, seg, keep, clo, chi, out):
    """out[j] = column_mean_around over the T rows sel[l] of x for column j of segment l
    (seg: (L+1,) local bounds), +0.0 outside [seg[0], seg[L]): the Multi-Krum (keep=T,
    clo=0, chi=T) and Bulyan (keep=T-2f, median centre) decode over a per-segment Krum
    selection.  Unselected rows are never read; sel is clamped into [0, P).  Definition:
    fallback.segment_mean_around."""
    ext = _native_for(x)
    if ext is not None:
        ext.segment_mean_around(x, sel.to(x.device), seg.to(x.device), int(keep), int(clo),
                                int(chi), out)
        return
    fallback.segment_mean_around(x, sel, seg, int(keep), int(clo), int(chi), out)
