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
