"""Training BatchNorm2d fused with the residual add and ReLU behind it (bf16 NHWC).

`fused_bn_act(x, bn, residual, relu)` computes `relu(bn(x) + residual)` with the HIP
kernels of csrc/bn_kernels.hip when the input is exactly the flagship's hot path, and
with the plain torch expression in every other case (CPU, eval mode, fp32, NCHW, odd
channel counts, extension not built), so nothing outside that gate changes.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .native import get_extension

_CL = torch.channels_last


def _native_gate(x, bn, residual) -> bool:
    if not (x.is_cuda and bn.training and x.dtype == torch.bfloat16 and x.dim() == 4):
        return False
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        return False
    c = x.shape[1]
    if c == 0 or c % 8 != 0 or x.numel() // c < 2 or x.numel() >= 2 ** 31:
        return False
    if not x.is_contiguous(memory_format=_CL):
        return False
    if residual is not None and not (
            residual.is_cuda and residual.dtype == torch.bfloat16
            and residual.shape == x.shape and residual.is_contiguous(memory_format=_CL)):
        return False
    if bn.weight.dtype != torch.float32 or bn.running_mean.dtype != torch.float32:
        return False
    return get_extension() is not None


class _FusedBNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, bn, relu):
        ext = get_extension()
        y, save_mean, save_invstd = ext.bn_act_forward(
            x, residual if residual is not None else x.new_empty(0), gamma, beta,
            bn.running_mean, bn.running_var, bn.num_batches_tracked,
            float(bn.momentum), float(bn.eps), relu)
        # y doubles as the ReLU mask: no pre-activation tensor is kept (and without a
        # ReLU the backward does not need y at all)
        ctx.save_for_backward(x, y if relu else None, gamma, save_mean, save_invstd)
        ctx.relu = relu
        ctx.has_residual = residual is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, y, gamma, save_mean, save_invstd = ctx.saved_tensors
        dy = dy.contiguous(memory_format=_CL)
        dx, dgamma, dbeta, dz = get_extension().bn_act_backward(
            dy, x, y if ctx.relu else x, gamma, save_mean, save_invstd, ctx.relu,
            ctx.has_residual)
        dres = None
        if ctx.has_residual:
            dres = dz if ctx.relu else dy
        return dx, dgamma, dbeta, dres, None, None


def fused_bn_act(x, bn, residual=None, relu=True):
    """[relu](bn(x) [+ residual]) for an nn.BatchNorm2d module `bn`."""
    if _native_gate(x, bn, residual):
        return _FusedBNAct.apply(x, bn.weight, bn.bias, residual, bn, bool(relu))
    out = bn(x)
    if residual is not None:
        out = out + residual
    if relu:
        out = F.relu(out)
    return out
