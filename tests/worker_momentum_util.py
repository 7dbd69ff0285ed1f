"""fp64 oracle and rounding bound for ops.worker_momentum_ (worker-side momentum,
arXiv:2012.10333), shared by the CPU and the GPU tests.

The op, per element:  first -> m = g;  later -> m = beta*m + (1-beta)*g, g = m;  a
non-finite g leaves m as it is (0 on the first step) and is sent unchanged.

The bound.  Exact value E = beta*m + (1-beta)*g with beta and 1-beta as doubles and m, g
the fp32 inputs.  Either implementation rounds to fp32 (u = 2^-24 relative, each): the
coefficient beta, the coefficient 1-beta (formed in double, cast once), the product
c*g, and the final fma (kernel) or add (fallback; the fallback also rounds the product
beta*m, the kernel does not).  Each of the two terms therefore carries at most three
roundings, (1+u)^3 - 1 < 3.0000004*u, and the last rounding acts on a sum of magnitude
at most (1+3.0000004*u)*(|beta*m| + |(1-beta)*g|); together that is below
4*u*(|beta*m| + |(1-beta)*g|).  2^-149 (one fp32 subnormal step) covers underflow of a
product or of the result.  First-step outputs and the non-finite branches involve no
arithmetic and are compared bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
NONFINITE = (float("nan"), float("inf"), float("-inf"))


def bits(t: torch.Tensor) -> torch.Tensor:
    """The fp32 bit patterns, for comparisons that NaN == NaN and -0.0 != 0.0."""
    return t.detach().cpu().contiguous().view(torch.int32)


def oracle(g, m, beta: float, first: bool):
    """(sent, m_new) in fp64 from fp32 arrays/tensors g, m (non-finite rule included)."""
    g = np.asarray(torch.as_tensor(g).detach().cpu().numpy(), dtype=np.float64)
    m = np.asarray(torch.as_tensor(m).detach().cpu().numpy(), dtype=np.float64)
    fin = np.isfinite(g)
    if first:
        return g.copy(), np.where(fin, g, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        upd = float(beta) * m + (1.0 - float(beta)) * g
    return np.where(fin, upd, g), np.where(fin, upd, m)


def bound(g, m, beta: float):
    """Per-element bound on |m_new - exact| for finite g (np.float64 array)."""
    g = np.asarray(torch.as_tensor(g).detach().cpu().numpy(), dtype=np.float64)
    m = np.asarray(torch.as_tensor(m).detach().cpu().numpy(), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return 4.0 * U * (np.abs(float(beta) * m) + np.abs((1.0 - float(beta)) * g)) + TINY


def check_update(g0, m0, g1, m1, beta: float, label="") -> float:
    """Assert one non-first update (g0, m0) -> (g1, m1) against the oracle: finite
    elements within the bound, sent element == new state bit for bit, non-finite
    elements untouched bit for bit.  Returns the worst error / bound ratio."""
    fin = torch.isfinite(torch.as_tensor(g0).detach().cpu()).numpy()
    sent, exact = oracle(g0, m0, beta, first=False)
    b = bound(g0, m0, beta)
    got = m1.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - exact)
    ratio = float((err[fin] / b[fin]).max()) if fin.any() else 0.0
    print(f"worker_momentum {label}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0, (label, ratio)
    bg0, bm0, bg1, bm1 = bits(g0), bits(m0), bits(g1), bits(m1)
    f = torch.from_numpy(fin)
    assert torch.equal(bg1[f], bm1[f]), (label, "sent row is not the new state")
    assert torch.equal(bm1[~f], bm0[~f]), (label, "state changed under a non-finite g")
    assert torch.equal(bg1[~f], bg0[~f]), (label, "non-finite g was not sent as it is")
    return ratio


def check_first(g0, g1, m1, label="") -> None:
    """First step: m = g bit for bit (0 where g is non-finite), g unchanged."""
    fin = torch.isfinite(torch.as_tensor(g0).detach().cpu())
    bg0, bg1, bm1 = bits(g0), bits(g1), bits(m1)
    assert torch.equal(bg1, bg0), (label, "g changed on the first step")
    assert torch.equal(bm1[fin], bg0[fin]), (label, "m is not a bit copy of g")
    assert bool((bm1[~fin] == 0).all()), (label, "m is not +0 under a non-finite g")


def make_pair(n: int, seed: int):
    """Random fp32 (g, m) of mixed magnitudes, with exact zeros and a -0.0."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(n, generator=gen) * torch.exp2(torch.randint(-12, 6, (n,), generator=gen).float())
    m = torch.randn(n, generator=gen) * torch.exp2(torch.randint(-12, 6, (n,), generator=gen).float())
    if n >= 4:
        g[1] = 0.0
        m[2] = 0.0
        g[3] = -0.0
    return g.contiguous(), m.contiguous()
