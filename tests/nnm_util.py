"""Shared by tests/test_nnm.py and tests/test_nnm_gpu.py: inputs and the plain fp64 loop
statement of ops.mix_rows_ with its derived bound."""
import torch

EPS = 2.0 ** -24


def skip_sets(P):
    return {"none": [], "first": [0], "last": [P - 1],
            "all_but_one": [k for k in range(P) if k != P // 2]}


def mix_case(P, n, skip, seed):
    """x random normal (no denormals), skipped rows NaN; w dense normal, asymmetric."""
    g = torch.Generator().manual_seed(seed)
    x, w = torch.randn(P, n, generator=g), torch.randn(P, P, generator=g)
    x[skip] = float("nan")
    return x, w


def mix_ref(x, w, skip):
    """(ref, bound) in fp64, one term at a time; bound = 2*(P+4)*2^-24 * sum_k |w[i, k]
    x[k, c]|: P products and P-1 additions, each off by at most one ulp whatever rounding
    the matrix unit uses; +4 is the slack the kernel edge tests give."""
    P = x.shape[0]
    X, W = x.double(), w.double()
    ref, mag = torch.zeros_like(X), torch.zeros_like(X)
    for i in range(P):
        for k in (k for k in range(P) if k not in skip):
            ref[i] += W[i, k] * X[k]
            mag[i] += (W[i, k] * X[k]).abs()
    return ref, 2.0 * (P + 4) * EPS * mag


def check_mix(got, x, w, skip, what):
    ref, bound = mix_ref(x, w, skip)
    assert bool(torch.isfinite(got).all()), what
    assert bool(((got.double() - ref).abs() <= bound).all()), what
