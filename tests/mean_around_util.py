"""Shared by tests/test_mean_around.py and tests/test_mean_around_gpu.py: the data
sets, the planted window groups and two independent numpy statements of
ops.column_mean_around (float64 "drop the farther end b times" and fp32 step by step).
"""
import numpy as np
import torch


def median_bounds(P):
    return (P - 1) // 2, P // 2 + 1


def bounds(P, b, center):
    """(keep, clo, chi) of the rule: centre = median or b-trimmed mean."""
    if center == "median":
        return (P - b,) + median_bounds(P)
    return P - b, b, P - b


def legal_bs(P):
    return sorted({0, 1, (P - 1) // 2} & set(range((P + 1) // 2)))


def data(P, d, seed):
    """Gaussian columns, with every third column drawn from a 16-value grid (ties)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, d, generator=g, dtype=torch.float32)
    grid = (torch.randint(0, 16, (P, d), generator=g).float() - 8.0) / 4.0
    x[:, ::3] = grid[:, ::3]
    return x


def plant(x, b, col0, per_group=8):
    """In place: for every m in 0..b, `per_group` columns from col0 on get m outliers
    far below (-1000 - r) and b - m far above (+1000 + r) the untouched values, in
    rows that rotate with the column.  Needs P > 2b, so both centres stay among the
    untouched values and the window start of group m is exactly m.  Returns
    {m: column indices}."""
    P = x.shape[0]
    assert P > 2 * b
    groups = {}
    col = col0
    for m in range(b + 1):
        cols = list(range(col, col + per_group))
        for j in cols:
            for r in range(b):
                row = (r + j) % P
                x[row, j] = (-1000.0 - r) if r < m else (1000.0 + r)
        groups[m] = cols
        col += per_group
    return groups


def definition_fp64(x, keep, clo, chi):
    """Float64 definition by elimination: sort, drop the end farther from the centre
    b times (a tie drops the top), average what is left.  Returns (out, w, kept |sum|)."""
    P, d = x.shape
    a = np.where(np.isnan(x), np.inf, x.astype(np.float64))
    s = np.sort(a, axis=0)
    cols = np.arange(d)
    with np.errstate(invalid="ignore"):
        c = s[clo:chi].sum(0) / (chi - clo)
        lo = np.zeros(d, dtype=np.int64)
        hi = np.full(d, P, dtype=np.int64)
        for _ in range(P - keep):
            drop_low = (c - s[lo, cols]) > (s[hi - 1, cols] - c)
            lo += drop_low
            hi -= ~drop_low
        assert ((hi - lo) == keep).all()
        win = np.stack([s[lo + k, cols] for k in range(keep)])
        return win.sum(0) / keep, lo, np.abs(win).sum(0)


def definition_fp32(x, keep, clo, chi):
    """The op's four steps in numpy fp32.  Returns (out, w)."""
    P, d = x.shape
    f32 = np.float32
    a = np.where(np.isnan(x), f32(np.inf), x.astype(f32))
    s = np.sort(a, axis=0)
    cols = np.arange(d)
    with np.errstate(invalid="ignore"):
        c = s[clo].copy()
        for k in range(clo + 1, chi):
            c = (c + s[k]).astype(f32)
        c = (c / f32(chi - clo)).astype(f32)
        b = P - keep
        w = np.zeros(d, dtype=np.int64)
        for j in range(b):
            w += ((c - s[j]).astype(f32) > (s[j + keep] - c).astype(f32))
        acc = s[w, cols].copy()
        for k in range(1, keep):
            acc = (acc + s[w + k, cols]).astype(f32)
        return (acc / f32(keep)).astype(f32), w


def same(a, b):
    """== wherever finite or infinite, NaN exactly where the other is NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        a[~np.isnan(a)], b[~np.isnan(b)])
