"""Shared by test_collusion.py and test_collusion_gpu.py: the data kinds, the fp64
oracle of ops.collude_ and its derived error bound.

Bound (u = 2^-24, M_j = max over honest |x[., j]|): sequential fp32 summation of
h <= P values gives |mu^ - mu| <= P*u*M_j; perturbing every deviation by delta moves
sigma by at most delta and the second summation adds at most P*u*M_j, so
|sigma^ - sigma| <= 2*P*u*M_j; together |out - exact| <= 2(|a|+|b|)*P*u*M_j plus the
final roundings.  The tests allow 4x that: 8*(|a|+|b|)*P*2^-24*M_j per column.
"""
import torch

U = 2.0 ** -24
KINDS = ("randn", "grid", "offset", "wide")
AB = [(1.0, -1.5), (-4.0, 0.0), (1.0, -0.3)]  # ALIE z=1.5, IPM eps=4, ALIE z=0.3


def make_data(kind, P, d, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "randn":
        return torch.randn(P, d, generator=g, dtype=torch.float32)
    if kind == "grid":  # 16 values: ties, sigma often small or zero
        return (torch.randint(0, 16, (P, d), generator=g).float() - 8.0) / 4.0
    if kind == "offset":  # the column that breaks a one-pass E[x^2] - mu^2 variance
        return 1e4 + 1e-3 * torch.randn(P, d, generator=g, dtype=torch.float32)
    if kind == "wide":  # magnitudes spread over e^+-8 and beyond
        return (torch.randn(P, d, generator=g, dtype=torch.float32)
                * torch.exp(8.0 * torch.randn(P, d, generator=g, dtype=torch.float32)))
    raise ValueError(kind)


def honest_rows(P, rows):
    byz = set(rows)
    return [p for p in range(P) if p not in byz]


def scattered(P):
    """floor((P-1)/2) rows spread over [0, P) (every other row, from row 1)."""
    return list(range(1, P, 2))[: (P - 1) // 2]


def oracle(x, rows, a, b):
    """fp64 a*mu + b*sigma of the honest rows of the fp32 x, and the allowed error."""
    X = x[honest_rows(x.shape[0], rows)].double()
    mu = X.mean(dim=0)
    sigma = ((X - mu) ** 2).mean(dim=0).sqrt()
    bound = 8.0 * (abs(a) + abs(b)) * x.shape[0] * U * X.abs().amax(dim=0)
    return a * mu + b * sigma, bound


def bits(t):
    return t.contiguous().view(torch.int32)


def check_result(x0, y, rows, a, b, what):
    """y = collude_(x0 copy): honest rows bitwise unchanged, Byzantine rows bitwise
    equal to each other and within the bound of the fp64 oracle.  Returns the largest
    |error| / bound (columns with bound 0 must be exact)."""
    P = x0.shape[0]
    hon = honest_rows(P, rows)
    assert torch.equal(bits(y[hon]), bits(x0[hon])), (what, "an honest row was written")
    for r in rows[1:]:
        assert torch.equal(bits(y[r]), bits(y[rows[0]])), (what, "Byzantine rows differ", r)
    ref, bound = oracle(x0, rows, a, b)
    err = (y[rows[0]].double() - ref).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), (what, int(bad.sum()), int(bad.nonzero()[0]),
                                 float(err[bad][0]), float(bound[bad][0]))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0
