"""Shared pieces of the centered-clipping tests (ops.clip_step_ and
CenteredClipAggregator): fp64 oracles and the rounding bounds, each derived here.

u = 2^-24 (fp32 unit roundoff).

v bound.  Per column, delta = sum of at most P terms w_i * (x_ij - v_j) with w_i >= 0 and
sum w_i <= 1, then v_j + delta.  With M_j = |v_j| + max over the rows with w_i != 0 of
|x_ij|: the difference rounds once (<= u*M_j), the product once, the sum of k <= P terms
adds <= (k-1)*u times the partial sums (each <= M_j because sum w_i <= 1), and the final
add rounds once: <= (P + 4)*u*M_j to first order, and FMA contraction only removes
roundings.  8*P*u*M_j covers it for every P >= 1.

d2 bound.  Evaluated in fp64 AT THE RESULT'S OWN v_new, so the error in v does not enter.
Every term (x_ij - v_j)^2 is non-negative: the difference rounds once, the square once
(relative 3u together), and a sum of n non-negative terms in ANY order has relative error
<= (n-1)*u: <= (n + 8)*u relative.  A row equal to v_new gives exactly 0.

Aggregator bounds (L2 over the whole vector).  For a fixed radius t the exact step
F_t(v) = v + (1/P) sum_i proj_t(x_i - v), proj_t the projection onto the ball of radius
t, is non-expansive in v (each v + proj_t(x_i - v) = x_i - (I - proj_t)(x_i - v) and
I - proj_t is 1-Lipschitz), 1/P-Lipschitz in each x_i, and 1-Lipschitz in t.  The
computed step differs from F_t at its own v and own t by
  * the clip factors: they come from computed distances d~ = d*(1 + eta), |eta| <= rho,
    rho = (n + 8)*u (the d2 bound; the root halves it, the fp64 arithmetic is
    negligible), and d * |min(1, t/d~) - min(1, t/d)| <= t*rho/(1 - rho);
  * the fp32 weight c/P: relative u, so <= u*t in the step;
  * the v bound, as an L2 norm: beta = ||8*P*u*2*max_i|x_ij| ||_2, using |v_j| <=
    max(|v0_j|, max_i |x_ij|) (a step is a sub-convex combination, sum w_i <= 1).
Auto t is an order statistic of the computed distances at v0, 1-Lipschitz in them:
|t~ - t| <= rho*D.  Clipping acts only where t < d, and every distance met is <=
D = 2*D0, D0 the largest finite distance to v0 (v stays in the hull of v0 and the rows), so
t may be replaced by D.  One iteration therefore adds at most
  step_error = rho*D + 1.001*rho*D + u*D + beta
to ||v_computed - v_exact||, and `iters` iterations add iters times that.
Two devices that also disagree on one row by eps_x in L2 (the colluding row, computed on
each device) differ by at most 2*iters*step_error + iters*(eps_x/P + eps_x): the row
enters the step with 1/P and auto t with 1.
"""
import torch

U = 2.0 ** -24
KINDS = ("randn", "offset", "equal_v")


def bits(t):
    return t.contiguous().view(torch.int32)


def make_case(kind, P, n, seed):
    """(x, v) fp32 on CPU."""
    g = torch.Generator().manual_seed(seed)
    if kind == "randn":
        return (torch.randn(P, n, generator=g), torch.randn(n, generator=g))
    if kind == "offset":  # x - v cancels seven digits
        v = 1e4 + 1e-3 * torch.randn(n, generator=g)
        return 1e4 + 1e-3 * torch.randn(P, n, generator=g), v
    if kind == "equal_v":  # every row equals v: delta and every distance are exactly 0
        v = torch.randn(n, generator=g)
        return v.repeat(P, 1).contiguous(), v
    raise ValueError(kind)


def weight_patterns(P, seed):
    """name -> (P,) fp32 weights, w_i >= 0, sum <= 1 (up to its own rounding)."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.rand(P, generator=g, dtype=torch.float64) + 0.05
    full = (raw / raw.sum()).float()
    edge = (raw / raw.sum() * 0.7).float()
    edge[0] = 0.0
    edge[P - 1] = 0.0
    return {"zero": torch.zeros(P), "edge_zeros": edge, "sum_one": full}


def oracle_step(x, v, w):
    """fp64 v_new of the fp32 inputs, and the per-column v bound."""
    P = x.shape[0]
    used = [p for p in range(P) if float(w[p]) != 0.0]
    V = v.double()
    if not used:
        return V.clone(), torch.zeros_like(V)
    X = x[used].double()
    W = w[used].double()
    v_new = V + (W[:, None] * (X - V)).sum(dim=0)
    bound = 8.0 * P * U * (V.abs() + X.abs().amax(dim=0))
    return v_new, bound


def oracle_d2(x, v_new):
    """fp64 squared distances of the fp32 rows to the fp32 v_new, and the relative bound."""
    n = x.shape[1]
    d2 = ((x.double() - v_new.double()) ** 2).sum(dim=1)
    return d2, (n + 8) * U


def check_step(x, v0, w, v_new, d2, what):
    """v_new / d2 = result of clip_step_(x, v0 copy, w).  Returns worst error / bound
    for v and for d2 (finite inputs)."""
    ref, bound = oracle_step(x, v0, w)
    if not bool((w != 0).any()):
        assert torch.equal(bits(v_new), bits(v0)), (what, "v written with every w_i == 0")
    err = (v_new.double() - ref).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), (what, "v", int(bad.sum()), float(err[bad][0]),
                                 float(bound[bad][0]))
    nz = bound > 0
    worst_v = float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0
    worst_d = 0.0
    if d2 is not None:
        want, rel = oracle_d2(x, v_new)
        derr = (d2.double() - want).abs()
        bad = ~(derr <= rel * want)
        assert not bool(bad.any()), (what, "d2", int(bad.sum()), float(derr[bad][0]),
                                     float(want[bad][0]))
        pos = want > 0
        if bool(pos.any()):
            worst_d = float((derr[pos] / (rel * want[pos])).max())
    return worst_v, worst_d


def oracle_aggregate(x, v0, tau, iters, excluded=()):
    """fp64 centered clipping of the rows of x from v0; the rows in `excluded` (and any
    row at a non-finite distance) get c = 0 and never enter the arithmetic.  tau None =
    auto: the (P+1)//2-th smallest distance to v0, excluded rows counted as +inf.
    Returns (v, last c)."""
    P = x.shape[0]
    keep = [p for p in range(P) if p not in set(excluded)]
    X = x[keep].double()
    v = v0.double().clone()
    inf = float("inf")

    def dists():
        d = torch.full((P,), inf, dtype=torch.float64)
        dk = ((X - v) ** 2).sum(dim=1).sqrt()
        d[keep] = torch.where(torch.isfinite(dk), dk, torch.full_like(dk, inf))
        return d

    d = dists()
    if tau is None:
        tau = float(torch.kthvalue(d, (P + 1) // 2).values)
    c = torch.zeros(P, dtype=torch.float64)
    for _ in range(iters):
        c = torch.where(d <= tau, torch.ones_like(d), tau / d)
        c = torch.where(torch.isfinite(d), c, torch.zeros_like(d))
        rows = [i for i, p in enumerate(keep) if float(c[p]) != 0.0]
        if rows:
            ck = c[keep][rows]
            v = v + (ck[:, None] * (X[rows] - v)).sum(dim=0) / P
        d = dists()
    return v, c


def step_error(x_finite, v0, P, iters):
    """iters * step_error of the module docstring for the finite rows x_finite (fp32) of a
    P-row block: the allowed L2 distance between the computed and the exact aggregate."""
    n = x_finite.shape[1]
    X = x_finite.double()
    D = 2.0 * float(((X - v0.double()) ** 2).sum(dim=1).sqrt().max())
    rho = (n + 8) * U
    m = torch.maximum(X.abs().amax(dim=0), v0.double().abs())
    beta = float((8.0 * P * U * 2.0 * m).norm())
    return iters * (rho * D + 1.001 * rho * D + U * D + beta)


def device_gap(x_finite, v0, P, iters, eps_x):
    """Allowed L2 distance between two devices' aggregates of blocks that differ by
    eps_x (L2) in one row."""
    return 2.0 * step_error(x_finite, v0, P, iters) + iters * (eps_x / P + eps_x)
