"""Shared by tests/test_bulyan.py and tests/test_bulyan_gpu.py: row selections, well
separated worker rows, an independent numpy statement of ops.segment_mean_around and
brute-force fp64 loop oracles of the two Krum selections (distances from the rows, in
the style of tests/test_aggregator_oracles.py::test_krum_matches_oracle).
"""
import numpy as np
import torch

from tests.mean_around_util import definition_fp32

EPS = 2.0 ** -24


def random_sel(L, P, T, seed):
    """(L, T) int64: a different random T-subset of range(P) per segment, unsorted."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(P, generator=g)[:T] for _ in range(L)])


def seg_definition_fp32(x, sel, seg, keep, clo, chi):
    """ops.segment_mean_around in numpy fp32: per segment, the op's four steps
    (mean_around_util.definition_fp32) on the gathered rows; +0.0 elsewhere."""
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros(x.shape[1], dtype=np.float32)
    for l in range(len(seg) - 1):
        lo, hi = int(seg[l]), int(seg[l + 1])
        if hi > lo:
            out[lo:hi] = definition_fp32(x[np.asarray(sel[l])][:, lo:hi], keep, clo, chi)[0]
    return out


def separated_rows(P, d, bad, seed, attack="plus100"):
    """(P, d) fp32: honest row p = g + 0.05*(p+1)*noise_p, so honest rows differ in
    their distance to the others by far more than the fp32 rounding of a Gram matrix;
    rows in `bad` are adversarial: "plus100" = g + 100*(k+1) for the k-th of them,
    "collude" = g + 100 for all of them (identical rows: distance 0 to each other),
    "rev" = -100*(k+1)*g, and "nan", "inf", "-inf" = an honest-looking row with every third
    element non-finite (every segment of 3+ elements holds one)."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=d).astype(np.float32)
    rows = np.stack([g + np.float32(0.05 * (p + 1)) * rng.normal(size=d).astype(np.float32)
                     for p in range(P)])
    for k, p in enumerate(bad):
        if attack == "plus100":
            rows[p] = g + np.float32(100.0 * (k + 1))
        elif attack == "collude":
            rows[p] = g + np.float32(100.0)
        elif attack == "rev":
            rows[p] = np.float32(-100.0 * (k + 1)) * g
        else:
            rows[p, ::3] = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf}[attack]
    return rows


def oracle_distances(Xl):
    """(P, P) fp64 squared distances computed from the rows; non-finite -> +inf."""
    P = Xl.shape[0]
    D = np.full((P, P), np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(P):
            for j in range(P):
                if i != j:
                    v = float(np.sum((Xl[i].astype(np.float64) - Xl[j].astype(np.float64)) ** 2))
                    D[i, j] = v if np.isfinite(v) else np.inf
    return D


def _score(D, i, others, keep):
    return float(sum(sorted(D[i, j] for j in others if j != i)[:keep])) if len(others) > 1 \
        else float("inf")


def oracle_multi_krum(D, f, m):
    """One-shot: the m lowest scores, ties to the lower index.  Returns (rows, scores)."""
    P = D.shape[0]
    keep = max(P - f - 2, 1)
    scores = [_score(D, i, range(P), keep) for i in range(P)]
    order = sorted(range(P), key=lambda i: (scores[i], i))
    return order[:m], scores


def oracle_bulyan(D, f, theta):
    """Iterative: theta picks, each the lowest score among the remaining rows (lower
    index on ties), scored against the remaining rows only.  Returns (rows, per-pick
    {row: score} of the candidates)."""
    remaining = list(range(D.shape[0]))
    picks, history = [], []
    for _ in range(theta):
        keep = max(len(remaining) - f - 2, 1)
        scores = {i: _score(D, i, remaining, keep) for i in remaining}
        win = min(remaining, key=lambda i: (scores[i], i))
        picks.append(win)
        history.append(scores)
        remaining.remove(win)
    return picks, history


def gram_error_bound(Xl, rows):
    """Worst-case error of an fp32-Gram squared distance between two of `rows`: three
    fp32 dot products of length n, each within n*2^-24*|a||b| of exact (plus the
    roundings of forming the combination, covered by n+2 and the factor 2)."""
    n = Xl.shape[1]
    norms = [float(np.linalg.norm(Xl[i].astype(np.float64))) for i in rows]
    top = sorted(norms)[-2:] if len(norms) > 1 else norms * 2
    return 2.0 * (n + 2) * EPS * (top[0] + top[1]) ** 2
