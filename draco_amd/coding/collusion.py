"""Colluding adversaries: Byzantine workers that act together and see the honest
gradients, where rev_grad / constant / gauss are computed by one worker from its own.

  alie  "A Little Is Enough" (Baruch et al., arXiv:1902.06156): every Byzantine worker
        sends mu - z*sigma per coordinate (mu, sigma = mean and population standard
        deviation of the honest workers' values).  It stays inside the honest spread,
        so distance tests and trimming do not remove it.
  ipm   inner-product manipulation (Xie et al., arXiv:1903.03936): every Byzantine
        worker sends -eps*mu.  A small eps sits near the middle of the cloud (Krum picks
        it); a large eps turns the plain mean into gradient ascent.

Both are the per-coordinate map a*mu + b*sigma (ops.collude_), so they commute with
the d/N sharding: the baseline aggregators apply them to the exchanged (P, shard)
block, whose row index is the logical worker id, with no extra communication.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from statistics import NormalDist

COLLUDING_MODES = ("alie", "ipm")
IPM_DEFAULT_EPS = 0.1


def alie_z_max(P: int, f: int) -> float:
    """The paper's z_max: with s = floor(P/2 + 1) - f (the honest workers the f
    Byzantine ones need on their side for a majority), z = Phi^-1((P - f - s)/(P - f)).
    0 where that ratio is <= 0.5 or the formula is undefined (P <= f, or s <= 0).  At
    small P this is often 0 -- (8, 2) gives 0, (7, 3) gives 0.6745 -- so experiments at
    small P pass the parameter explicitly."""
    if P - f <= 0:
        return 0.0
    s = math.floor(P / 2 + 1) - f
    ratio = (P - f - s) / (P - f)
    if not 0.5 < ratio < 1.0:
        return 0.0
    return NormalDist().inv_cdf(ratio)


def collusion_coefficients(mode: str, P: int, f: int, param: float = math.nan):
    """(a, b) of the overwrite a*mu + b*sigma for a colluding mode with P workers, f of
    them Byzantine.  param is z (alie) or eps (ipm); NaN takes the default: alie_z_max
    (which can be 0 at small P, see there) and eps = 0.1."""
    default = param is None or math.isnan(param)
    if mode == "alie":
        z = alie_z_max(P, f) if default else float(param)
        return 1.0, 0.0 - z
    if mode == "ipm":
        eps = IPM_DEFAULT_EPS if default else float(param)
        return -eps, 0.0
    raise ValueError(f"unknown colluding mode {mode!r}; the colluding modes are "
                     f"{'/'.join(COLLUDING_MODES)}")


@dataclass
class Collusion:
    """What an Aggregator needs to overwrite the Byzantine rows of the exchanged block:
    the coefficients, fixed for the run, and the step's Byzantine rows, which the
    trainer sets from the host-side schedule before every aggregate()."""

    a: float
    b: float
    rows: tuple = ()
