"""Nearest-neighbour mixing on the CPU: fallback.mix_rows_ against the fp64 loop, the
selection against a brute-force numpy oracle, and the wiring."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.ops import fallback as fb
from draco_amd.parallel import Communicator, FlatSpace
from draco_amd.parallel import aggregators as A
from draco_amd.parallel.mixing import NearestNeighborMixing
from tests.bulyan_util import oracle_distances
from tests.nnm_util import EPS, check_mix, mix_case, skip_sets

CPU = torch.device("cpu")
COMM = Communicator(0, 1, CPU)


@pytest.mark.parametrize("kind", ["none", "first", "last"])
@pytest.mark.parametrize("P", [1, 2, 3, 7, 32])
def test_fallback_mix_rows(P, kind):
    skip = skip_sets(P)[kind]
    x, w = mix_case(P, 20, skip, seed=P)
    y = x.clone()
    fb.mix_rows_(y, w, skip)
    check_mix(y, x, w, skip, (P, kind))
    assert "mix_rows_" in ops.__all__


@pytest.mark.parametrize("f", [1, 2])
def test_selection_matches_brute_force(f):
    """Integer points on a line: every fp32 Gram entry is exact, neighbour gaps are >= 9.
    Rows 4 and 5 are exactly equidistant from row 0 (the lower index wins the last place
    of N_0 at f = 2); row 3 is non-finite."""
    pos = [0.0, 3.0, -3.0, 50.0, 10.0, -10.0, 7.0]
    P, bad = len(pos), 3
    x = torch.zeros(P, 8)
    x[:, 0] = torch.tensor(pos)
    x[bad, 5] = float("nan")
    D = oracle_distances(x.numpy())
    np.fill_diagonal(D, 0.0)
    near = [sorted(range(P), key=lambda j: (D[i, j], j))[: P - f] for i in range(P)]
    mix = NearestNeighborMixing(COMM, f)
    y, W = mix(x.clone()), mix.last_weights
    assert bool(torch.isnan(W[bad]).all()) and bool(torch.isnan(y[bad]).all())
    for i in (i for i in range(P) if i != bad):
        assert bad not in near[i]
        assert sorted(torch.nonzero(W[i]).flatten().tolist()) == sorted(near[i]), i
        assert bool((W[i][near[i]] == np.float32(1.0 / (P - f))).all())
        want = x[near[i]].double().mean(dim=0)  # |x| <= 50 and the weights sum to 1
        assert bool(torch.isfinite(y[i]).all())
        assert bool(((y[i].double() - want).abs() <= 2 * (P + 4) * EPS * 50.0).all()), i
    if f == 2:
        assert 4 in near[0] and 5 not in near[0]


def _cfg(**kw):
    return Config(**{**dict(network="FC", dataset="MNIST", device="cpu", approach="baseline",
                            mode="median", worker_fail=1, pre_aggregation="nnm"), **kw})


def test_wiring():
    P = 7
    torch.manual_seed(0)
    space = FlatSpace(nn.Sequential(nn.Linear(30, 9), nn.Linear(9, 3)), 1, CPU)
    agg = A.build_baseline_aggregator(_cfg(), COMM, space, P)
    assert isinstance(agg.mixing, NearestNeighborMixing) and agg.mixing.f == 1
    payload = torch.zeros(P, space.d_pad)
    payload[:, : space.d] = torch.randn(P, space.d)
    hand = payload.clone()
    NearestNeighborMixing(COMM, 1)(hand)
    want = torch.empty(space.d_pad)
    ops.column_trimmed_mean(hand, 3, 4, want)
    assert torch.equal(agg.aggregate(payload.clone(), 0), want)
    assert not torch.equal(hand, payload)
    mean = A.build_baseline_aggregator(_cfg(mode="normal"), COMM, space, P)
    assert type(mean) is A.TrimmedMeanAggregator and mean.name == "mean" and mean.trim == 0
    for mode in ("normal", "median", "multi_krum"):
        off = A.build_baseline_aggregator(_cfg(mode=mode, pre_aggregation="none"), COMM, space, P)
        assert off.mixing is None and A.Aggregator.mixing is None


@pytest.mark.parametrize("kw", [dict(approach="maj_vote"), dict(approach="cyclic"),
                                dict(topology="ps"), dict(health_timeout=5.0),
                                dict(worker_fail=0), dict(pre_aggregation="mix")])
def test_sanity_rejects(kw):
    _cfg(worker_momentum=0.9, momentum=0.0, err_mode="alie").sanity()
    with pytest.raises(ValueError, match="pre-aggregation"):
        _cfg(**kw).sanity()


@pytest.mark.parametrize("P,f", [(4, 2), (33, 1)])
def test_worker_count_checked_at_construction_and_per_call(P, f):
    for build in (lambda: NearestNeighborMixing(COMM, f, num_workers=P),
                  lambda: NearestNeighborMixing(COMM, f)(torch.zeros(P, 8))):
        with pytest.raises(ValueError, match="nnm"):
            build()
