"""Colluding adversaries (ALIE, arXiv:1902.06156; inner-product manipulation,
arXiv:1903.03936) on CPU: fallback.collude_ against an fp64 oracle within the derived
bound (tests/collusion_util.py), the attack definitions, the config restrictions, the
aggregator hook, training under attack and the sharded decode.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from draco_amd import ops
from draco_amd.coding import COLLUDING_MODES, Collusion, collusion_coefficients
from draco_amd.config import Config, parse_cli
from draco_amd.ops import fallback as fb
from draco_amd.parallel.aggregators import TrimmedMeanAggregator
from draco_amd.parallel.comm import Communicator
from draco_amd.parallel.flat import FlatSpace
from tests.collusion_util import AB, KINDS, U, bits, check_result, make_data, scattered
from tests.dist_util import run_dist

D = 4096


def _row_sets(P):
    sets = [[P - 1], [0]]
    if (P - 1) // 2 >= 1:
        sets.append(scattered(P))
    return sets


# --------------------------------------------------------------- 1. fallback vs fp64
@pytest.mark.parametrize("P", [2, 3, 5, 8, 17, 33, 64])
def test_fallback_within_bound_of_fp64_oracle(P):
    worst = 0.0
    for k, kind in enumerate(KINDS):
        x0 = make_data(kind, P, D, seed=100 * P + k)
        for a, b in AB:
            for rows in _row_sets(P):
                y = x0.clone()
                ops.collude_(y, rows, a, b)  # CPU tensor: the dispatcher takes the fallback
                worst = max(worst, check_result(x0, y, rows, a, b, (P, kind, a, b, rows)))
    print(f"P={P}: worst |error| / bound = {worst:.4f}")


# --------------------------------------------------------------- 2. equal honest rows
@pytest.mark.parametrize("P", [2, 5, 64])
def test_equal_honest_rows_give_a_times_c_and_never_nan(P):
    g = torch.Generator().manual_seed(P)
    c = torch.randn(D, generator=g) * torch.exp(4.0 * torch.randn(D, generator=g))
    c[::7] = 0.0
    c[1::7] = 1e4
    x0 = c.repeat(P, 1).contiguous()
    for a, b in AB:
        for rows in _row_sets(P):
            y = x0.clone()
            fb.collude_(y, rows, a, b)
            out = y[rows[0]]
            assert bool(torch.isfinite(out).all()), (P, a, b, rows)
            bound = 8.0 * (abs(a) + abs(b)) * P * U * c.double().abs()
            assert bool(((out.double() - a * c.double()).abs() <= bound).all()), (P, a, b, rows)
            check_result(x0, y, rows, a, b, (P, a, b, rows))


# --------------------------------------------------------------- 3. rejections
def test_rejections_and_empty_rows():
    with pytest.raises(ValueError):
        fb.collude_(torch.zeros(1, 8), [0], 1.0, -1.0)  # P = 1
    with pytest.raises(ValueError):
        fb.collude_(torch.zeros(65, 8), [0], 1.0, -1.0)  # P = 65
    with pytest.raises(ValueError):
        fb.collude_(torch.zeros(4, 6), [0], 1.0, -1.0)  # d % 4 != 0
    with pytest.raises(ValueError):
        fb.collude_(torch.zeros(4, 8), [1, 1], 1.0, -1.0)  # duplicate
    with pytest.raises(ValueError):
        fb.collude_(torch.zeros(4, 8), [4], 1.0, -1.0)  # out of range
    with pytest.raises(ValueError):
        fb.collude_(torch.zeros(4, 8), [-1], 1.0, -1.0)
    with pytest.raises(ValueError):
        fb.collude_(torch.zeros(4, 8), [0, 1, 2, 3], 1.0, -1.0)  # nobody honest
    with pytest.raises(ValueError):
        fb.collude_(torch.zeros(4, 8, dtype=torch.float64), [0], 1.0, -1.0)
    with pytest.raises(ValueError):
        fb.collude_(torch.zeros(8, 4).t(), [0], 1.0, -1.0)  # not contiguous
    with pytest.raises(ValueError):
        fb.collude_(torch.zeros(8), [0], 1.0, -1.0)  # not 2-D
    with pytest.raises(ValueError, match="colluding"):
        collusion_coefficients("rev_grad", 7, 1, math.nan)
    x0 = make_data("randn", 4, 8, seed=1)
    y = x0.clone()
    ops.collude_(y, [], 1.0, -1.0)
    assert torch.equal(bits(y), bits(x0))
    ops.collude_(torch.zeros(4, 0), [1], 1.0, -1.0)  # d = 0: nothing to do
    # the send-boundary injection does not know the colluding modes, and says where
    for mode in COLLUDING_MODES:
        with pytest.raises(ValueError, match="collude_"):
            ops.inject_(torch.zeros(8), mode)
    with pytest.raises(ValueError):
        ops.inject_(torch.zeros(8), "no_such_mode")


# --------------------------------------------------------------- 4. attack definitions
def test_collusion_coefficients():
    assert COLLUDING_MODES == ("alie", "ipm")
    a, b = collusion_coefficients("alie", 7, 3, math.nan)
    assert a == 1.0 and abs(-b - 0.6745) <= 1e-4
    assert collusion_coefficients("alie", 8, 2, math.nan) == (1.0, 0.0)
    assert collusion_coefficients("alie", 2, 2, math.nan) == (1.0, 0.0)  # undefined: 0
    assert collusion_coefficients("alie", 8, 2, 1.5) == (1.0, -1.5)
    assert collusion_coefficients("alie", 7, 3, 0.25) == (1.0, -0.25)
    assert collusion_coefficients("ipm", 7, 1, math.nan) == (-0.1, 0.0)
    assert collusion_coefficients("ipm", 7, 1, 12.0) == (-12.0, 0.0)


# --------------------------------------------------------------- 5. config
def test_config_restrictions_and_cli():
    ok = dict(approach="baseline", mode="median", err_mode="alie", worker_fail=1)
    Config(**ok).sanity()
    assert math.isnan(Config().attack_param)
    for bad in (dict(approach="maj_vote", mode="maj_vote"), dict(approach="cyclic", mode="cyclic"),
                dict(topology="ps"), dict(health_timeout=5.0), dict(worker_fail=0)):
        for err_mode in COLLUDING_MODES:
            with pytest.raises(ValueError, match="colluding"):
                Config(**{**ok, "err_mode": err_mode, **bad}).sanity()
    Config(approach="maj_vote", err_mode="rev_grad").sanity()  # the others are untouched
    cfg = parse_cli(["--approach", "baseline", "--mode", "median", "--err-mode", "alie",
                     "--attack-param", "1.5", "--worker-fail", "1"])
    assert cfg.err_mode == "alie" and cfg.attack_param == 1.5
    cfg = parse_cli(["--approach", "baseline", "--err-mode", "ipm", "--worker-fail", "1"])
    assert math.isnan(cfg.attack_param)


# --------------------------------------------------------------- 6. aggregator algebra
P6, BYZ6 = 7, (2, 5)


def _agg_setup():
    torch.manual_seed(3)
    comm = Communicator(0, 1, torch.device("cpu"))
    model = nn.Sequential(nn.Linear(30, 7), nn.Linear(7, 4))
    space = FlatSpace(model, 1, torch.device("cpu"))
    g = torch.Generator().manual_seed(11)
    payload = torch.randn(P6, space.d_pad, generator=g)
    payload[:, space.d:] = 0.0
    return comm, space, payload


def test_aggregator_without_collusion_is_unchanged():
    comm, space, payload = _agg_setup()
    agg = TrimmedMeanAggregator(comm, space, num_workers=P6)
    assert agg.collusion is None
    before = payload.clone()
    recv = agg.exchanged(payload)
    assert torch.equal(bits(recv), bits(before))
    agg.collusion = Collusion(1.0, -1.0)  # attached, but no Byzantine row this step
    assert torch.equal(bits(agg.exchanged(payload)), bits(before))


@pytest.mark.parametrize("eps", [0.5, 12.0])
def test_plain_mean_under_ipm_is_scaled_honest_mean(eps):
    """mean over the exchange path (trim=0) with f rows at -eps*mu: exactly
    ((h - f*eps)/P) * mu_honest.  Allowed: the op's bound with that factor as the
    coefficient, 8*|(h - f*eps)/P|*P*u*M_j.  Worst case by the same summation model:
    the Byzantine rows are off by <= 2*eps*P*u*M_j each (f/P of it reaches the mean) and
    the P-term sum adds <= (P-1)*u*(h + f*eps)*M_j/P, one rounding for the division:
    eps=0.5 -> about 8 u*M_j of the 32 allowed, eps=12 -> about 74 of 152."""
    comm, space, payload = _agg_setup()
    agg = TrimmedMeanAggregator(comm, space, num_workers=P6, trim=0)
    agg.collusion = Collusion(-eps, 0.0, BYZ6)
    honest = [p for p in range(P6) if p not in BYZ6]
    H = payload[honest].double()
    out = agg.aggregate(payload.clone(), 0).double()
    h, f = len(honest), len(BYZ6)
    factor = (h - f * eps) / P6
    bound = 8.0 * abs(factor) * P6 * U * H.abs().amax(dim=0)
    err = (out - factor * H.mean(dim=0)).abs()
    print(f"eps={eps}: worst |error| / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}")
    assert bool((err <= bound).all())
    assert bool((out[space.d:] == 0).all())


@pytest.mark.parametrize("trim", [None, 2])
def test_envelope_survives_alie(trim):
    """f=2 of P=7 colluding at mu - sigma: the median and the trim=2 mean still lie
    inside the honest rows' [min, max] in every coordinate."""
    comm, space, payload = _agg_setup()
    agg = TrimmedMeanAggregator(comm, space, num_workers=P6, trim=trim)
    agg.collusion = Collusion(1.0, -1.0, BYZ6)
    honest = [p for p in range(P6) if p not in BYZ6]
    H = payload[honest][:, : space.d]
    work = payload.clone()
    out = agg.aggregate(work, 0)[: space.d]
    assert not torch.equal(work[2], payload[2]) and torch.equal(work[2], work[5])
    assert bool((out >= H.min(dim=0).values).all()) and bool((out <= H.max(dim=0).values).all())


# --------------------------------------------------------------- 7. training under IPM
def test_ipm_turns_the_mean_into_ascent_and_median_survives(tmp_path):
    """P=7, f=1, eps=12: h - f*eps = -6, so the plain mean is -6/7 of the honest mean,
    ascent by construction; the median is not moved past the honest values.  The only
    threshold is the run's own first loss."""
    from draco_amd.parallel import Trainer

    def run(mode):
        cfg = Config(network="LeNet", dataset="MNIST", batch_size=8, device="cpu", lr=0.05,
                     dtype="fp32", max_steps=100, eval_freq=0, log_dir="",
                     train_dir=str(tmp_path / "ckpt"), approach="baseline", mode=mode,
                     worker_fail=1, err_mode="ipm", attack_param=12.0, workers_per_rank=7)
        t = Trainer(cfg)
        t.logger.stdout_every = 0
        assert t.P == 7 and t.agg.collusion is not None
        assert (t.agg.collusion.a, t.agg.collusion.b) == (-12.0, 0.0)
        name = t.agg.name
        losses = [t.train_step()["loss"] for _ in range(40)]
        t.close()
        return name, losses

    name, mean_losses = run("normal")
    assert name == "mean"
    tail = float(np.mean(mean_losses[-5:]))
    print(f"normal: first {mean_losses[0]:.3f} last five {tail:.3f}")
    assert not tail < mean_losses[0]  # NaN counts
    name, med_losses = run("median")
    assert name == "median"
    tail = float(np.mean(med_losses[-5:]))
    print(f"median: first {med_losses[0]:.3f} last five {tail:.3f}")
    assert tail < med_losses[0]


def test_normal_mode_over_64_workers_names_the_limit(tmp_path):
    from draco_amd.parallel import Trainer

    cfg = Config(network="FC", dataset="MNIST", batch_size=4, device="cpu", max_steps=10,
                 eval_freq=0, log_dir="", train_dir=str(tmp_path / "ckpt"),
                 approach="baseline", mode="normal", worker_fail=1, err_mode="ipm",
                 workers_per_rank=65)
    with pytest.raises(ValueError, match="64"):
        Trainer(cfg)


# --------------------------------------------------------------- 8. sharding invariance
def _worker_grad(w, d):
    gen = torch.Generator().manual_seed(6000 + w)
    g = torch.randn(d, generator=gen)
    g[::5] = torch.randint(-2, 3, (len(g[::5]),), generator=gen).float()  # ties
    return g


def _decode(comm, world, rank, L):
    torch.manual_seed(7)
    model = nn.Linear(50, 10)
    space = FlatSpace(model, world, torch.device("cpu"))
    payload = space.alloc_payload(L)
    for l in range(L):
        payload[l, : space.d] = _worker_grad(l * world + rank, space.d)
    agg = TrimmedMeanAggregator(comm, space, num_workers=L * world)
    agg.collusion = Collusion(1.0, -1.0, (2,))  # logical worker 2, ALIE z=1
    return agg.aggregate(payload, step=0)[: space.d].clone()


def _shard_worker(rank, world, L):
    comm = Communicator(rank, world, torch.device("cpu"), backend="gloo")
    out = _decode(comm, world, rank, L)
    comm.shutdown()
    return out.numpy()


def test_sharded_decode_bit_equals_world1():
    """The overwrite is column-wise and order-fixed, the median too: P=4 logical workers
    as 2 ranks x 2 (recv row l*world + src = worker id) decode to the same bits as
    1 rank x 4, and the Byzantine worker's own gradient never reaches the output."""
    res = run_dist(_shard_worker, 2, 2)
    local = _decode(Communicator(0, 1, torch.device("cpu")), 1, 0, 4).numpy()
    for r in range(2):
        assert np.array_equal(res[r].view(np.int32), local.view(np.int32)), r
    d = local.shape[0]
    rows = torch.stack([_worker_grad(w, d) for w in range(4)])
    rows_pad = torch.cat([rows, torch.zeros(4, (-d) % 4)], dim=1).contiguous()
    fb.collude_(rows_pad, [2], 1.0, -1.0)
    ref = torch.empty(rows_pad.shape[1])
    fb.column_trimmed_mean(rows_pad, 1, 3, ref)
    assert np.array_equal(ref[:d].numpy().view(np.int32), local.view(np.int32))
