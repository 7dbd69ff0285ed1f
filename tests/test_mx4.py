"""The MXFP4 block-scaled wire on the CPU: the ops' fallback against the numpy/fp64 statement
of tests/mx4_util.py (exact, both roundings), the error bounds, the missing bias of the
stochastic rounding, the aggregator (one process and a world-2 gloo lane), what Config refuses."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.ops import fallback as fb
from draco_amd.parallel import Communicator, FlatSpace, Trainer
from draco_amd.parallel import aggregators as A
from tests import mx4_util as U
from tests.dist_util import run_dist

CPU = torch.device("cpu")
BASE = dict(network="FC", dataset="MNIST", device="cpu", approach="baseline", mode="trimmed_mean",
            compress_grad="mx4", mx_rounding="nearest", worker_fail=1, eval_freq=0, log_dir="",
            train_dir="")


@pytest.mark.parametrize("seed", [None, 0, 2 ** 64 - 3])
def test_encode_is_exact(seed):
    x = U.encode_case()
    got = U.pack(ops, torch.from_numpy(x), 64, seed).numpy()
    assert np.array_equal(got, U.encode(x, 64, seed))
    scales = got.reshape(-1, 48)[:, 32:34]
    assert {2, 127, 253, 255} <= set(scales.reshape(-1).tolist()) and ops.mx4_chunk_bytes(576) == 320


def test_decode_is_exact():
    rows = U.decode_case()
    out = torch.empty(len(rows), 64)
    ops.mx4_unpack(torch.from_numpy(rows), out)
    ref = torch.from_numpy(U.decode(rows, 64))
    assert U.same_values(out, ref)
    # the clamp at 2, the overflow and the NaN scale are in the case
    assert torch.equal(ref[0], ref[2]) and float(ref[0, 2]) == 2.0 ** -126
    assert bool(torch.isinf(ref[6]).any()) and bool(torch.isnan(ref[7]).all())


def _roundtrip(x, seed):
    n, y = x.numel(), torch.empty(1, x.numel())
    packed = U.pack(ops, x, n, seed)
    ops.mx4_unpack(packed.view(1, -1), y)
    scale = 2.0 ** (packed[n // 2: n // 2 + n // 32].double() - 127)  # X = 2^e per block
    return x.double().view(-1, 32), y.double().view(-1, 32), scale[:, None]


def test_error_bounds():
    x = U.random_case(4096, seed=1, span=20)
    x64, y, X = _roundtrip(x, None)
    assert bool(((y - x64).abs() <= torch.maximum(x64.abs() / 4, X / 4)).all())
    assert bool((X < x64.abs().amax(1, keepdim=True) / 3).all())
    x64, y, X = _roundtrip(x, 11)
    t = x64.abs() / X
    step = X * torch.where(t < 2, 0.5, torch.where(t < 4, 1.0, 2.0))
    assert bool(((y - x64).abs() < step).all()) and bool(((y - x64).abs() > step / 2).any())


def test_stochastic_rounding_has_no_bias():
    """K seeds, n = 64: the mean decoded value within 6 standard errors of x, a standard
    error being at most step / (2 sqrt(K)) (a two-point variable on [lo, lo + step])."""
    K, x = 4096, U.random_case(64, seed=2, span=20)
    total, y = torch.zeros(64, dtype=torch.float64), torch.empty(1, 64)
    for seed in range(K):
        fb.mx4_unpack(U.pack(fb, x, 64, seed * 0x9E3779B97F4A7C15).view(1, -1), y)
        total += y[0].double()
    x64, _, X = _roundtrip(x, None)
    t = x64.abs() / X
    step = X * torch.where(t < 2, 0.5, torch.where(t < 4, 1.0, 2.0))
    worst = ((total.view(-1, 32) / K - x64).abs() / (step / (2 * K ** 0.5))).max()
    print(f"worst bias: {float(worst):.2f} standard errors")
    assert float(worst) <= 6.0
    a, b = U.pack(ops, x, 64, 5), U.pack(ops, x, 64, 6)
    assert not torch.equal(a, b) and torch.equal(a, U.pack(ops, x, 64, 5))


def test_trainer_aggregates_the_roundtripped_rows():
    t = Trainer(Config(**{**BASE, "workers_per_rank": 7}))
    assert t.agg.wire == "mx4" and type(t.agg) is A.TrimmedMeanAggregator
    rows = torch.zeros(7, t.space.d_pad)
    rows[:, : t.space.d] = U.random_case(7 * 32 * (t.space.d // 32 + 1), seed=5, span=8).view(
        7, -1)[:, : t.space.d]
    t.payload.copy_(rows)
    out = t.agg.aggregate(t.payload, step=0).clone()
    t.close()
    ref = torch.empty_like(out)
    fb.column_trimmed_mean(U.roundtrip(rows, rows.shape[1]), 1, 6, ref)
    assert torch.equal(out, ref)


def _space_and_rows(world, P):
    torch.manual_seed(7)
    space = FlatSpace(nn.Linear(50, 10), world, CPU)  # d = 510: the pad tail is not empty
    rows = torch.zeros(P, space.d_pad)
    rows[:, : space.d] = torch.randn(P, space.d) * 2.0 ** torch.randint(-8, 8, (P, 1)).float()
    rows[0, 3] = float("nan")  # costs row 0 a block, trimmed like any other extreme
    ref = torch.empty(space.d_pad)
    ops.column_trimmed_mean(U.roundtrip(rows, space.shard), 1, P - 1, ref)
    return space, rows, ref


def _gloo_worker(rank, world):
    L, (space, rows, ref) = 2, _space_and_rows(world, 2 * world)
    comm = Communicator(rank, world, CPU, backend="gloo")
    agg = A.build_baseline_aggregator(Config(**BASE), comm, space, L * world)
    payload = rows[[l * world + rank for l in range(L)]].contiguous()
    ok = agg.wire == "mx4"
    for _ in range(2):
        agg.start_row(payload, 0)  # one row posted early, one left to aggregate()
        ok = ok and U.same_values(agg.aggregate(payload, step=0).clone(), ref)
    comm.shutdown()
    return ok


def test_world2_gloo_equals_single_process_reference():
    assert all(run_dist(_gloo_worker, 2).values())


def test_builder_mode_normal_and_seeds():
    space = _space_and_rows(1, 7)[0]
    build = lambda **kw: A.build_baseline_aggregator(  # noqa: E731
        Config(**{**BASE, **kw}), Communicator(0, 1, CPU), space, 7)
    agg = build(mode="normal")
    assert type(agg) is A.TrimmedMeanAggregator and (agg.name, agg.trim, agg.wire) == ("mean", 0, "mx4")
    assert agg.wire_seed is None and agg.exchanged_packed(torch.zeros(7, space.d_pad)) is None
    with pytest.raises(ValueError, match="compress-grad mx4.*64 workers"):
        A.build_baseline_aggregator(Config(**{**BASE, "mode": "normal"}), Communicator(0, 1, CPU),
                                    space, 65)
    agg = build(mx_rounding="stochastic", seed=9)
    assert [agg._row_seed() for _ in range(3)] == [9 << 32, 9 << 32 | 1, 9 << 32 | 2]


@pytest.mark.parametrize("kw", [
    dict(approach="maj_vote", mode="maj_vote"), dict(approach="cyclic", mode="cyclic"),
    dict(topology="ps"), dict(health_timeout=5.0), dict(mx_rounding="up"),
    dict(compress_grad="mx8"), dict(compress_grad="none")],
    ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()))
def test_config_rejections(kw):
    Config(**BASE).sanity()
    Config(**{**BASE, "mx_rounding": "stochastic", "err_mode": "alie"}).sanity()
    with pytest.raises(ValueError, match="mx4|mx-rounding"):
        Config(**{**BASE, **kw}).sanity()
