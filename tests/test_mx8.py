"""The MXFP8 block-scaled wire on the CPU: the ops' fallback against the numpy/fp64
definition of tests/mx8_util.py (exact), the error bound, the record layout, the aggregator
(one process and a world-2 gloo lane), what Config accepts and refuses, one training run."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.parallel import Communicator, FlatSpace, Trainer
from draco_amd.parallel import aggregators as A
from tests import mx8_util as U
from tests.dist_util import run_dist

CPU = torch.device("cpu")
BASE = dict(network="FC", dataset="MNIST", device="cpu", approach="baseline",
            mode="trimmed_mean", compress_grad="mx8", err_mode="rev_grad", worker_fail=1)


pack = U.pack


def test_decode_is_exact():
    rows = U.decode_case()
    out = torch.empty(len(rows), 64)
    ops.mx8_unpack(torch.from_numpy(rows), out)
    ref = torch.from_numpy(U.decode(rows, 64))
    assert U.same_values(out, ref)
    # the clamp at 10, the overflow and the NaN scale are in the case
    assert bool(torch.isinf(ref).any()) and bool(torch.isnan(ref[-4:]).all())
    assert torch.equal(ref[0], ref[8]) and float(ref[0, 1]) == 2.0 ** -126


def test_encode_is_exact():
    x = U.encode_case()
    assert np.array_equal(pack(ops, torch.from_numpy(x), 64).numpy(), U.encode(x, 64))


@pytest.mark.parametrize("n", [64, 192, 576])
def test_roundtrip_error_bound(n):
    x = U.random_case(n, seed=n)
    y = torch.empty(1, n)
    ops.mx8_unpack(pack(ops, x, n).view(1, -1), y)
    x64, err = x.double().view(-1, 32), (y.double().view(-1, 32) - x.double().view(-1, 32)).abs()
    scale = 2.0 ** (pack(ops, x, n)[n: n + n // 32].double() - 127)  # X = 2^e per block
    bound = torch.maximum(x64.abs() / 16, scale[:, None] / 1024)
    assert bool((err <= bound).all()) and bool((err > bound / 4).any())
    assert bool((scale < x64.abs().amax(1) / 224).all())


@pytest.mark.parametrize("chunk", [64, 576])
def test_slices_pack_to_records_and_padding_is_zero(chunk):
    cb = ops.mx8_chunk_bytes(chunk)
    assert cb == {64: 80, 576: 608}[chunk] == U.chunk_bytes(chunk)
    x = U.random_case(3 * chunk, seed=chunk, special=True)
    whole = pack(ops, x, chunk).view(3, cb)
    assert np.array_equal(whole.numpy().reshape(-1), U.encode(x.numpy(), chunk))
    for a, b in ((0, 1), (1, 3), (2, 3)):
        assert torch.equal(pack(ops, x[a * chunk: b * chunk], chunk), whole[a:b].reshape(-1))
    assert bool((whole[:, chunk + chunk // 32:] == 0).all()) and cb > chunk + chunk // 32


def _space_and_rows(world, P):
    torch.manual_seed(7)
    space = FlatSpace(nn.Linear(50, 10), world, CPU)  # d = 510: the pad tail is not empty
    rows = torch.zeros(P, space.d_pad)
    rows[:, : space.d] = torch.randn(P, space.d) * 2.0 ** torch.randint(-8, 8, (P, 1)).float()
    rows[0, 3] = float("nan")  # trimmed like any other extreme
    return space, rows


def _reference(space, rows):
    """The same rule on rows that went through decode(encode(.)) by the definition."""
    ref = torch.empty(space.d_pad)
    ops.column_trimmed_mean(U.roundtrip(rows, space.shard), 1, len(rows) - 1, ref)
    return ref


def _build(space, P, **kw):
    return A.build_baseline_aggregator(Config(**{**BASE, **kw}), Communicator(0, 1, CPU),
                                       space, P)


def test_aggregator_world1():
    space, rows = _space_and_rows(1, 7)
    agg = _build(space, 7)
    assert type(agg) is A.TrimmedMeanAggregator and agg.wire == "mx8"
    ref = _reference(space, rows)
    assert not U.same_values(ref, A.TrimmedMeanAggregator(
        Communicator(0, 1, CPU), space, num_workers=7, trim=1).aggregate(rows.clone(), 0))
    for _ in range(2):  # the second call reuses the buffers
        payload = rows.clone()
        agg.start_row(payload, 2)  # one row posted early
        assert U.same_values(agg.aggregate(payload, step=0), ref)
    assert space.d_pad > space.d and not bool(ref[space.d:].view(torch.int32).any())


def _gloo_worker(rank, world):
    L, (space, rows) = 2, _space_and_rows(world, 2 * world)
    comm = Communicator(rank, world, CPU, backend="gloo")
    agg = A.build_baseline_aggregator(Config(**BASE), comm, space, L * world)
    payload = rows[[l * world + rank for l in range(L)]].contiguous()
    ok = True
    for _ in range(2):
        agg.start_row(payload, 0)  # one row posted early, one left to aggregate()
        out = agg.aggregate(payload, step=0).clone()
        ok = ok and U.same_values(out, _reference(space, rows))
    comm.shutdown()
    return ok


def test_world2_gloo_equals_single_process_reference():
    assert all(run_dist(_gloo_worker, 2).values())


@pytest.mark.parametrize("comp,cls,name,wire", [
    ("mx8", A.TrimmedMeanAggregator, "mean", "mx8"), ("none", A.MeanAggregator, "mean", None),
    ("bf16", A.MeanAggregator, "mean", None)])
def test_builder_mode_normal(comp, cls, name, wire):
    space = _space_and_rows(1, 7)[0]
    agg = _build(space, 7, mode="normal", compress_grad=comp)
    assert type(agg) is cls and agg.name == name and agg.wire == wire
    if comp == "mx8":
        assert agg.trim == 0
        with pytest.raises(ValueError, match="64 workers"):
            _build(space, 65, mode="normal")


@pytest.mark.parametrize("kw,ok", [
    (dict(approach="maj_vote", mode="maj_vote"), False),
    (dict(approach="cyclic", mode="cyclic"), False),
    (dict(topology="ps"), False), (dict(health_timeout=5.0), False),
    (dict(err_mode="alie"), True), (dict(pre_aggregation="nnm"), True),
    (dict(worker_momentum=0.9, momentum=0.0), True),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_config_rejections_and_acceptances(kw, ok):
    cfg = Config(**{**BASE, **kw})
    if ok:
        cfg.sanity()
        assert _build(_space_and_rows(1, 7)[0], 7, **kw).wire == "mx8"
    else:
        with pytest.raises(ValueError, match="mx8"):
            cfg.sanity()


def test_host_rejections():
    f32, u8 = torch.zeros(128), torch.zeros(160, dtype=torch.uint8)
    for g, out, chunk in ((f32.double(), u8, 64), (f32, u8.int(), 64), (f32[:96], u8[:120], 96),
                          (f32, u8, 96), (f32, u8[:159], 64), (f32, u8, 128)):
        with pytest.raises(ValueError):
            ops.mx8_pack(g, out, chunk)
    for packed, out in ((u8.view(2, 80).int(), f32.view(2, 64)), (u8.view(2, 80), f32.view(1, 128)),
                        (u8.view(2, 80), f32.view(2, 64).double()), (u8[:120].view(1, 120), f32[:96].view(1, 96))):
        with pytest.raises(ValueError):
            ops.mx8_unpack(packed, out)
    ops.mx8_unpack(torch.zeros(0, 80, dtype=torch.uint8), torch.zeros(0, 64))  # P = 0


def test_training_descends_under_rev_grad(tmp_path):
    """LeNet, P=7, f=1, rev_grad, trimmed_mean, 40 steps, batch 32, lr 0.05, --momentum 0: the
    settings of the sign test's run.  The gap to the fp32 wire is recorded in
    profiles/convergence_mx8.md, not asserted."""
    t = Trainer(Config(**{**BASE, "network": "LeNet", "lr": 0.05, "momentum": 0.0,
                          "batch_size": 32, "dtype": "fp32", "max_steps": 50, "eval_freq": 0,
                          "log_dir": "", "train_dir": str(tmp_path), "workers_per_rank": 7}))
    t.logger.stdout_every = 0
    assert t.agg.wire == "mx8"
    losses = [t.train_step()["loss"] for _ in range(40)]
    t.close()
    assert losses[-1] < losses[0]
