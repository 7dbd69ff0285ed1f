"""signSGD with majority vote on the CPU: the ops' fallback against the int64 reference of
tests/sign_util.py (exact), the packed format's slice property, the aggregator (one process
and a world-2 gloo lane), what Config and the builder refuse, one short training run."""
import pytest
import torch
import torch.nn as nn

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.parallel import Communicator, FlatSpace, Trainer
from draco_amd.parallel import aggregators as A
from tests.dist_util import run_dist
from tests.sign_util import pack_rows, same_bits, sign_case, sign_ref

CPU = torch.device("cpu")
BASE = dict(network="FC", dataset="MNIST", device="cpu", approach="baseline", mode="normal",
            compress_grad="sign", err_mode="rev_grad", worker_fail=1)


@pytest.mark.parametrize("n", [64, 192, 320])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 7, 8, 64])
def test_fallback_equals_int64_reference(P, n):
    x = sign_case(P, n, seed=1000 * P + n)
    votes, ref = sign_ref(x)
    # the columns the vote can get wrong do occur: unanimous, all-abstain, ties
    assert bool((votes == -1).all(0).any()) and bool((votes == 0).all(0).any())
    assert P < 2 or bool(((votes != 0).any(0) & (votes.sum(0) == 0)).any())
    out = torch.full((n,), 9.0)
    ops.sign_majority(pack_rows(ops, x), out)
    assert same_bits(out, ref)  # +0.0 on ties, never -0.0


@pytest.mark.parametrize("a,b", [(0, 64), (64, 256), (128, 320)])
def test_packed_slice_is_slice_of_packed(a, b):
    x = sign_case(1, 320, seed=5)
    assert torch.equal(pack_rows(ops, x)[0, a // 16: b // 16],
                       pack_rows(ops, x[:, a:b].contiguous())[0])


def _space_and_rows(world, P):
    torch.manual_seed(7)
    space = FlatSpace(nn.Linear(50, 10), world, CPU)  # d = 510: the pad tail is not empty
    rows = torch.zeros(P, space.d_pad)
    rows[:, : space.d] = sign_case(P, space.d, seed=P)
    return space, rows


def _build(space, P, **kw):
    return A.build_baseline_aggregator(Config(**{**BASE, **kw}), Communicator(0, 1, CPU),
                                       space, P)


def test_builder_and_aggregator_world1():
    space, rows = _space_and_rows(1, 7)
    with pytest.raises(ValueError, match="at most 64"):
        _build(space, 65)
    for comp in ("none", "bf16"):  # unchanged defaults
        Config(**{**BASE, "compress_grad": comp}).sanity()
        assert type(_build(space, 7, compress_grad=comp)) is A.MeanAggregator
    agg = _build(space, 7)
    assert type(agg) is A.SignMajorityAggregator and agg.name == "sign_majority"
    for _ in range(2):  # the second call reuses the send buffer
        out = agg.aggregate(rows.clone(), step=0)
        assert same_bits(out, sign_ref(rows)[1])
    assert space.d_pad > space.d and same_bits(out[space.d:], torch.zeros(2))


def _gloo_worker(rank, world):
    L, (space, rows) = 2, _space_and_rows(world, 2 * world)
    comm = Communicator(rank, world, CPU, backend="gloo")
    agg = A.SignMajorityAggregator(comm, space, num_workers=L * world)
    payload = rows[[l * world + rank for l in range(L)]].contiguous()
    agg.start_row(payload, 0)  # one row posted early, one left to aggregate()
    out = agg.aggregate(payload, step=0).clone()
    comm.shutdown()
    return same_bits(out, sign_ref(rows)[1])


def test_world2_gloo_equals_single_process_reference():
    assert all(run_dist(_gloo_worker, 2).values())


@pytest.mark.parametrize("kw", [
    dict(approach="maj_vote", mode="maj_vote"), dict(approach="cyclic", mode="cyclic"),
    dict(mode="median"), dict(topology="ps"), dict(health_timeout=5.0),
    dict(err_mode="alie"), dict(err_mode="ipm"), dict(pre_aggregation="nnm"),
    dict(worker_momentum=0.9),  # Signum is accepted, its --momentum 0 rule unchanged
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_config_and_builder_rejections(kw):
    with pytest.raises(ValueError):
        Config(**{**BASE, **kw}).sanity()
    if "worker_momentum" in kw:
        Config(**{**BASE, **kw, "momentum": 0.0}).sanity()
    elif set(kw) <= {"mode", "err_mode", "pre_aggregation"}:
        with pytest.raises(ValueError):
            _build(_space_and_rows(1, 7)[0], 7, **kw)


def test_training_under_rev_grad_descends_where_the_mean_does_not(tmp_path):
    """LeNet, P=7, f=1, rev_grad, 40 steps, batch 32, --momentum 0; lr 0.001 under the sign
    wire and 0.05 for the plain mean: the settings (and step count) of the rev_grad row of
    profiles/convergence_sign_majority.md (tools/convergence_sign.py)."""
    losses = {}
    for comp, lr in (("sign", 0.001), ("none", 0.05)):
        t = Trainer(Config(**{**BASE, "network": "LeNet", "compress_grad": comp, "lr": lr,
                              "momentum": 0.0, "batch_size": 32, "dtype": "fp32",
                              "max_steps": 50, "eval_freq": 0, "log_dir": "",
                              "train_dir": str(tmp_path), "workers_per_rank": 7}))
        t.logger.stdout_every = 0
        losses[comp] = [t.train_step()["loss"] for _ in range(40)]
        t.close()
    assert losses["sign"][-1] < losses["sign"][0]
    assert not losses["none"][-1] < losses["none"][0]
