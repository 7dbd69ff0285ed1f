"""Worker-side momentum (arXiv:2012.10333) on the CPU: ops.worker_momentum_'s definition
against the fp64 oracle, the non-finite rule, the trainer's recurrence on all three send
paths, the sidecar checkpoint, and the public interface.  Oracle, bound and its
derivation: tests/worker_momentum_util.py.
"""
import glob
import json
import os

import numpy as np
import pytest
import torch

from draco_amd import ops
from draco_amd.config import Config, parse_cli
from draco_amd.ops import fallback as fb
from tests.dist_util import run_dist
from tests.worker_momentum_util import (NONFINITE, bits, check_first, check_update, make_pair,
                                        oracle)


# --------------------------------------------------------------- 1. the op's definition
@pytest.mark.parametrize("beta", [0.5, 0.9, 0.99])
def test_fallback_within_bound_of_fp64_oracle(beta):
    g0, m0 = make_pair(4096, seed=int(beta * 100))
    g, m = g0.clone(), m0.clone()
    ops.worker_momentum_(g, m, beta, False)
    check_update(g0, m0, g, m, beta, f"fallback beta={beta}")
    # the dispatch on CPU tensors IS the fallback
    g2, m2 = g0.clone(), m0.clone()
    fb.worker_momentum_(g2, m2, beta, False)
    assert torch.equal(bits(g2), bits(g)) and torch.equal(bits(m2), bits(m))
    # first step: a bit copy, g untouched, whatever m held
    g, m = g0.clone(), m0.clone()
    ops.worker_momentum_(g, m, beta, True)
    check_first(g0, g, m, f"fallback first beta={beta}")


def test_dyadic_beta_is_exact():
    g0 = torch.tensor([1.0, -3.0, 0.5, 8.0])
    m0 = torch.tensor([3.0, 1.0, -0.5, 0.0])
    g, m = g0.clone(), m0.clone()
    ops.worker_momentum_(g, m, 0.5, False)
    assert m.tolist() == [2.0, -1.0, 0.0, 4.0] and g.tolist() == m.tolist()
    sent, exact = oracle(g0, m0, 0.5, False)
    assert sent.tolist() == exact.tolist() == m.tolist()


@pytest.mark.parametrize("first", [False, True])
def test_nonfinite_gradient_does_not_reach_the_state(first):
    n = 64
    g0, m0 = make_pair(n, seed=7)
    plants = {0: NONFINITE[0], 5: NONFINITE[1], 6: NONFINITE[2], n - 1: NONFINITE[0]}
    gp = g0.clone()
    for i, v in plants.items():
        gp[i] = v
    g, m = gp.clone(), m0.clone()
    ops.worker_momentum_(g, m, 0.9, first)
    idx = torch.tensor(sorted(plants))
    keep = torch.ones(n, dtype=torch.bool)
    keep[idx] = False
    # the sent element is g's own bits
    assert torch.equal(bits(g)[idx], bits(gp)[idx])
    if first:
        check_first(gp, g, m, "planted first")
        assert bool((bits(m)[idx] == 0).all())
    else:
        check_update(gp, m0, g, m, 0.9, "planted")
        assert torch.equal(bits(m)[idx], bits(m0)[idx])
    # every other element is what it is without the plants
    gc, mc = g0.clone(), m0.clone()
    ops.worker_momentum_(gc, mc, 0.9, first)
    assert torch.equal(bits(g)[keep], bits(gc)[keep])
    assert torch.equal(bits(m)[keep], bits(mc)[keep])
    assert bool(torch.isfinite(m).all())


def test_fallback_rejects_bad_arguments():
    g, m = torch.zeros(8), torch.zeros(8)
    with pytest.raises(ValueError, match="fp32"):
        fb.worker_momentum_(g.double(), m, 0.9, False)
    with pytest.raises(ValueError, match="contiguous"):
        fb.worker_momentum_(torch.zeros(16)[::2], m, 0.9, False)
    with pytest.raises(ValueError, match="multiple of 4"):
        fb.worker_momentum_(torch.zeros(6), torch.zeros(6), 0.9, False)
    with pytest.raises(ValueError, match="length"):
        fb.worker_momentum_(g, torch.zeros(12), 0.9, False)
    for beta in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="beta"):
            fb.worker_momentum_(g, m, beta, False)
    e = torch.zeros(0)
    fb.worker_momentum_(e, e.clone(), 0.9, False)  # nothing to do
    assert "worker_momentum_" in ops.__all__


# --------------------------------------------------------------- 2. the trainer
def _lenet_cfg(tmp_path, **kw):
    base = dict(network="LeNet", dataset="MNIST", batch_size=8, device="cpu", lr=0.05,
                dtype="fp32", max_steps=100, eval_freq=0, log_dir="",
                train_dir=str(tmp_path / "ckpt"), approach="baseline", mode="median",
                worker_fail=1, err_mode="rev_grad", workers_per_rank=4, momentum=0.0)
    base.update(kw)
    return Config(**base)


def _spy_trainer(cfg, monkeypatch=None):
    """Trainer whose aggregate() records the payload it is handed and whose
    ops.worker_momentum_ calls record the raw gradient they are handed."""
    from draco_amd.parallel import trainer as trainer_mod

    t = trainer_mod.Trainer(cfg)
    t.logger.stdout_every = 0
    t.sent, t.raw = [], []
    inner = t.agg.aggregate

    def aggregate(payload, step):
        t.sent.append(payload.clone())
        return inner(payload, step)

    t.agg.aggregate = aggregate
    if monkeypatch is not None:
        op = trainer_mod.ops.worker_momentum_

        def worker_momentum_(g, m, beta, first):
            t.raw.append((g.clone(), bool(first)))
            op(g, m, beta, first)

        monkeypatch.setattr(trainer_mod.ops, "worker_momentum_", worker_momentum_)
    return t


def test_trainer_sends_the_momentum_recurrence(tmp_path, monkeypatch):
    """LeNet / synthetic MNIST, one process hosting P=4 workers, median, one rev_grad
    worker per step, beta=0.9, 3 steps.  The first step sends m = g, so its median and
    the parameters after it are those of the beta=0 run: steps 1 and 2 see the beta=0
    run's gradients bit for bit; later steps are checked through the recurrence on the
    gradients the op was handed."""
    beta, steps, L = 0.9, 3, 4
    t0 = _spy_trainer(_lenet_cfg(tmp_path))
    assert t0.wm is None
    for _ in range(2):
        t0.train_step()
    t = _spy_trainer(_lenet_cfg(tmp_path, worker_momentum=beta), monkeypatch)
    assert t.wm.state.shape == (L, t.space.d_pad) and t.wm.first == [True] * L
    prev = None
    for s in range(steps):
        t.train_step()
        raw = t.raw[s * L:(s + 1) * L]
        assert len(raw) == L and all(first == (s == 0) for _, first in raw)
        byz = sorted(t.schedule.adversaries_at(s))
        assert len(byz) == 1
        if s < 2:  # same parameters as the beta=0 run: same honest gradients
            for l in range(L):
                if l not in byz:
                    assert torch.equal(bits(raw[l][0]), bits(t0.sent[s][l])), (s, l)
        for l in range(L):
            g_raw = raw[l][0]
            assert bool(torch.isfinite(g_raw).all()) and bool(g_raw.abs().max() > 0)
            if s == 0:
                assert torch.equal(bits(t.wm.state[l]), bits(g_raw))
            else:
                # the state is honest in EVERY slot, the Byzantine one included
                check_update(g_raw, prev[l], t.wm.state[l], t.wm.state[l], beta, f"step {s} slot {l}")
            if l in byz:
                assert torch.equal(bits(t.sent[s][l]), bits(t.wm.state[l] * fb.ADVERSARY_)), (s, l)
            else:
                assert torch.equal(bits(t.sent[s][l]), bits(t.wm.state[l])), (s, l)
        prev = t.wm.state.clone()
    assert t.wm.first == [False] * L
    # what step 2 sends is the momenta, not the beta=0 run's gradients
    assert not torch.equal(t.sent[1], t0.sent[1])
    t.close()
    t0.close()


def test_beta_zero_changes_nothing(tmp_path):
    out = []
    for kw in (dict(), dict(worker_momentum=0.0)):
        t = _spy_trainer(_lenet_cfg(tmp_path, momentum=0.5, **kw))
        assert t.wm is None
        for _ in range(3):
            t.train_step()
        out.append(t.space.flat_param.clone())
        t.save()
        t.close()
    assert torch.equal(bits(out[0]), bits(out[1]))
    assert sorted(os.listdir(str(tmp_path / "ckpt"))) == ["model_step_3"]


# --------------------------------------------------------------- 3. bucketed == whole-row
def _bucket_worker(rank, world, mode, worker_fail):
    from draco_amd.parallel.trainer import Trainer

    out = {}
    for bucket_mb in (0.0, 0.01):
        cfg = Config(network="LeNet", dataset="MNIST", batch_size=4, device="cpu", lr=0.05,
                     dtype="fp32", approach="baseline", mode=mode, err_mode="rev_grad",
                     worker_fail=worker_fail, workers_per_rank=2, momentum=0.0,
                     worker_momentum=0.9, max_steps=50, eval_freq=0, log_dir="",
                     train_dir="/tmp/draco_wm_bkt", bucket_mb=bucket_mb)
        t = Trainer(cfg)
        t.logger.stdout_every = 0
        assert t.use_buckets == (bucket_mb > 0), "bucketed path did not activate"
        if bucket_mb > 0:
            assert len(t._buckets) >= 2, "LeNet should split into several buckets"
        for s in range(3):
            t.train_step()
            assert t.wm.first == [False, False]
        out[bucket_mb] = (t.space.flat_param.clone(), t.wm.state.clone())
        t.close()
    for a, b in zip(out[0.0], out[0.01]):
        assert torch.equal(bits(a), bits(b)), float((a - b).abs().max())
    assert bool(torch.isfinite(out[0.0][0]).all()) and bool(out[0.0][1].abs().max() > 0)
    return True


@pytest.mark.parametrize("mode,worker_fail", [("normal", 0), ("trimmed_mean", 1)])
def test_bucketed_equals_whole_row(mode, worker_fail):
    # normal: MeanAggregator.start_bucket all-reduces the payload slice in place (world
    # = 2: both paths sum in the same order); trimmed_mean: the exchange path, with the
    # per-chunk injection after the per-chunk momentum
    run_dist(_bucket_worker, 2, mode, worker_fail)


# --------------------------------------------------------------- 4. checkpoint
def test_checkpoint_round_trip(tmp_path):
    def trainer(**kw):
        t = _spy_trainer(_lenet_cfg(tmp_path, worker_momentum=0.9, **kw))
        return t

    t = trainer(eval_freq=2)
    losses = [t.train_step()["loss"] for _ in range(4)]  # saves after steps 2 and 4
    ref_param, ref_wm = t.space.flat_param.clone(), t.wm.state.clone()
    t.close()
    ckpt = str(tmp_path / "ckpt")
    side = os.path.join(ckpt, "worker_momentum_step_2.rank0")
    assert os.path.exists(side)
    # evaluate.py globs model_step_* and parses the tail as the step number
    mains = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ckpt, "model_step_*")))
    assert mains == ["model_step_2", "model_step_4"]
    assert not glob.glob(os.path.join(ckpt, "*.tmp"))
    state = torch.load(side, map_location="cpu", weights_only=False)
    assert state["beta"] == 0.9 and state["world"] == 1 and state["L"] == 4
    assert state["first"] == [False] * 4 and len(state["rows"]) == 4

    t = trainer(checkpoint_step=2)
    assert t.wm.first == [False] * 4
    resumed = [t.train_step()["loss"] for _ in range(2)]
    assert resumed == losses[2:]
    assert torch.equal(bits(t.space.flat_param), bits(ref_param))
    assert torch.equal(bits(t.wm.state), bits(ref_wm))
    t.close()

    # sidecar of another worker layout, then no sidecar: every slot starts over
    logs = tmp_path / "logs"
    state["L"] = 2
    torch.save(state, side)
    for k, remove in enumerate((False, True)):
        if remove:
            os.remove(side)
        t = trainer(checkpoint_step=2, log_dir=str(logs))
        assert t.wm.first == [True] * 4 and not bool(t.wm.state.any())
        again = [t.train_step()["loss"] for _ in range(2)]
        assert np.isfinite(again).all() and t.skipped_updates == 0
        assert t.wm.first == [False] * 4
        t.close()
        with open(logs / "rank0.jsonl") as fh:
            events = [json.loads(line) for line in fh]
        restarts = [e for e in events if e.get("event") == "worker_momentum_restart"]
        assert len(restarts) == k + 1 and restarts[-1]["step"] == 2


# --------------------------------------------------------------- 5. public interface
def _sane(**kw):
    base = dict(approach="baseline", mode="median", worker_momentum=0.9, momentum=0.0)
    base.update(kw)
    Config(**base).sanity()


@pytest.mark.parametrize("kw", [
    dict(worker_momentum=1.0),
    dict(worker_momentum=-0.1),
    dict(worker_momentum=float("nan")),
    dict(approach="maj_vote", mode="maj_vote"),
    dict(approach="cyclic", mode="cyclic"),
    dict(topology="ps"),
    dict(health_timeout=5.0),
    dict(momentum=0.5),
    dict(optimizer="sgd", momentum=0.9),
])
def test_sanity_rejections_name_the_flag(kw):
    with pytest.raises(ValueError, match="worker-momentum"):
        _sane(**kw)


def test_sanity_accepts_and_cli_parses():
    _sane()
    _sane(optimizer="adam", momentum=0.5)  # Adam has no --momentum to stack on
    _sane(err_mode="alie", worker_fail=1)
    with pytest.raises(ValueError, match="--momentum 0"):
        _sane(momentum=0.5)
    Config(approach="maj_vote", topology="ps", health_timeout=0.0).sanity()  # 0 = off
    assert Config().worker_momentum == 0.0
    cfg = parse_cli(["--worker-momentum", "0.9", "--momentum", "0", "--approach", "baseline",
                     "--mode", "centered_clip"])
    assert cfg.worker_momentum == 0.9 and cfg.momentum == 0.0
    with pytest.raises(ValueError, match="worker-momentum"):
        parse_cli(["--worker-momentum", "0.9", "--approach", "baseline"])  # momentum 0.5
