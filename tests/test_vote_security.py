"""Adversary-model tests for the tolerance vote (VoteAggregator).

The GPU vote is tolerance-based (MIOpen backward is not bitwise-reproducible), which
relaxes the adversary model: a perturbation INSIDE the equality ball passes the vote.
These tests pin down exactly what that buys an adversary:
  * row granularity: worst-case aggregate bias == the ball radius
    (atol + rtol * max|g|), no more — measured, not asserted;
  * segment granularity: the same row-ball adversary is EXCLUDED (its perturbation
    exceeds the per-tensor ball on small segments), so the reachable bias shrinks to
    rtol * max|g_seg| per tensor;
  * end-to-end: training under a persistent within-tolerance adversary still tracks
    the clean loss curve (gloo, world 3).
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from draco_amd.parallel.aggregators import VoteAggregator
from draco_amd.parallel.comm import Communicator
from draco_amd.parallel.flat import FlatSpace
from tests.dist_util import run_dist


def _single_comm():
    return Communicator(0, 1, torch.device("cpu"))


class TwoScale(nn.Module):
    """Two parameter tensors with very different magnitudes (a late bias vs a big
    conv): the case where the row-level ball is orders of magnitude too generous."""

    def __init__(self):
        super().__init__()
        self.big = nn.Parameter(torch.empty(1000))
        self.small = nn.Parameter(torch.empty(20))


def _payload(space, rtol, adversary_member, granularity_scale="row"):
    """3-member group: honest gradient g in members (with tiny replica noise), the
    chosen member replaced by g + 0.99 * ball * sign-noise."""
    torch.manual_seed(0)
    g = torch.zeros(space.d_pad)
    g[:1000] = torch.randn(1000) * 50.0   # big segment, |.| ~ 200 max
    g[1000:1020] = torch.randn(20) * 0.01  # small segment, |.| ~ 0.03 max
    payload = space.alloc_payload(3)
    for m in range(3):
        noise = torch.randn(space.d_pad) * 1e-6
        payload[m] = g + noise
    ball = rtol * float(g.abs().max())
    sign = torch.sign(torch.randn(space.d_pad))
    payload[adversary_member] = g + 0.99 * ball * sign
    return payload, g, ball


def test_row_ball_bias_is_bounded_by_ball_radius():
    """Worst case for the row vote: the adversary sits at the first member slot (the
    deterministic tie-break winner) with a just-inside-ball perturbation.  It WINS
    the vote — and the resulting bias equals the ball radius, never more.  This is
    the measured version of the README's 'shift <= tol' claim."""
    comm = _single_comm()
    model = TwoScale()
    space = FlatSpace(model, 1, torch.device("cpu"))
    rtol = 0.1
    agg = VoteAggregator(comm, space, group_size=3, rtol=rtol,
                         member_rows=np.array([[0, 1, 2]]))
    payload, g, ball = _payload(space, rtol, adversary_member=0)
    out = agg.aggregate(payload, step=0)
    bias = (out - g).abs().max()
    assert float(bias) > 0.5 * ball, "adversary should have won the tie-break"
    assert float(bias) <= 1.0 * ball + 1e-5, f"bias {float(bias)} exceeds ball {ball}"
    # the small segment got poisoned by the BIG segment's scale: bias there is huge
    # relative to its own magnitude — the weakness segment granularity closes
    small_bias = (out[1000:1020] - g[1000:1020]).abs().max()
    assert float(small_bias) > 100 * float(g[1000:1020].abs().max())


def test_segment_granularity_excludes_row_ball_adversary():
    """The same adversary under granularity='segment': its row-level perturbation
    violates the small tensor's per-segment ball, the pairs with it go unequal, the
    honest pair wins, and the aggregate tracks the honest gradient."""
    comm = _single_comm()
    model = TwoScale()
    space = FlatSpace(model, 1, torch.device("cpu"))
    rtol = 0.1
    agg = VoteAggregator(comm, space, group_size=3, rtol=rtol,
                         member_rows=np.array([[0, 1, 2]]), granularity="segment")
    payload, g, ball = _payload(space, rtol, adversary_member=0)
    out = agg.aggregate(payload, step=0)
    bias = (out - g).abs().max()
    assert float(bias) < 1e-4, f"segment vote failed to exclude the adversary ({float(bias)})"


def test_segment_granularity_admits_honest_noise():
    """Per-segment thresholds must not break the honest case: replica noise scaled
    to each segment's own magnitude still votes equal."""
    comm = _single_comm()
    model = TwoScale()
    space = FlatSpace(model, 1, torch.device("cpu"))
    agg = VoteAggregator(comm, space, group_size=3, rtol=0.1,
                         member_rows=np.array([[0, 1, 2]]), granularity="segment")
    torch.manual_seed(3)
    g = torch.randn(space.d_pad)
    g[1000:1020] *= 0.01
    payload = space.alloc_payload(3)
    seg_scale = torch.ones(space.d_pad)
    seg_scale[1000:1020] = 0.01
    for m in range(3):
        payload[m] = g + torch.randn(space.d_pad) * 1e-4 * seg_scale
    out = agg.aggregate(payload, step=0)
    assert agg.degenerate_steps == 0
    assert float((out - g).abs().max()) < 1e-3


def _within_tol_train_worker(rank, world, err_mode, granularity="row"):
    from draco_amd.config import Config
    from draco_amd.parallel.trainer import Trainer

    cfg = Config(network="FC", dataset="MNIST", batch_size=8, device="cpu", lr=0.05,
                 approach="maj_vote", mode="maj_vote", group_size=3, worker_fail=1,
                 err_mode=err_mode, vote_rtol=0.1, vote_granularity=granularity,
                 max_steps=100, eval_freq=0,
                 log_dir="", train_dir="/tmp/draco_wt", bucket_mb=0)
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    losses = [t.train_step()["loss"] for _ in range(30)]
    h = float(t.space.flat_param.double().sum())
    t.close()
    return losses, h


def test_training_tracks_clean_under_within_tol_attack():
    """A persistent within-tolerance adversary (passes the vote every step) must not
    prevent convergence: final loss tracks the clean run within a modest margin."""
    attacked = run_dist(_within_tol_train_worker, 3, "within_tol")
    clean = run_dist(_within_tol_train_worker, 3, "none")
    assert attacked[0][1] == attacked[1][1] == attacked[2][1], "params diverged"
    la, lc = attacked[0][0], clean[0][0]
    assert la[-1] < la[0], "attacked run failed to converge at all"
    assert la[-1] < lc[-1] + 0.3, f"attacked {la[-1]:.3f} vs clean {lc[-1]:.3f}"


def test_segment_vote_neutralizes_within_tol_attack_e2e():
    """Under granularity='segment' the row-ball adversary violates small tensors'
    per-segment balls and loses every vote: the attacked trajectory should hug the
    clean one much tighter than under the row vote."""
    attacked = run_dist(_within_tol_train_worker, 3, "within_tol", "segment")
    clean = run_dist(_within_tol_train_worker, 3, "none", "segment")
    la, lc = attacked[0][0], clean[0][0]
    assert attacked[0][1] == attacked[1][1] == attacked[2][1]
    assert abs(la[-1] - lc[-1]) < 0.1, f"attacked {la[-1]:.3f} vs clean {lc[-1]:.3f}"


# ------------------------------------------------------------- non-finite adversaries
NONFINITE = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def nonfinite_vote_case(device, granularity, rtol, bad_slots, bad, plant):
    """One 3-member group (atol=1e-3) whose members all hold the same honest g, then
    the members in `bad_slots` get `bad` planted at element 7 or over the whole row.
    Shared with the on-device run in tests/test_kernels_gpu_edges.py."""
    device = torch.device(device)
    comm = Communicator(0, 1, device)
    space = FlatSpace(TwoScale(), 1, device)
    agg = VoteAggregator(comm, space, group_size=3, atol=1e-3, rtol=rtol,
                         member_rows=np.array([[0, 1, 2]]), granularity=granularity)
    gen = torch.Generator().manual_seed(0)
    g = torch.zeros(space.d_pad)
    g[:1000] = torch.randn(1000, generator=gen) * 50.0
    g[1000:1020] = torch.randn(20, generator=gen) * 0.01
    g = g.to(device)
    payload = space.alloc_payload(3)
    payload[:] = g
    for slot in bad_slots:
        if plant == "element":
            payload[slot, 7] = bad
        else:
            payload[slot, :] = bad
    out = agg.aggregate(payload, step=0)
    return out, g, agg


NONFINITE_GRID = [
    pytest.param(gran, rtol, bad, plant, slot, id=f"{gran}-rtol{rtol}-{bad}-{plant}-slot{slot}")
    for gran in ("row", "segment") for rtol in (0.0, 0.1) for bad in NONFINITE
    for plant in ("element", "row") for slot in (0, 2)
]


@pytest.mark.parametrize("granularity,rtol,bad,plant,slot", NONFINITE_GRID)
def test_nonfinite_adversary_loses_the_vote(granularity, rtol, bad, plant, slot):
    """A member holding any NaN/+Inf/-Inf is outside every ball: the two honest
    members form the majority class even when the adversary sits in slot 0 (the
    tie-break winner), with rtol > 0 (thresh = atol + rtol*inf = inf must not admit
    it) and under both granularities."""
    out, g, agg = nonfinite_vote_case("cpu", granularity, rtol, [slot], NONFINITE[bad], plant)
    assert torch.isfinite(out).all()
    assert torch.equal(out, g), float((out - g).abs().max())
    assert agg.degenerate_steps == 0


@pytest.mark.parametrize("granularity,rtol", [("row", 0.0), ("row", 0.1), ("segment", 0.1)])
@pytest.mark.parametrize("honest", [0, 1, 2])
def test_two_nonfinite_members_are_flagged_degenerate(granularity, rtol, honest):
    """Two of three members non-finite (beyond the code's tolerance s=1): no pair has
    a finite statistic, so every equality class has size 1 and the group has no
    equal pair.  Observed behaviour, pinned here: the step is counted in
    degenerate_steps (exactly 1 — never a silent loss), and the pick falls to the
    deterministic tie-break, member slot 0.  So the honest gradient comes out
    bit-exactly iff the honest member sits in slot 0; otherwise the aggregate is
    non-finite, which the trainer's nan-guard then skips."""
    bad_slots = [s for s in range(3) if s != honest]
    out, g, agg = nonfinite_vote_case("cpu", granularity, rtol, bad_slots,
                                      float("nan"), "element")
    assert agg.degenerate_steps == 1
    if honest == 0:
        assert torch.equal(out, g)
    else:
        assert not torch.isfinite(out).all()
        assert not torch.isfinite(out[7])
