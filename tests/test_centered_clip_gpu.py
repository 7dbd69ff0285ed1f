"""ops.clip_step_ and CenteredClipAggregator on the MI355X: the HIP kernels against the
fp64 oracle within the derived bounds of tests/centered_clip_util.py (bit-equality with
the fallback is not claimed: the compiler may contract w*(x - v) into FMAs, and the
distance sum has another order).

Layout facts the shapes are chosen for (ops/csrc/draco_kernels.hip, k_clip_step): the
column sits in registers padded to N in {4, 8, 12, 16, 24, 32, 48, 64} rows, the smallest
N >= P; a lane owns four adjacent columns up to N = 32 and two at N = 48 / 64; 256-thread
blocks, grid capped at 2048 blocks, so at four columns per lane one grid-stride trip
covers 2048*256*4 = 2 097 152 columns; the distances go lane -> wave -> block -> one
workspace row per block -> k_clip_finish, in a fixed order.
"""
import numpy as np
import pytest
import torch

from tests.centered_clip_util import (KINDS, bits, check_step, device_gap, make_case,
                                      weight_patterns)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops.native import available, require_extension

    assert available(), "HIP extension must be built and importable on the GPU box"

DEV = "cuda:0"
TRIP = 2048 * 256 * 4  # columns per grid-stride trip at four columns per lane


def _gpu(x, v0, w, dist=True):
    xd, vd, wd = x.to(DEV), v0.to(DEV), w.to(DEV)
    d2 = ops.clip_step_(xd, vd, wd, dist=dist)
    torch.cuda.synchronize()
    assert torch.equal(bits(xd.cpu()), bits(x))  # x is only read
    return vd.cpu(), (d2.cpu() if d2 is not None else None)


# ------------------------------------------------------------ 1. kernel vs fp64 oracle
# every padded size at its lower edge and its upper edge
@pytest.mark.parametrize("P", [1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49, 64])
def test_kernel_within_bounds_of_fp64_oracle(P):
    worst = [0.0, 0.0]
    shapes = [4096] + ([4] if P == 5 else [])
    for n in shapes:
        for k, kind in enumerate(KINDS):
            x, v0 = make_case(kind, P, n, seed=100 * P + k)
            for name, w in weight_patterns(P, seed=P).items():
                what = (P, n, kind, name)
                v, d2 = _gpu(x, v0, w)
                wv, wd = check_step(x, v0, w, v, d2, what)
                worst = [max(worst[0], wv), max(worst[1], wd)]
                if kind == "equal_v":
                    assert torch.equal(bits(v), bits(v0)) and bool((d2 == 0).all()), what
                v_again, d2_again = _gpu(x, v0, w)
                assert torch.equal(bits(v_again), bits(v)), (what, "v not repeatable")
                assert torch.equal(bits(d2_again), bits(d2)), (what, "d2 not repeatable")
    print(f"P={P}: worst v error / bound = {worst[0]:.4f}, d2 = {worst[1]:.4f}")


# ------------------------------------------------------------ 2. grid-stride edges
def test_second_grid_stride_trip_is_exact():
    """n = one full trip of 2048x256 lanes x 4 columns plus 2 lanes of a second.  x and v
    are zero except small integers at the first column, the last of the first trip, the
    first of the second and the very last; w is dyadic, so every sum is exact in fp32."""
    P, n = 4, TRIP + 8
    cols = [0, TRIP - 1, TRIP, n - 1]
    x = torch.zeros(P, n)
    v0 = torch.zeros(n)
    for k, c in enumerate(cols):
        x[:, c] = torch.tensor([4.0, 8.0, -12.0, 16.0]) * (k + 1)
        v0[c] = 8.0 * (k + 1)
    w = torch.full((P,), 0.25)
    v, d2 = _gpu(x, v0, w)
    # x - v = (-4, 0, -20, 8)*(k+1), delta = -4*(k+1): v_new = 4*(k+1)
    assert [float(v[c]) for c in cols] == [4.0, 8.0, 12.0, 16.0]
    want_v = v0.double() + (0.25 * (x.double() - v0.double())).sum(dim=0)
    assert bool((v.double() == want_v).all())
    want_d2 = ((x.double() - want_v) ** 2).sum(dim=1)
    assert bool((d2.double() == want_d2).all()), (d2, want_d2)
    assert d2.tolist() == [0.0, 480.0, 7680.0, 4320.0]  # row 0 equals v_new: exactly 0
    # a step that does move v: three rows weigh in, the fourth does not
    w2 = torch.tensor([0.25, 0.25, 0.0, 0.25])
    v, d2 = _gpu(x, v0, w2)
    want_v = v0.double() + (w2.double()[[0, 1, 3], None]
                            * (x[[0, 1, 3]].double() - v0.double())).sum(dim=0)
    assert bool((v.double() == want_v).all())
    assert bool((v[cols] != v0[cols]).all())
    want_d2 = ((x.double() - want_v) ** 2).sum(dim=1)
    assert bool((d2.double() == want_d2).all()), (d2, want_d2)


# ------------------------------------------------------------ 3. rows that must not be read
@pytest.mark.parametrize("P", [5, 40])
def test_zero_weight_row_is_not_read(P):
    x, v0 = make_case("randn", P, 4096, seed=31)
    w = weight_patterns(P, seed=2)["edge_zeros"]
    clean_v, clean_d2 = _gpu(x, v0, w)
    x[0] = float("nan")
    x[P - 1, 100] = float("inf")
    v, d2 = _gpu(x, v0, w)
    assert bool(torch.isfinite(v).all())
    assert torch.equal(bits(v), bits(clean_v))
    assert not bool(torch.isfinite(d2[[0, P - 1]]).any())
    assert torch.equal(bits(d2[1:P - 1]), bits(clean_d2[1:P - 1]))


# ------------------------------------------------------------ 4. dist=False
@pytest.mark.parametrize("P", [3, 24, 64])
def test_without_distances_same_v_bits(P):
    x, v0 = make_case("randn", P, 4096, seed=41)
    for name, w in weight_patterns(P, seed=4).items():
        v, d2 = _gpu(x, v0, w)
        v_only, none = _gpu(x, v0, w, dist=False)
        assert none is None and d2 is not None
        assert torch.equal(bits(v_only), bits(v)), (P, name)


# ------------------------------------------------------------ 5. host-side rejections
def test_host_rejections():
    def call(x=None, v=None, w=None, P=4, n=8):
        x = torch.zeros(P, n, device=DEV) if x is None else x
        v = torch.zeros(n, device=DEV) if v is None else v
        w = torch.zeros(P, device=DEV) if w is None else w
        return ops.clip_step_(x, v, w)

    bad = [
        dict(x=torch.zeros(4, 8, device=DEV, dtype=torch.float64)),
        dict(v=torch.zeros(8, device=DEV, dtype=torch.float64)),
        dict(w=torch.zeros(4, device=DEV, dtype=torch.float64)),
        dict(x=torch.zeros(8, 4, device=DEV).t()),          # not contiguous
        dict(v=torch.zeros(16, device=DEV)[::2]),           # not contiguous
        dict(P=65), dict(P=0),
        dict(n=6),                                          # n % 4 != 0
        dict(x=torch.zeros(4 * 8 + 1, device=DEV)[1:].view(4, 8)),  # misaligned x
        dict(v=torch.zeros(9, device=DEV)[1:]),             # misaligned v
        dict(v=torch.zeros(12, device=DEV)), dict(w=torch.zeros(5, device=DEV)),
        dict(w=torch.zeros(4)), dict(v=torch.zeros(8)),     # wrong device
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    with pytest.raises(RuntimeError):  # a CPU tensor handed to the native entry
        require_extension().clip_step(torch.zeros(4, 8), torch.zeros(8), torch.zeros(4), True)
    d2 = call(n=0, w=torch.ones(4, device=DEV))  # n = 0: no launch
    assert call(n=0, w=torch.ones(4, device=DEV)) is not None
    torch.cuda.synchronize()
    assert d2.shape == (4,) and bool((d2 == 0).all())


# ------------------------------------------------------------ 6. aggregator, GPU vs CPU
def test_gpu_aggregator_matches_cpu():
    """P=6, iters=3, auto radius, one ALIE row (computed on each device, so the two
    blocks differ in that row by at most 2 x the collusion bound): the two aggregates
    differ by at most centered_clip_util.device_gap in L2."""
    import torch.nn as nn

    from draco_amd.coding import Collusion
    from draco_amd.parallel.aggregators import CenteredClipAggregator
    from draco_amd.parallel.comm import Communicator
    from draco_amd.parallel.flat import FlatSpace
    from tests.collusion_util import oracle as collusion_oracle

    P, byz, iters = 6, (3,), 3
    payload_cpu = None
    outs, weights, blocks = {}, {}, {}
    for dev in ("cpu", DEV):
        device = torch.device(dev)
        torch.manual_seed(5)
        model = nn.Sequential(nn.Linear(30, 7), nn.Linear(7, 4)).to(device)
        space = FlatSpace(model, 1, device)
        agg = CenteredClipAggregator(Communicator(0, 1, device), space, num_workers=P,
                                     tau=0.0, iters=iters)
        agg.collusion = Collusion(1.0, -1.0, byz)
        if payload_cpu is None:
            torch.manual_seed(9)
            payload_cpu = torch.randn(P, space.d_pad)
            payload_cpu[2] *= 4.0  # one honest row is far out: it is clipped
            payload_cpu[:, space.d:] = 0.0  # pad tail is always zero in production
        payload = space.alloc_payload(P)
        payload.copy_(payload_cpu.to(device))
        outs[dev] = agg.aggregate(payload, step=0).cpu()
        weights[dev] = agg.last_weights.cpu()
        blocks[dev] = payload.cpu()
    _, cbound = collusion_oracle(payload_cpu, list(byz), 1.0, -1.0)
    eps_x = float((2.0 * cbound).norm())
    assert float((blocks[DEV][3].double() - blocks["cpu"][3].double()).norm()) <= eps_x
    allowed = device_gap(blocks["cpu"], torch.zeros(space.d_pad), P, iters, eps_x)
    gap = float((outs[DEV].double() - outs["cpu"].double()).norm())
    print(f"||gpu - cpu|| = {gap:.3e}, allowed {allowed:.3e}, ratio {gap / allowed:.4f}")
    assert gap <= allowed
    assert float(outs["cpu"].norm()) > 100 * allowed  # the bound says something
    assert float(weights["cpu"].min()) < 0.9 and float(weights["cpu"].max()) == 1.0
    assert bool(((weights[DEV] - weights["cpu"]).abs() <= 1e-3).all())
    assert bool((outs[DEV][space.d:] == 0).all())


# ------------------------------------------------------------ 7. trainer steps
@pytest.mark.parametrize("err_mode,param", [("alie", 1.0), ("ipm", 0.5)])
def test_gpu_trainer_steps(tmp_path, err_mode, param):
    from draco_amd.config import Config
    from draco_amd.parallel.trainer import Trainer

    cfg = Config(network="ResNet18", dataset="Cifar10", batch_size=32, device="cuda",
                 lr=0.02, dtype="bf16", max_steps=60, eval_freq=0, log_dir="",
                 train_dir=str(tmp_path / "ckpt"), approach="baseline", mode="centered_clip",
                 worker_fail=1, err_mode=err_mode, attack_param=param, workers_per_rank=4)
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    assert t.agg.name == "centered_clip" and t.P == 4 and t.agg.collusion is not None
    losses = []
    for step in range(2):
        losses.append(t.train_step()["loss"])
        (byz,) = t.schedule.adversaries_at(step)
        assert t.agg.collusion.rows == (byz,)
        lw = t.agg.last_weights
        assert lw.shape == (4,) and bool(((lw >= 0) & (lw <= 1)).all())
        assert bool(torch.isfinite(t.agg.state()).all())
    assert np.isfinite(losses).all()
    assert t.skipped_updates == 0
    t.close()
