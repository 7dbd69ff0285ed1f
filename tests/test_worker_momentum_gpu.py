"""ops.worker_momentum_ on the MI355X: the HIP kernel against the fp64 oracle within the
bound of tests/worker_momentum_util.py (bit-equality with the fallback is not claimed:
the kernel contracts the update into one FMA), bit for bit on the first step and on the
non-finite branches, and through the trainer.

Layout facts the shapes are chosen for (ops/csrc/draco_kernels.hip, k_worker_momentum):
a lane owns one float4; 256-thread blocks, grid capped at 2048 blocks, so one
grid-stride trip covers 2048*256*4 = 2 097 152 elements.
"""
import numpy as np
import pytest
import torch

from tests.worker_momentum_util import (NONFINITE, bits, check_first, check_update, make_pair,
                                        oracle)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops.native import available, require_extension

    assert available(), "HIP extension must be built and importable on the GPU box"

DEV = "cuda:0"
TRIP = 2048 * 256 * 4  # elements per grid-stride trip


def _gpu(g, m, beta, first):
    gd, md = g.to(DEV), m.to(DEV)
    ops.worker_momentum_(gd, md, beta, first)
    torch.cuda.synchronize()
    return gd.cpu(), md.cpu()


# ------------------------------------------------------------ 1. kernel vs fp64 oracle
# one float4 in one lane; a partial last block; four full blocks
@pytest.mark.parametrize("n", [4, 1020, 1024])
@pytest.mark.parametrize("beta", [0.5, 0.9, 0.99])
def test_kernel_within_bound_of_fp64_oracle(n, beta):
    g0, m0 = make_pair(n, seed=n + int(beta * 100))
    g, m = _gpu(g0, m0, beta, False)
    check_update(g0, m0, g, m, beta, f"kernel n={n} beta={beta}")
    g2, m2 = _gpu(g0, m0, beta, False)
    assert torch.equal(bits(g2), bits(g)) and torch.equal(bits(m2), bits(m))
    g, m = _gpu(g0, m0, beta, True)
    check_first(g0, g, m, f"kernel first n={n}")
    g2, m2 = _gpu(g0, m0, beta, True)
    assert torch.equal(bits(g2), bits(g)) and torch.equal(bits(m2), bits(m))


def test_second_grid_stride_trip_is_exact():
    """n = one full trip + two lanes of a second.  Small even integers and beta = 0.5:
    every result is exact in fp32, so the WHOLE row is compared with == against the
    oracle, the planted columns at both ends of both trips included."""
    n = TRIP + 8
    gen = torch.Generator().manual_seed(11)
    g0 = (torch.randint(-500, 500, (n,), generator=gen) * 2).float()
    m0 = (torch.randint(-500, 500, (n,), generator=gen) * 2).float()
    plants = {0: (6.0, 2.0, 4.0), TRIP - 1: (-8.0, 2.0, -3.0), TRIP: (10.0, -20.0, -5.0),
              n - 1: (1024.0, 2.0, 513.0)}
    for i, (gv, mv, _) in plants.items():
        g0[i], m0[i] = gv, mv
    sent, exact = oracle(g0, m0, 0.5, False)
    g, m = _gpu(g0, m0, 0.5, False)
    assert np.array_equal(m.numpy().astype(np.float64), exact)
    assert torch.equal(bits(g), bits(m))
    for i, (_, _, want) in plants.items():
        assert float(m[i]) == want, (i, float(m[i]))
    g2, m2 = _gpu(g0, m0, 0.5, False)
    assert torch.equal(bits(g2), bits(g)) and torch.equal(bits(m2), bits(m))
    g, m = _gpu(g0, m0, 0.5, True)
    check_first(g0, g, m, "two trips first")


# ------------------------------------------------------------ 2. non-finite rule
@pytest.mark.parametrize("first", [False, True])
def test_nonfinite_gradient_does_not_reach_the_state(first):
    n = 1024
    g0, m0 = make_pair(n, seed=7)
    # the first and the last element, and one in each half of a float4
    plants = {0: NONFINITE[0], 9: NONFINITE[1], 14: NONFINITE[2], 517: NONFINITE[0],
              n - 1: NONFINITE[1]}
    gp = g0.clone()
    for i, v in plants.items():
        gp[i] = v
    g, m = _gpu(gp, m0, 0.9, first)
    idx = torch.tensor(sorted(plants))
    keep = torch.ones(n, dtype=torch.bool)
    keep[idx] = False
    assert torch.equal(bits(g)[idx], bits(gp)[idx])
    if first:
        check_first(gp, g, m, "kernel planted first")
        assert bool((bits(m)[idx] == 0).all())
    else:
        check_update(gp, m0, g, m, 0.9, "kernel planted")
        assert torch.equal(bits(m)[idx], bits(m0)[idx])
    gc, mc = _gpu(g0, m0, 0.9, first)
    assert torch.equal(bits(g)[keep], bits(gc)[keep])
    assert torch.equal(bits(m)[keep], bits(mc)[keep])
    assert bool(torch.isfinite(m).all())


# ------------------------------------------------------------ 3. slices of two buffers
@pytest.mark.parametrize("first", [False, True])
def test_slice_of_a_row_leaves_the_rest_alone(first):
    gen = torch.Generator().manual_seed(3)
    payload0 = torch.randn(3, 8192, generator=gen)
    state0 = torch.randn(3, 8192, generator=gen)
    payload, state = payload0.to(DEV), state0.to(DEV)
    lo, hi = 64, 64 + 4096
    ops.worker_momentum_(payload[1, lo:hi], state[1, lo:hi], 0.9, first)
    torch.cuda.synchronize()
    payload, state = payload.cpu(), state.cpu()
    if first:
        check_first(payload0[1, lo:hi], payload[1, lo:hi], state[1, lo:hi], "slice first")
    else:
        check_update(payload0[1, lo:hi], state0[1, lo:hi], payload[1, lo:hi], state[1, lo:hi],
                     0.9, "slice")
    outside = torch.ones(3, 8192, dtype=torch.bool)
    outside[1, lo:hi] = False
    assert torch.equal(bits(payload)[outside], bits(payload0)[outside])
    assert torch.equal(bits(state)[outside], bits(state0)[outside])


# ------------------------------------------------------------ 4. host-side rejections
def test_host_rejections():
    def call(g=None, m=None, beta=0.9, n=8):
        g = torch.zeros(n, device=DEV) if g is None else g
        m = torch.zeros(n, device=DEV) if m is None else m
        return ops.worker_momentum_(g, m, beta, False)

    bad = [
        dict(g=torch.zeros(8, device=DEV, dtype=torch.float64)),
        dict(m=torch.zeros(8, device=DEV, dtype=torch.float64)),
        dict(g=torch.zeros(16, device=DEV)[::2]),            # not contiguous
        dict(m=torch.zeros(16, device=DEV)[::2]),            # not contiguous
        dict(n=6),                                           # numel % 4 != 0
        dict(g=torch.zeros(9, device=DEV)[1:]),              # misaligned g
        dict(m=torch.zeros(9, device=DEV)[1:]),              # misaligned m
        dict(m=torch.zeros(12, device=DEV)),                 # length mismatch
        dict(m=torch.zeros(8)),                              # wrong device
        dict(beta=1.0), dict(beta=-0.5),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    with pytest.raises(RuntimeError):  # a CPU tensor handed to the native entry
        require_extension().worker_momentum(torch.zeros(8), torch.zeros(8), 0.9, False)
    call(n=0)  # n = 0: no launch
    torch.cuda.synchronize()


# ------------------------------------------------------------ 5. trainer steps
@pytest.mark.parametrize("hip_graphs", [True, False])
def test_gpu_trainer_steps(tmp_path, hip_graphs):
    from draco_amd.config import Config
    from draco_amd.parallel.trainer import Trainer

    cfg = Config(network="ResNet18", dataset="Cifar10", batch_size=32, device="cuda",
                 lr=0.02, dtype="bf16", max_steps=60, eval_freq=0, log_dir="",
                 train_dir=str(tmp_path / "ckpt"), approach="baseline", mode="centered_clip",
                 worker_fail=1, err_mode="alie", attack_param=1.0, workers_per_rank=4,
                 worker_momentum=0.9, momentum=0.0, hip_graphs=hip_graphs)
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    assert t.use_graphs == hip_graphs and t.P == 4 and t.wm.state.shape == (4, t.space.d_pad)
    losses = [t.train_step()["loss"]]
    wm1 = t.wm.state.clone()
    losses.append(t.train_step()["loss"])
    torch.cuda.synchronize()
    assert np.isfinite(losses).all()
    assert t.skipped_updates == 0
    assert t.wm.first == [False] * 4
    for l in range(4):
        assert bool(torch.isfinite(t.wm.state[l]).all()) and bool(wm1[l].abs().max() > 0)
        assert bool(t.wm.state[l].abs().max() > 0)
        assert not torch.equal(t.wm.state[l], wm1[l]), l
    t.close()
