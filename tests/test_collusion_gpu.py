"""ops.collude_ on the MI355X: the HIP kernel against the fp64 oracle within the derived
bound of tests/collusion_util.py (8*(|a|+|b|)*P*2^-24*M_j per column; bit-equality with
the fallback is not claimed, the compiler may contract a*mu + b*sigma into FMAs).

Layout facts the shapes are chosen for (ops/csrc/draco_kernels.hip, k_collude): four
adjacent columns per lane (one 16-byte access per row), 256-thread blocks, grid capped
at 2048 blocks, so one grid-stride trip covers 2048*256*4 = 2 097 152 columns; the
honest values sit in registers padded to N in {4, 8, 12, 16, 24, 32, 48, 64} rows, the
smallest N >= P; the Byzantine row set is a 64-bit mask passed by value (rows 31, 32
and 63 are where a 32-bit shift would break).
"""
import numpy as np
import pytest
import torch

from tests.collusion_util import (AB, KINDS, U, bits, check_result, honest_rows, make_data,
                                  oracle, scattered)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops.native import available, require_extension

    assert available(), "HIP extension must be built and importable on the GPU box"

DEV = "cuda:0"
TRIP = 2048 * 256 * 4  # columns per grid-stride trip
SENTINEL = -12345.0


def _gpu(x0, rows, a, b):
    """Kernel result for x0 with the Byzantine rows prefilled with a sentinel (a row
    that is never written shows; a Byzantine row that is read shows as an error)."""
    x = x0.clone()
    x[rows] = SENTINEL
    y = x.to(DEV)
    ops.collude_(y, rows, a, b)
    torch.cuda.synchronize()
    return y.cpu()


def _row_sets(P):
    sets = [[0], [P - 1]]
    if (P - 1) // 2 >= 1:
        sets.append(scattered(P))
    wide = [r for r in (31, 32, 63) if r < P]
    if wide and len(wide) < P:
        sets.append(wide)
    return sets


# ------------------------------------------------------------ 1. kernel vs fp64 oracle
# every padded size at its lower edge and its upper edge
@pytest.mark.parametrize("P", [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64])
def test_kernel_within_bound_of_fp64_oracle(P):
    worst = 0.0
    for k, kind in enumerate(KINDS):
        x0 = make_data(kind, P, 4096, seed=100 * P + k)
        for a, b in AB:
            for rows in _row_sets(P):
                y = _gpu(x0, rows, a, b)
                worst = max(worst, check_result(x0, y, rows, a, b, (P, kind, a, b, rows)))
                again = _gpu(x0, rows, a, b)
                assert torch.equal(bits(again), bits(y)), (P, kind, a, b, rows, "not repeatable")
    print(f"P={P}: worst |error| / bound = {worst:.4f}")


# ------------------------------------------------------------ 2. grid-stride edges
def test_second_grid_stride_trip_and_smallest_shape():
    P, d = 4, TRIP + 8  # one full trip of 2048x256 lanes x 4 columns, plus 2 lanes of a second
    x0 = make_data("randn", P, d, seed=77)
    rows = [2]
    # the last column of the first trip, the first of the second, the very last
    for col, vals in ((TRIP - 1, (1.0, 2.0, 3.0)), (TRIP, (1000.0, 2000.0, 3000.0)),
                      (d - 1, (-6000.0, -4000.0, -5000.0))):
        x0[honest_rows(P, rows), col] = torch.tensor(vals)
    ipm = _gpu(x0, rows, -1.0, 0.0)  # IPM eps=1: minus the honest mean
    check_result(x0, ipm, rows, -1.0, 0.0, "ipm")
    assert float(ipm[2, TRIP - 1]) == -2.0
    assert float(ipm[2, TRIP]) == -2000.0
    assert float(ipm[2, d - 1]) == 5000.0
    alie = _gpu(x0, rows, 1.0, -1.0)  # sigma of {1000, 2000, 3000} = 1000*sqrt(2/3)
    check_result(x0, alie, rows, 1.0, -1.0, "alie")
    want = 2000.0 - 1000.0 * np.sqrt(2.0 / 3.0)
    assert abs(float(alie[2, TRIP]) - want) <= 8 * 2 * P * U * 3000.0
    xs = make_data("randn", 3, 4, seed=78)
    for a, b in AB:
        check_result(xs, _gpu(xs, [1], a, b), [1], a, b, "d=4")


# ------------------------------------------------------------ 3. b = 0 and b != 0 paths
def test_sigma_path_and_mean_only_path_on_the_same_input():
    P, rows = 9, [0, 4, 8]
    for kind in ("randn", "offset"):
        x0 = make_data(kind, P, 4096, seed=9)
        mean_only = _gpu(x0, rows, -4.0, 0.0)
        with_sigma = _gpu(x0, rows, -4.0, 2.0)
        check_result(x0, mean_only, rows, -4.0, 0.0, (kind, "b=0"))
        check_result(x0, with_sigma, rows, -4.0, 2.0, (kind, "b=2"))
        X = x0[honest_rows(P, rows)].double()
        bound = 8.0 * 4.0 * P * U * X.abs().amax(dim=0)
        assert bool(((mean_only[0].double() + 4.0 * X.mean(dim=0)).abs() <= bound).all())
        if kind == "randn":
            # six Gaussian values: 2*sigma is far above the rounding of -4*mu in every
            # column, so the two paths must differ everywhere
            assert bool((with_sigma[0] > mean_only[0]).all())


# ------------------------------------------------------------ 4. host-side rejections
def test_host_rejections():
    def call(P, d, rows, x=None):
        x = torch.zeros(P, d, device=DEV) if x is None else x
        ops.collude_(x, rows, 1.0, -1.0)

    with pytest.raises(RuntimeError):
        call(1, 8, [0])
    with pytest.raises(RuntimeError):
        call(65, 8, [0])
    with pytest.raises(RuntimeError):
        call(4, 6, [0])
    with pytest.raises(RuntimeError):
        call(4, 8, [1, 1])
    with pytest.raises(RuntimeError):
        call(4, 8, [4])
    with pytest.raises(RuntimeError):
        call(4, 8, [-1])
    with pytest.raises(RuntimeError):
        call(4, 8, [0, 1, 2, 3])
    with pytest.raises(RuntimeError):
        call(4, 8, [0], x=torch.zeros(4, 8, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        call(4, 8, [0], x=torch.zeros(8, 4, device=DEV).t())
    with pytest.raises(RuntimeError):  # a CPU tensor handed to the native path
        require_extension().collude(torch.zeros(4, 8), [0], 1.0, -1.0)
    x0 = make_data("randn", 4, 8, seed=1)
    y = x0.to(DEV)
    ops.collude_(y, [], 1.0, -1.0)  # no Byzantine row: no launch
    call(4, 0, [1])  # d = 0: no launch
    torch.cuda.synchronize()
    assert torch.equal(bits(y.cpu()), bits(x0))


# ------------------------------------------------------------ 5. aggregator, GPU vs CPU
@pytest.mark.parametrize("trim", [None, 0])
def test_gpu_aggregator_matches_cpu(trim):
    """median and the trim=0 mean under ALIE z=1, P=6, f=1.  Both rules are 1-Lipschitz
    per coordinate in the sup norm, so the difference between the two devices'
    Byzantine rows (each within the bound of the exact value) reaches the output at
    most once: |gpu - cpu| <= 2 x the bound."""
    import torch.nn as nn

    from draco_amd.coding import Collusion
    from draco_amd.parallel.aggregators import TrimmedMeanAggregator
    from draco_amd.parallel.comm import Communicator
    from draco_amd.parallel.flat import FlatSpace

    P, byz = 6, (3,)
    payload_cpu = None
    outs = {}
    for dev in ("cpu", DEV):
        device = torch.device(dev)
        torch.manual_seed(5)
        model = nn.Sequential(nn.Linear(300, 40), nn.Linear(40, 9)).to(device)
        space = FlatSpace(model, 1, device)
        agg = TrimmedMeanAggregator(Communicator(0, 1, device), space, num_workers=P, trim=trim)
        agg.collusion = Collusion(1.0, -1.0, byz)
        if payload_cpu is None:
            torch.manual_seed(9)
            payload_cpu = torch.randn(P, space.d_pad)
            payload_cpu[:, space.d:] = 0.0  # pad tail is always zero in production
        payload = space.alloc_payload(P)
        payload.copy_(payload_cpu.to(device))
        outs[dev] = agg.aggregate(payload, step=0).cpu()
        assert not torch.equal(payload[3].cpu(), payload_cpu[3])  # the row was overwritten
    d = space.d
    _, bound = oracle(payload_cpu, list(byz), 1.0, -1.0)
    diff = (outs[DEV].double() - outs["cpu"].double()).abs()
    print(f"trim={trim}: worst |gpu - cpu| / (2 x bound) = "
          f"{float((diff[:d] / (2 * bound[:d])).max()):.4f}")
    assert bool((diff <= 2 * bound).all())
    assert bool((outs[DEV][d:] == 0).all())


# ------------------------------------------------------------ 6. trainer steps
@pytest.mark.parametrize("err_mode,param", [("alie", 1.0), ("ipm", 0.5)])
def test_gpu_trainer_steps(tmp_path, err_mode, param):
    from draco_amd.config import Config
    from draco_amd.parallel.trainer import Trainer

    cfg = Config(network="ResNet18", dataset="Cifar10", batch_size=32, device="cuda",
                 lr=0.02, dtype="bf16", max_steps=60, eval_freq=0, log_dir="",
                 train_dir=str(tmp_path / "ckpt"), approach="baseline", mode="median",
                 worker_fail=1, err_mode=err_mode, attack_param=param, workers_per_rank=4)
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    assert t.agg.name == "median" and t.P == 4 and t.agg.collusion is not None
    computed = []
    exchange = t.agg._exchange

    def recording_exchange(payload):
        recv = exchange(payload)
        computed.append(recv.clone())  # what the workers computed, before the overwrite
        return recv

    t.agg._exchange = recording_exchange
    losses = []
    for step in range(2):
        losses.append(t.train_step()["loss"])
        (byz,) = t.schedule.adversaries_at(step)
        assert t.agg.collusion.rows == (byz,)
        block = t.payload.view(4, t.space.shard)  # world 1: the exchanged block is the payload
        hon = honest_rows(4, [byz])
        assert torch.equal(block[hon], computed[step][hon])
        assert not torch.equal(block[byz], computed[step][byz])
    assert np.isfinite(losses).all()
    assert t.skipped_updates == 0
    t.close()
