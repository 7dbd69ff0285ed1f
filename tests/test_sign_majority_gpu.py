"""ops.sign_pack / ops.sign_majority on the MI355X, all exact.  A wave of k_sign_pack owns
256 elements (n % 256 runs over 0, 64, 128, 192); P runs over both sides of every counter
carry of k_sign_majority, n over one record, a partial wave, one block's 256 records + 16."""
import pytest
import torch

from tests.sign_util import pack_rows, same_bits, sign_case, sign_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops import fallback as fb
    from draco_amd.ops.native import available

    assert available(), "HIP extension must be built and importable on the GPU box"

DEV = "cuda:0"


@pytest.mark.parametrize("n", [64, 128, 192, 256, 320, 1088])
def test_pack_bytes_equal_fallback(n):
    x = sign_case(1, n, seed=n)
    buf = torch.full((n // 16 + 64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)  # 64 guards
    ops.sign_pack(x[0].to(DEV), buf[: n // 16])
    torch.cuda.synchronize()
    assert bool((buf[n // 16:] == 0x5A5A5A5A).all())
    assert torch.equal(buf[: n // 16].cpu(), pack_rows(fb, x)[0])


@pytest.mark.parametrize("n", [64, 192, 256, 1088, 256 * 64 + 1024])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64])
def test_majority_equals_int64_reference(P, n):
    x = sign_case(P, n, seed=1000 * P + n)
    ref = sign_ref(x)[1]
    # P = 7: packed on the CPU, voted here
    packed = pack_rows(fb, x).to(DEV) if P == 7 else pack_rows(ops, x.to(DEV))
    runs = []
    for _ in range(2):
        buf = torch.full((n + 64,), -12345.0, device=DEV)  # 64 guard floats behind out
        ops.sign_majority(packed, buf[:n])
        torch.cuda.synchronize()
        assert bool((buf[n:] == -12345.0).all())
        runs.append(buf[:n].cpu())
    assert same_bits(runs[0], ref) and same_bits(runs[0], runs[1])


def test_grid_stride_trips_of_both_kernels():
    """Past 2048 blocks * 256 records either kernel takes a second trip.  Inputs and
    reference are made on the GPU, without the family's subnormals (the reference's float
    compare may flush them there; the small cases carry them)."""
    from tests.sign_util import FAMILY
    P, n = 3, (2048 * 256 + 300) * 64
    g = torch.Generator(device=DEV).manual_seed(9)
    x = FAMILY[:9].to(DEV)[torch.randint(9, (P, n), generator=g, device=DEV)]
    out = torch.empty(n, device=DEV)
    ops.sign_majority(pack_rows(ops, x), out)
    assert torch.equal(out.view(torch.int32), sign_ref(x)[1].view(torch.int32))


def test_host_rejections():
    f32 = lambda *s: torch.zeros(*s, device=DEV)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    for g, out in ((f32(96), i32(6)), (f32(128).double(), i32(8)), (f32(128), f32(8)),
                   (f32(128), i32(12)), (f32(256)[::2], i32(8)), (f32(128), i32(8).cpu())):
        with pytest.raises(RuntimeError):
            ops.sign_pack(g, out)
    for packed, out in ((i32(2, 6), f32(96)), (i32(2, 8).long(), f32(128)),
                        (i32(2, 8), f32(128).double()), (i32(2, 8), f32(192)),
                        (i32(8, 2).t(), f32(128)), (i32(2, 8), f32(128).cpu()),
                        (i32(65, 8), f32(128))):
        with pytest.raises(RuntimeError):
            ops.sign_majority(packed, out)
    ops.sign_pack(f32(0), i32(0))  # n = 0 and P = 0: no launch
    ops.sign_majority(i32(3, 0), f32(0))
    ops.sign_majority(i32(0, 8), f32(128))
    torch.cuda.synchronize()


def test_gpu_trainer_aggregate_equals_cpu_aggregator():
    from draco_amd.config import Config
    from draco_amd.parallel import Trainer
    outs = {}
    for dev in ("cuda", "cpu"):
        t = Trainer(Config(network="FC", dataset="MNIST", device=dev, approach="baseline",
                           mode="normal", compress_grad="sign", workers_per_rank=4,
                           worker_fail=1, eval_freq=0, log_dir="", train_dir=""))
        assert t.agg.name == "sign_majority" and t.device.type == dev
        rows = torch.zeros(4, t.space.d_pad)
        rows[:, : t.space.d] = sign_case(4, t.space.d, seed=11)
        t.payload.copy_(rows)
        outs[dev] = t.agg.aggregate(t.payload, step=0).cpu()
        t.close()
    assert same_bits(outs["cuda"], outs["cpu"]) and same_bits(outs["cpu"], sign_ref(rows)[1])
