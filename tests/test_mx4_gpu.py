"""ops.mx4_pack / ops.mx4_unpack on the MI355X, all exact.  Both kernels walk units of 512
elements of one record, two units per wave per trip (1024 elements), four waves per block
(4096), at most 2048 blocks.  n = 64 is less than a unit (two quads); 576 ends 64 elements
into its second unit (18 scale bytes: two past a 16-byte run); 1024 is an even unit count;
4160 is just over one block's trip and spans two blocks; chunk 64 and 576 with three records
put a record boundary and its padding mid-wave; the last case takes a wave through a second
trip of the grid."""
import pytest
import torch

from tests import mx4_util as U

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops import fallback as fb
    from draco_amd.ops.native import available

    assert available(), "HIP extension must be built and importable on the GPU box"

DEV = "cuda:0"


def twice(run, size, dtype, fill):
    """Two runs of run(out) into a guarded buffer; they agree, the guard is intact."""
    outs = []
    for _ in range(2):
        buf = torch.full((size + 64,), fill, dtype=dtype, device=DEV)
        run(buf[:size])
        torch.cuda.synchronize()
        assert bool((buf[size:] == fill).all())
        outs.append(buf[:size].cpu())
    assert U.same_values(outs[0].float(), outs[1].float())
    return outs[0]


@pytest.mark.parametrize("seed", [None, 0x1234567890ABCDEF], ids=["nearest", "stochastic"])
@pytest.mark.parametrize("n,chunk", [(64, 64), (576, 576), (1024, 1024), (4160, 4160), (192, 64),
                                     (1728, 576)])
def test_pack_equals_fallback(n, chunk, seed):
    x = U.random_case(n, seed=n, special=True)
    if n == 576:
        x = torch.from_numpy(U.encode_case()[:576])  # grid values, midpoints, subnormals
    got = twice(lambda out: ops.mx4_pack(x.to(DEV), out, chunk, seed),
                n // chunk * U.chunk_bytes(chunk), torch.uint8, 0x5A)
    assert torch.equal(got, U.pack(fb, x, chunk, seed))


@pytest.mark.parametrize("chunk", [64, 576, 1024])
@pytest.mark.parametrize("P", [1, 2, 7])
def test_unpack_equals_fallback_on_any_bytes(P, chunk):
    g = torch.Generator().manual_seed(100 * P + chunk)
    packed = torch.randint(0, 256, (P, U.chunk_bytes(chunk)), generator=g, dtype=torch.uint8)
    packed[0, chunk // 2] = 255  # a NaN block and a clamped scale, whatever the draw
    packed[-1, chunk // 2 + 1] = 1
    if chunk == 64:
        packed[0] = torch.from_numpy(U.decode_case()[5])  # every code, s = 253; then 254
        packed[-1, :34] = torch.from_numpy(U.decode_case()[6, :34])
    ref = torch.empty(P, chunk)
    fb.mx4_unpack(packed, ref)
    got = twice(lambda out: ops.mx4_unpack(packed.to(DEV), out.view(P, chunk)), P * chunk,
                torch.float32, -12345.0).view(P, chunk)
    assert U.same_values(got, ref)


def test_second_grid_trip_and_host_checks():
    """Past 2048 blocks * 8 units a wave takes a second trip; the reference is the
    fallback's torch statement run on the same device.  Then the extension's own checks."""
    n = (2048 * 8 + 5) * 512
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(n, generator=g, device=DEV) * 2.0 ** torch.randint(
        -20, 20, (n // 32, 1), generator=g, device=DEV).float().expand(-1, 32).reshape(-1)
    x[::100003] = float("nan")
    for seed in (None, 77):
        got, ref = U.pack(ops, x, n, seed), U.pack(fb, x, n, seed)
        assert torch.equal(got, ref)
    y, yref = torch.empty(1, n, device=DEV), torch.empty(1, n, device=DEV)
    ops.mx4_unpack(got.view(1, -1), y)
    fb.mx4_unpack(ref.view(1, -1), yref)
    assert U.same_values(y, yref)
    f32, u8 = torch.zeros(129, device=DEV), torch.zeros(96, dtype=torch.uint8, device=DEV)
    for a, out, chunk in ((f32[:128].double(), u8, 64), (f32[:128], u8, 96), (f32[:128], u8[:95], 64),
                          (f32[1:], u8, 64), (f32[:128], u8.cpu(), 64)):  # f32[1:]: misaligned
        with pytest.raises(RuntimeError):
            ops.mx4_pack(a, out, chunk)
    with pytest.raises(RuntimeError):
        ops.mx4_unpack(u8.view(2, 48), f32[:128].view(1, 128))
    ops.mx4_unpack(u8[:0].view(0, 48), f32[:0].view(0, 64))  # P = 0: no launch


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
def test_gpu_aggregator_equals_cpu_aggregator(rounding):
    """The decode is exact, the stochastic bits are a stateless hash of (seed, index), and
    column_trimmed_mean is bit-exact against its fallback (tests/test_trimmed_mean_gpu.py)."""
    from draco_amd.config import Config
    from draco_amd.parallel import Trainer
    outs = {}
    for dev in ("cuda", "cpu"):
        t = Trainer(Config(network="LeNet", dataset="MNIST", device=dev, approach="baseline",
                           mode="trimmed_mean", compress_grad="mx4", mx_rounding=rounding,
                           workers_per_rank=7, worker_fail=1, eval_freq=0, log_dir="", train_dir=""))
        assert t.agg.wire == "mx4" and t.device.type == dev
        rows = torch.zeros(7, t.space.d_pad)
        rows[:, : t.space.d] = U.random_case(7 * 32 * (t.space.d // 32 + 1), seed=5).view(
            7, -1)[:, : t.space.d]
        t.payload.copy_(rows)
        outs[dev] = t.agg.aggregate(t.payload, step=0).cpu()
        t.close()
    assert torch.equal(outs["cuda"], outs["cpu"])
    if rounding == "nearest":
        ref = torch.empty_like(outs["cpu"])
        fb.column_trimmed_mean(U.roundtrip(rows, rows.shape[1]), 1, 6, ref)
        assert torch.equal(outs["cpu"], ref)
