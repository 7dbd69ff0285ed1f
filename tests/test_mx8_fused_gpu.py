"""ops.mx8_column_trimmed_mean / ops.mx8_column_mean_around on the MI355X against
mx8_util.decode (the fp64 definition) then the fallback column op, exactly (NaN positions
equal, other values ==, the sign of a zero not compared).  A lane owns 4 columns, a wave 256,
a block 1024; the grid is capped at 2048 blocks: one trip is 2 097 152 columns."""
import functools

import pytest
import torch

from tests import mx8_util as U
from tests.test_mx8_fused import RULES as MODES

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops import fallback as fb

DEV = "cuda:0"


def bounds(P):
    """median, full mean, trim 1; meamed and phocas at b = 1, (P-1)//2 (b = 0 where P <= 2)"""
    med = ((P - 1) // 2, P // 2 + 1)
    bs = [b for b in sorted({1, (P - 1) // 2}) if 1 <= b and 2 * b < P] or [0]
    return ([("tm", *a) for a in [med, (0, P)] + [(1, P - 1)] * (P >= 3)]
            + [("ma", P - b, *c) for b in bs for c in (med, (b, P - b))])


def same(got, ref):
    n = torch.isnan(ref.cpu())
    return torch.equal(torch.isnan(got.cpu()), n) and bool(((got.cpu() == ref.cpu()) | n).all())


def rule(o, kind, src, args, out):  # the mx8_ op where src is packed bytes
    name = "column_trimmed_mean" if kind == "tm" else "column_mean_around"
    getattr(o, ("mx8_" if src.dtype == torch.uint8 else "") + name)(src, *args, out)


def check(packed, chunk):
    x, dev = torch.from_numpy(U.decode(packed.numpy(), chunk)), packed.to(DEV)
    for kind, *args in bounds(len(packed)):
        ref, buf = torch.empty(chunk), torch.full((chunk + 64,), -12345.0, device=DEV)
        rule(fb, kind, x, args, ref)
        rule(ops, kind, dev, args, buf[:chunk])
        torch.cuda.synchronize()
        assert bool((buf[chunk:] == -12345.0).all()), (kind, args, "guard")
        assert same(buf[:chunk], ref), (kind, args)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49, 63, 64])
def test_every_padded_size_equals_decode_then_rule(P):
    """chunk 576: two full units and a 64-column tail, the scale run padded 18 -> 32."""
    x = U.random_case(P * 576, seed=P, special=True)
    check(U.pack(fb, x, 576).view(P, -1), 576)


@pytest.mark.parametrize("chunk", [64, 320, 1088])
@pytest.mark.parametrize("P", [2, 7])
def test_any_bytes(P, chunk):
    """Less than a wave, ending in a wave, two blocks; NaN block, clamped scale, +-Inf."""
    g = torch.Generator().manual_seed(100 * P + chunk)
    packed = torch.randint(0, 256, (P, U.chunk_bytes(chunk)), generator=g, dtype=torch.uint8)
    packed[0, chunk], packed[-1, chunk + 1] = 255, 3
    packed[0, chunk + 1], packed[0, 32], packed[0, 33] = 250, 0x7E, 0xFE
    check(packed, chunk)


def test_second_grid_trip():
    """Reference: the fallback on the device; medians 2 and 4 planted at the first column
    of the second trip and at the last column."""
    chunk = 2048 * 4 * 256 + 64
    g = torch.Generator(device=DEV).manual_seed(3)
    packed = torch.randint(0, 256, (3, U.chunk_bytes(chunk)), generator=g, dtype=torch.uint8,
                           device=DEV)
    for col, codes in ((chunk - 64, (0x38, 0x40, 0x48)), (chunk - 1, (0x50, 0x40, 0x48))):
        packed[:, chunk + col // 32] = 127
        packed[:, col] = torch.tensor(codes, dtype=torch.uint8, device=DEV)
    for kind, *args in (("tm", 1, 2), ("ma", 2, 1, 2)):
        got, ref = torch.empty(chunk, device=DEV), torch.empty(chunk, device=DEV)
        rule(ops, kind, packed, args, got)
        rule(fb, kind, packed, args, ref)
        assert same(got, ref), (kind, args)
        if kind == "tm":
            assert got[chunk - 64].item() == 2.0 and got[chunk - 1].item() == 4.0


def test_host_rejections():
    u8, out = torch.zeros(65 * 80 + 1, dtype=torch.uint8, device=DEV), torch.zeros(128, device=DEV)
    p2, o64 = u8[:160].view(2, 80), out[:64]
    # P = 65, record length, chunk 96, misaligned, CPU out, fp64 out, lo >= hi
    for packed, o, lo in ((u8[:65 * 80].view(65, 80), o64, 0), (u8[:192].view(2, 96), o64, 0),
                          (u8[:224].view(2, 112), out[:96], 0), (u8[1:161].view(2, 80), o64, 0),
                          (p2, o64.cpu(), 0), (p2, o64.double(), 0), (p2, o64, 1)):
        with pytest.raises(RuntimeError):
            ops.mx8_column_trimmed_mean(packed, lo, 1, o)
        with pytest.raises(RuntimeError):
            ops.mx8_column_mean_around(packed, 1, lo, 1, o)
    ops.mx8_column_trimmed_mean(u8[:0].view(2, 0), 0, 1, out[:0])  # chunk = 0: no launch
    ops.mx8_column_mean_around(u8[:0].view(2, 0), 1, 0, 1, out[:0])


@functools.lru_cache(None)
def trainer_rows(d, d_pad):  # the rows of test_gpu_aggregator_equals_cpu_aggregator, and decoded
    rows = torch.zeros(7, d_pad)
    rows[:, :d] = U.random_case(7 * 32 * (d // 32 + 1), seed=5).view(7, -1)[:, :d]
    return rows, U.roundtrip(rows, d_pad)


@pytest.mark.parametrize("mode,err_mode", [(m, "rev_grad") for m in MODES] + [("median", "alie")])
def test_aggregator_decodes_in_the_rule_kernel(mode, err_mode):
    from draco_amd.config import Config
    from draco_amd.parallel import Trainer
    extra = {"attack_param": 1.0} if err_mode == "alie" else {}
    t = Trainer(Config(network="LeNet", dataset="MNIST", device="cuda", approach="baseline",
                       mode=mode, compress_grad="mx8", workers_per_rank=7, worker_fail=1,
                       err_mode=err_mode, eval_freq=0, log_dir="", train_dir="", **extra))
    rows, decoded = trainer_rows(t.space.d, t.space.d_pad)
    t.payload.copy_(rows)
    out, ref = t.agg.aggregate(t.payload, step=0).cpu(), torch.empty(t.space.d_pad)
    kind, *args = MODES[mode]
    rule(fb, kind, decoded, args, ref)
    assert same(out, ref)  # no colluding row is set: alie changes nothing here
    assert (t.agg._recv32 is None) == (err_mode != "alie")  # alie: unfused, still taken
    t.close()
