"""ops.mx4_column_trimmed_mean / ops.mx4_column_mean_around on the MI355X against
mx4_util.decode (the fp64 definition) then the fallback column op, exactly (NaN positions
equal, other values ==, the sign of a zero not compared).  A lane owns 8 columns, a wave 512,
a block 2048; the grid is capped at 2048 blocks: one trip is 4 194 304 columns."""
import functools

import pytest
import torch

from tests import mx4_util as U
from tests.test_mx4_fused import RULES as MODES, column_op as rule, reference
from tests.test_mx8_fused_gpu import bounds, same

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops import fallback as fb

DEV = "cuda:0"


def check(packed, chunk):
    x, dev = torch.from_numpy(U.decode(packed.numpy(), chunk)), packed.to(DEV)
    for kind, *args in bounds(len(packed)):
        ref, buf = reference(x, kind, args), torch.full((chunk + 64,), -12345.0, device=DEV)
        rule(ops, kind, dev, args, buf[:chunk])
        torch.cuda.synchronize()
        assert bool((buf[chunk:] == -12345.0).all()), (kind, args, "guard")
        assert same(buf[:chunk], ref), (kind, args)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49, 63, 64])
def test_every_padded_size_equals_decode_then_rule(P):
    """chunk 1088: two full units and a 64-column tail, the scale run padded 34 -> 48; a NaN
    element in blocks 0, 1, 2 of rows 0, 1, 2 and one all-zero block."""
    x = U.random_case(P * 1088, seed=P).view(P, 1088)
    for p in range(min(P, 3)):
        x[p, 32 * p + 5] = float("nan")
    x[P - 1, 96:128] = 0.0
    check(U.pack(fb, x.reshape(-1), 1088).view(P, -1), 1088)


@pytest.mark.parametrize("chunk", [64, 320, 1088])
@pytest.mark.parametrize("P", [2, 7])
def test_any_bytes(P, chunk):
    """Less than one quad of lanes, ending inside a wave, across units; a NaN block, a clamped
    scale, an overflow block (code 7 of either sign at s = 254; every code from 4 up
    overflows there, so at chunk 64 it shares the NaN block's columns to leave the others)."""
    g = torch.Generator().manual_seed(100 * P + chunk)
    packed = torch.randint(0, 256, (P, U.chunk_bytes(chunk)), generator=g, dtype=torch.uint8)
    s0, ob = chunk // 2, 2 if chunk > 64 else 0  # the first scale byte, the overflow block
    packed[0, s0], packed[-1, s0 + 1] = 255, 1
    packed[-1, s0 + ob], packed[-1, 16 * ob], packed[-1, 16 * ob + 1] = 254, 0x7F, 0xF7
    check(packed, chunk)


def test_second_grid_trip():
    """Reference: the fallback on the device; medians 2 and 4 planted at the first column
    of the second trip and at the last column."""
    chunk = 2048 * 4 * 512 + 64
    g = torch.Generator(device=DEV).manual_seed(3)
    packed = torch.randint(0, 256, (3, U.chunk_bytes(chunk)), generator=g, dtype=torch.uint8,
                           device=DEV)
    # low nibbles 2, 4, 5 are 1, 2, 3 and high nibbles 6, 7, 5 are 4, 6, 3 at scale 2^0
    for col, codes in ((chunk - 64, (0x02, 0x04, 0x05)), (chunk - 1, (0x60, 0x70, 0x50))):
        packed[:, chunk // 2 + col // 32] = 127
        packed[:, col // 2] = torch.tensor(codes, dtype=torch.uint8, device=DEV)
    for kind, *args in (("tm", 1, 2), ("ma", 2, 1, 2)):
        got, ref = torch.empty(chunk, device=DEV), torch.empty(chunk, device=DEV)
        rule(ops, kind, packed, args, got)
        rule(fb, kind, packed, args, ref)
        assert same(got, ref) and int(torch.isfinite(ref).sum()) * 3 >= chunk, (kind, args)
        if kind == "tm":
            assert got[chunk - 64].item() == 2.0 and got[chunk - 1].item() == 4.0


def test_host_rejections():
    u8, out = torch.zeros(65 * 48 + 1, dtype=torch.uint8, device=DEV), torch.zeros(128, device=DEV)
    p2, o64 = u8[:96].view(2, 48), out[:64]
    # P = 65, record length, chunk 96, misaligned, CPU out, fp64 out, lo >= hi
    for packed, o, lo in ((u8[:65 * 48].view(65, 48), o64, 0), (u8[:128].view(2, 64), o64, 0),
                          (u8[:128].view(2, 64), out[:96], 0), (u8[1:97].view(2, 48), o64, 0),
                          (p2, o64.cpu(), 0), (p2, o64.double(), 0), (p2, o64, 1)):
        with pytest.raises(RuntimeError):
            ops.mx4_column_trimmed_mean(packed, lo, 1, o)
        with pytest.raises(RuntimeError):
            ops.mx4_column_mean_around(packed, 1, lo, 1, o)
    for bad in ((p2.int(), 1, o64), (p2, 1, out[::2]), (p2, 0, o64), (p2, 3, o64)):
        with pytest.raises(RuntimeError):  # int32 records, strided out, keep outside 1..P
            ops.mx4_column_mean_around(bad[0], bad[1], 0, 1, bad[2])
    ops.mx4_column_trimmed_mean(u8[:0].view(2, 0), 0, 1, out[:0])  # chunk = 0: no launch
    ops.mx4_column_mean_around(u8[:0].view(2, 0), 1, 0, 1, out[:0])


@functools.lru_cache(None)
def trainer_rows(d, d_pad):  # the rows of test_mx4_gpu's aggregator test, and decoded
    rows = torch.zeros(7, d_pad)
    rows[:, :d] = U.random_case(7 * 32 * (d // 32 + 1), seed=5).view(7, -1)[:, :d]
    return rows, U.roundtrip(rows, d_pad)


@pytest.mark.parametrize("mode,err_mode", [(m, "rev_grad") for m in MODES] + [("median", "alie")])
def test_aggregator_decodes_in_the_rule_kernel(mode, err_mode):
    from draco_amd.config import Config
    from draco_amd.parallel import Trainer
    extra = {"attack_param": 1.0} if err_mode == "alie" else {}
    t = Trainer(Config(network="LeNet", dataset="MNIST", device="cuda", approach="baseline",
                       mode=mode, compress_grad="mx4", mx_rounding="nearest", workers_per_rank=7,
                       worker_fail=1, err_mode=err_mode, eval_freq=0, log_dir="", train_dir="",
                       **extra))
    rows, decoded = trainer_rows(t.space.d, t.space.d_pad)
    t.payload.copy_(rows)
    out = t.agg.aggregate(t.payload, step=0).cpu()
    kind, *args = MODES[mode]
    assert same(out, reference(decoded, kind, args))  # no colluding row is set: alie changes nothing
    assert (t.agg._recv32 is None) == (err_mode != "alie")  # alie: unfused, still taken
    t.close()
