"""ops.mx8_segment_gram and ops.mx8_segment_mean_around on the MI355X, then the Trainer.
Gram: against the fp64 Gram of mx8_util.decode per segment.  Every product of two codes and
two power-of-two scales is exact in fp32, so the only error is the accumulation: for a finite
entry |G - G64| <= len * 2^-23 * S, len the segment length and S = sum |x_a||x_b| in fp64; a
non-finite reference entry must come out non-finite.  Gather: exactly
fallback.segment_mean_around on the decoded rows."""
import numpy as np
import pytest
import torch

from tests import mx8_util as U
from tests.bulyan_util import random_sel, separated_rows

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops import fallback as fb

DEV = "cuda:0"
# chunk 576: a zero-length segment, bounds inside a dword and a block, seg[0] > 0, seg[L] < chunk
SEG = [3, 3, 70, 129, 321, 570]


def check_gram(packed, chunk, seg, values=True):
    got = ops.mx8_segment_gram(packed.to(DEV), torch.tensor(seg, device=DEV)).cpu().double().numpy()
    x = U.decode(packed.numpy(), chunk).astype(np.float64)
    assert np.array_equal(got, got.transpose(0, 2, 1), equal_nan=True)  # exactly symmetric
    finite_x = np.abs(x[np.isfinite(x) & (x != 0)])
    for l, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        with np.errstate(invalid="ignore", over="ignore"):
            ref = x[:, lo:hi] @ x[:, lo:hi].T
            S = np.abs(x[:, lo:hi]) @ np.abs(x[:, lo:hi]).T
        fin = np.isfinite(ref)
        assert not np.isfinite(got[l][~fin]).any(), (l, "a non-finite entry came out finite")
        if values:
            # the tolerance's conditions: no product underflows fp32, S <= 2^100
            assert finite_x.min() ** 2 >= 2.0 ** -126 and (S[fin] <= 2.0 ** 100).all()
            err = np.abs(got[l][fin] - ref[fin])
            assert (err <= (hi - lo) * 2.0 ** -23 * S[fin]).all(), (l, float(err.max()))
            if hi == lo:
                assert not got[l].any()


@pytest.mark.parametrize("P", [1, 2, 7, 24, 31, 32])
def test_gram_equals_fp64_gram_of_decoded_rows(P):
    """Rows >= P unloaded; planted: a NaN code and an overflowing product (scale 250, code
    448) in row P-1, a 0xFF scale on row 0's block [320, 352), which lies in two segments, and
    NaN codes in columns 2 and 572, outside every segment, which must reach nothing."""
    packed = U.pack(fb, U.random_case(P * 576, seed=P), 576).view(P, -1).clone()
    packed[P - 1, 100], packed[P - 1, 576 + 17], packed[P - 1, 544] = 0xFF, 250, 0x7E
    packed[0, 576 + 10], packed[0, 2], packed[P // 2, 572] = 0xFF, 0x7F, 0xFF
    check_gram(packed, 576, SEG)


def test_gram_second_trip_and_segment_over_blocks():
    """chunk = 64 * 8192 * 5: 40 960 spans over the capped grid's 2048 blocks x 4 waves are 5
    spans per wave, a trip of 4 and one of 1; a block covers 1280 columns, so the segment
    [1000, 1 500 003) is covered by 1172 blocks and both of its bounds fall inside a span."""
    chunk, P = 64 * 8192 * 5, 3
    x = U.random_case(P * chunk, seed=11).to(DEV)
    check_gram(U.pack(ops, x, chunk).view(P, -1).cpu(), chunk, [5, 1000, 1_500_003, chunk - 70])


def any_bytes(P, chunk, seed):
    g = torch.Generator().manual_seed(seed)
    packed = torch.randint(0, 256, (P, U.chunk_bytes(chunk)), generator=g, dtype=torch.uint8)
    packed[0, chunk], packed[-1, chunk + 1], packed[0, chunk + 2] = 255, 3, 250  # NaN, clamp, Inf
    packed[0, 64:68] = torch.tensor([0x7E, 0xFE, 0x7F, 0xFF], dtype=torch.uint8)
    return packed


def test_gram_any_bytes():
    """Scale < 10, 0xFF scale, NaN codes, overflow: the non-finite entries alone are compared."""
    check_gram(any_bytes(7, 576, 3), 576, SEG, values=False)


def same(got, ref):
    n = torch.isnan(ref)
    return torch.equal(torch.isnan(got), n) and bool(((got == ref) | n).all())


def check_gather(packed, sel, plans):
    chunk, seg, x = 576, torch.tensor(SEG), torch.from_numpy(U.decode(packed.numpy(), 576))
    for keep, clo, chi in plans:
        ref, buf = torch.empty(chunk), torch.full((chunk + 64,), -12345.0, device=DEV)
        fb.segment_mean_around(x, sel, seg, keep, clo, chi, ref)
        ops.mx8_segment_mean_around(packed.to(DEV), sel.to(DEV), seg.to(DEV), keep, clo, chi,
                                    buf[:chunk])
        assert bool((buf[chunk:] == -12345.0).all()), "guard"
        assert same(buf[:chunk].cpu(), ref), (keep, clo, chi)
        yield ref


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32])
def test_gather_equals_fallback_on_decoded_rows(T):
    """Multi-Krum's plan (keep = T) and Bulyan's (median centre, keep = T - 2f, f = 1 from
    T = 3).  Row P-1 is selected nowhere (T < P): NaN codes under 0xFF scales."""
    P = min(32, T + 3)
    packed = U.pack(fb, U.random_case(P * 576, seed=T), 576).view(P, -1).clone()
    sel = random_sel(len(SEG) - 1, P - (T < P), T, seed=T)
    if T < P:
        packed[P - 1, :576], packed[P - 1, 576:594] = 0x7F, 0xFF
    for ref in check_gather(packed, sel, [(T, 0, T), (T - 2 * (T >= 3), (T - 1) // 2, T // 2 + 1)]):
        assert bool(torch.isfinite(ref).all()) and not bool(ref[:3].any() or ref[570:].any())


def test_gather_any_bytes():
    list(check_gather(any_bytes(7, 576, 5), random_sel(len(SEG) - 1, 7, 5, seed=1),
                      [(5, 0, 5), (3, 2, 3)]))


def test_host_rejections():
    u8, out = torch.zeros(33 * 80, dtype=torch.uint8, device=DEV), torch.zeros(64, device=DEV)
    seg, sel = torch.tensor([0, 64], device=DEV), torch.zeros(1, 2, dtype=torch.long, device=DEV)
    p2 = u8[:160].view(2, 80)
    for packed in (u8.view(33, 80), u8[:192].view(2, 96)):  # P = 33, a wrong record length
        with pytest.raises(RuntimeError):
            ops.mx8_segment_gram(packed, seg)
        with pytest.raises(RuntimeError):
            ops.mx8_segment_mean_around(packed, sel, seg, 1, 0, 1, out)
    for s, o in ((sel, out.cpu()), (torch.zeros(1, 3, dtype=torch.long, device=DEV), out)):
        with pytest.raises(RuntimeError):  # a CPU out, T > P
            ops.mx8_segment_mean_around(p2, s, seg, 1, 0, 1, o)
    ops.mx8_segment_mean_around(p2, sel, seg, 1, 0, 1, out)


@pytest.mark.parametrize("mode", ["multi_krum", "bulyan"])
def test_trainer_runs_the_rule_on_the_records(mode):
    from draco_amd.config import Config
    from draco_amd.models import build_model
    from draco_amd.parallel import Communicator, FlatSpace, Trainer
    from draco_amd.parallel.aggregators import build_baseline_aggregator
    kw = dict(network="LeNet", dataset="MNIST", approach="baseline", mode=mode, worker_fail=1,
              compress_grad="mx8", err_mode="rev_grad", eval_freq=0, log_dir="", train_dir="")
    t, cpu = Trainer(Config(device="cuda", workers_per_rank=7, **kw)), torch.device("cpu")
    space = FlatSpace(build_model("LeNet", "MNIST"), 1, cpu)  # the same segments
    agg = build_baseline_aggregator(Config(device="cpu", **kw), Communicator(0, 1, cpu), space, 7)
    rows = torch.zeros(7, space.d_pad)
    rows[:, :space.d] = torch.from_numpy(separated_rows(7, space.d, [5], seed=9))
    ref = agg.aggregate(rows.clone(), step=0)
    t.payload.copy_(rows)
    out = t.agg.aggregate(t.payload, step=0).cpu()
    assert t.agg._recv32 is None and t.agg.wire == "mx8"
    assert torch.equal(t.agg.last_sel.cpu(), agg.last_sel) and not bool((agg.last_sel == 5).any())
    assert same(out, ref) and bool(torch.isfinite(out).all())
    t.close()
