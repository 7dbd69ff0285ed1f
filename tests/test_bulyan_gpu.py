"""ops.segment_mean_around on the MI355X: the HIP kernel against the fp32 fallback, bit
for bit — both gather the same rows, sort the same values and run column_mean_around's
arithmetic in the same order, so bit-exactness is the claim (NaN positions must be
equal; the sign of a zero result is not compared) — then MultiKrumAggregator and
BulyanAggregator GPU against CPU, and the two baseline modes in the Trainer.

Layout facts the shapes are chosen for (ops/csrc/draco_kernels.hip): one column per
lane, 256-thread blocks, grid capped at 2048 blocks (one grid-stride trip covers
2048*256 columns); T selected rows padded with +inf to N in {4, 8, 12, 16, 24, 32, 48,
64}, the padding slots re-reading table entry T-1 before a select replaces them; the
segment of a column is found by binary search per lane, so a wave that straddles a
boundary gathers different rows per lane and a lane on an uncovered column sorts +inf
and stores 0.
"""
import numpy as np
import pytest
import torch

from tests.bulyan_util import random_sel, separated_rows
from tests.mean_around_util import bounds, data, legal_bs, plant

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops import fallback as fb
    from draco_amd.ops.native import available

    assert available(), "HIP extension must be built and importable on the GPU box"

DEV = "cuda:0"
INF = float("inf")
BADS = (float("nan"), INF, -INF)
TRIP = 2048 * 256  # columns per grid-stride trip
CENTERS = ["median", "trimmed_mean"]

# empty segments, lane (1, 63/64/65), wave and block (255/257) straddles, uncovered head
# (column 0) and tail (4093..4095) columns
D_MAIN = 4096
SEG_MAIN = [1, 1, 63, 64, 65, 255, 257, 1000, 1000, 2048, 4093]


def _gpu(x, sel, seg, keep, clo, chi):
    out = torch.full((x.shape[1],), -7.0, dtype=torch.float32, device=DEV)
    ops.segment_mean_around(x.to(DEV), sel.to(DEV), torch.as_tensor(seg).to(DEV), keep, clo,
                            chi, out)
    torch.cuda.synchronize()
    return out.cpu()


def _cpu(x, sel, seg, keep, clo, chi):
    out = torch.full((x.shape[1],), -7.0, dtype=torch.float32)
    fb.segment_mean_around(x, sel, torch.as_tensor(seg), keep, clo, chi, out)
    return out


def _assert_same(got, ref, what):
    nan_g, nan_r = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(nan_g, nan_r), (what, "NaN positions differ")
    ok = (got == ref) | nan_r
    assert bool(ok.all()), (what, int((~ok).sum()), int((~ok).nonzero()[0]))


def _scatter(P, gathered, sel, seg, seed):
    """(P, d) rows in which segment l's selected rows sel[l] hold `gathered` (T, d) in
    table order, and every other element is unrelated noise — a kernel that read a
    wrong row, or a wrong segment's rows, gets different values."""
    x = data(P, gathered.shape[1], seed=seed) * 3.0 + 50.0
    for l in range(len(seg) - 1):
        lo, hi = seg[l], seg[l + 1]
        if hi > lo:
            x[sel[l], lo:hi] = gathered[:, lo:hi]
    return x


# ------------------------------------------------------------ 1. kernel == fallback
# every padded size at its lower edge, its upper edge and (where there is room) inside
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49,
                               64])
def test_kernel_equals_fallback_bitwise(T):
    P = min(64, T + 3)
    L = len(SEG_MAIN) - 1
    sel = random_sel(L, P, T, seed=T)  # a different subset, in a different order, per segment
    if P > T:
        assert len({tuple(sorted(s.tolist())) for s in sel}) > 1
    base = data(T, D_MAIN, seed=T)
    cases = [(T, 0, T)]
    for b in legal_bs(T):
        g = base.clone()
        plant(g, b, col0=1024)  # every window start 0..b, inside segment [1000, 2048)
        x = _scatter(P, g, sel, SEG_MAIN, seed=100 + T)
        xg, sg, segg = x.to(DEV), sel.to(DEV), torch.tensor(SEG_MAIN, device=DEV)
        for center in CENTERS:
            keep, clo, chi = bounds(T, b, center)
            _, _, w = fb.mean_around_window(g[:, 1000:2048], keep, clo, chi)
            assert set(w.tolist()) == set(range(b + 1)), (T, b, center)
            out = torch.full((D_MAIN,), -7.0, dtype=torch.float32, device=DEV)
            ops.segment_mean_around(xg, sg, segg, keep, clo, chi, out)
            got = out.cpu()
            _assert_same(got, _cpu(x, sel, SEG_MAIN, keep, clo, chi), (T, b, center))
            assert float(got[0]) == 0.0 and bool((got[4093:] == 0.0).all())
    x = _scatter(P, base, sel, SEG_MAIN, seed=100 + T)
    for keep, clo, chi in cases:
        _assert_same(_gpu(x, sel, SEG_MAIN, keep, clo, chi),
                     _cpu(x, sel, SEG_MAIN, keep, clo, chi), (T, "keep=T"))


# ------------------------------------------------------------ 2. grid-stride second trip
def test_second_grid_stride_trip():
    P, T, d = 5, 3, TRIP + 8  # one full trip of 2048x256 lanes plus 8 columns of a second
    seg = [4, TRIP + 3, TRIP + 7]  # a boundary inside the second trip; last column uncovered
    sel = torch.tensor([[4, 0, 2], [1, 3, 0]])
    g = data(T, d, seed=77)
    g[:, TRIP] = torch.tensor([1000.0, 3100.0, 2000.0])      # top is farther: w = 0
    g[:, d - 2] = torch.tensor([-6200.0, -4000.0, -5000.0])  # bottom is farther: w = 1
    x = _scatter(P, g, sel, seg, seed=78)
    for center in CENTERS:
        keep, clo, chi = bounds(T, 1, center)
        got = _gpu(x, sel, seg, keep, clo, chi)
        _assert_same(got, _cpu(x, sel, seg, keep, clo, chi), center)
        assert float(got[TRIP]) == 1500.0 and float(got[d - 2]) == -4500.0
        assert bool((got[:4] == 0.0).all()) and float(got[d - 1]) == 0.0


# ------------------------------------------------------------ 3. planted non-finites
D_NF = 1024
NF_COLS = [0, 63, 64, 255, 256, D_NF - 1]  # lane, wave and block edges
NF_SEG = [0, 60, 64, 250, 256, 300, D_NF]
NF_P, NF_T = 7, 5
NF_CASES = [bounds(NF_T, 2, c) for c in CENTERS]


def _seg_of(col):
    return max(l for l in range(len(NF_SEG) - 1) if NF_SEG[l] <= col)


@pytest.fixture(scope="module")
def clean_nf():
    sel = random_sel(len(NF_SEG) - 1, NF_P, NF_T, seed=5)
    x = data(NF_P, D_NF, seed=5)
    return x, sel, {case: _gpu(x, sel, NF_SEG, *case) for case in NF_CASES}


@pytest.mark.parametrize("bad", BADS)
@pytest.mark.parametrize("slot", [0, NF_T - 1])
def test_planted_nonfinite_in_a_selected_row(clean_nf, bad, slot):
    clean, sel, clean_out = clean_nf
    x = clean.clone()
    for col in NF_COLS:
        x[sel[_seg_of(col), slot], col] = bad
    other = torch.ones(D_NF, dtype=torch.bool)
    other[NF_COLS] = False
    for case, ref_clean in clean_out.items():
        got = _gpu(x, sel, NF_SEG, *case)
        assert torch.equal(got[other].view(torch.int32), ref_clean[other].view(torch.int32))
        _assert_same(got, _cpu(x, sel, NF_SEG, *case), (bad, slot, case))
        assert bool(torch.isfinite(got).all())  # one bad value per column, b = 2


def test_more_nonfinite_selected_rows_than_b_match_the_fallback(clean_nf):
    clean, sel, _ = clean_nf
    x = clean.clone()
    for col in NF_COLS:
        rows = sel[_seg_of(col)]
        x[rows[0], col] = INF
        x[rows[2], col] = float("nan")
        x[rows[4], col] = -INF
    for case in NF_CASES:
        _assert_same(_gpu(x, sel, NF_SEG, *case), _cpu(x, sel, NF_SEG, *case), case)


@pytest.mark.parametrize("bad", BADS)
def test_nonfinite_in_unselected_rows_changes_nothing(clean_nf, bad):
    """What 0/1 weights in segment_weighted_mean cannot give (fmaf(0, NaN, acc) is NaN):
    a row that lost the selection is never read."""
    clean, sel, clean_out = clean_nf
    x = clean.clone()
    for l in range(len(NF_SEG) - 1):
        lose = sorted(set(range(NF_P)) - set(sel[l].tolist()))
        assert len(lose) == NF_P - NF_T
        x[lose, NF_SEG[l]:NF_SEG[l + 1]] = bad  # the whole segment, edge columns included
    for case, ref_clean in clean_out.items():
        got = _gpu(x, sel, NF_SEG, *case)
        assert torch.equal(got.view(torch.int32), ref_clean.view(torch.int32)), (bad, case)


# ------------------------------------------------------------ 4. host-side rejections
def test_host_rejections():
    def call(P=6, d=8, T=4, L=2, keep=3, clo=1, chi=3, x=None, sel=None, seg=None, out=None):
        x = torch.zeros(P, d, device=DEV) if x is None else x
        sel = torch.arange(T, device=DEV).repeat(L, 1) if sel is None else sel
        seg = torch.linspace(0, d, L + 1).long().to(DEV) if seg is None else seg
        out = torch.zeros(d, device=DEV) if out is None else out
        ops.segment_mean_around(x, sel, seg, keep, clo, chi, out)

    call()  # the shape the rejections below vary
    bad_calls = [
        dict(T=0, keep=1, clo=0, chi=1),           # T outside 1..64
        dict(P=66, T=65, keep=3),
        dict(P=3, T=4),                            # T > P
        dict(keep=0), dict(keep=5), dict(keep=-1),  # keep outside 1..T
        dict(clo=2, chi=2), dict(clo=3, chi=1), dict(clo=0, chi=5), dict(clo=-1, chi=2),
        dict(d=6),                                 # d % 4 != 0
        dict(out=torch.zeros(12, device=DEV)),     # out size
        dict(out=torch.zeros(8)),                  # a CPU tensor (sel and seg are moved)
        dict(out=torch.zeros(8, device=DEV, dtype=torch.float64)),  # dtypes
        dict(x=torch.zeros(6, 8, device=DEV, dtype=torch.float64)),
        dict(x=torch.zeros(6, 8, device=DEV, dtype=torch.bfloat16)),
        dict(sel=torch.arange(4, device=DEV, dtype=torch.int32).repeat(2, 1)),
        dict(seg=torch.tensor([0, 4, 8], device=DEV, dtype=torch.int32)),
        dict(sel=torch.arange(4, device=DEV).repeat(3, 1)),   # sel rows != L
        dict(sel=torch.arange(4, device=DEV).repeat(1, 1)),
        dict(sel=torch.arange(4, device=DEV)),                # sel not 2D
        dict(x=torch.zeros(48, device=DEV)),                  # x not 2D
        dict(seg=torch.zeros(0, dtype=torch.int64, device=DEV), sel=torch.zeros(
            0, 4, dtype=torch.int64, device=DEV)),            # no bounds at all
    ]
    for kw in bad_calls:
        with pytest.raises(RuntimeError):
            call(**kw)
    # the extension itself refuses CPU tensors in every position (ops moves sel and seg)
    from draco_amd.ops.native import require_extension

    ext = require_extension()
    good = [torch.zeros(6, 8, device=DEV), torch.arange(4, device=DEV).repeat(2, 1),
            torch.tensor([0, 4, 8], device=DEV), 3, 1, 3, torch.zeros(8, device=DEV)]
    ext.segment_mean_around(*good)
    for pos in (0, 1, 2, 6):
        args = list(good)
        args[pos] = args[pos].cpu()
        with pytest.raises(RuntimeError):
            ext.segment_mean_around(*args)
    out = torch.zeros(0, device=DEV)
    call(d=0, out=out)  # d = 0: no launch
    torch.cuda.synchronize()
    assert out.numel() == 0
    # L = 0 (one bound, no segment): everything is outside, all +0.0
    out = torch.full((8,), -7.0, device=DEV)
    call(L=0, seg=torch.tensor([3], device=DEV), out=out,
         sel=torch.zeros(0, 4, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


# ------------------------------------------------------------ 5. aggregators, GPU == CPU
@pytest.mark.parametrize("rule", ["bulyan", "multi_krum"])
def test_gpu_aggregator_matches_cpu(rule):
    import torch.nn as nn

    from draco_amd.parallel.aggregators import BulyanAggregator, MultiKrumAggregator
    from draco_amd.parallel.comm import Communicator
    from draco_amd.parallel.flat import FlatSpace

    P, f, adversary = 7, 1, 5
    cls = BulyanAggregator if rule == "bulyan" else MultiKrumAggregator
    payload_cpu = None
    outs, sels = {}, {}
    for dev in ("cpu", DEV):
        device = torch.device(dev)
        torch.manual_seed(5)
        model = nn.Sequential(nn.Linear(300, 40), nn.Linear(40, 9)).to(device)
        space = FlatSpace(model, 1, device)
        agg = cls(Communicator(0, 1, device), space, num_workers=P, f=f)
        if payload_cpu is None:
            payload_cpu = torch.zeros(P, space.d_pad)  # pad tail is always zero in production
            payload_cpu[:, : space.d] = torch.tensor(
                separated_rows(P, space.d, [adversary], seed=9, attack="plus100"))
        payload = space.alloc_payload(P)
        payload.copy_(payload_cpu.to(device))
        outs[dev] = agg.aggregate(payload, step=0).cpu()
        sels[dev] = agg.last_sel.cpu()
    d = space.d
    assert torch.equal(sels[DEV], sels["cpu"])
    assert not bool((sels[DEV] == adversary).any())
    T = P - 2 * f if rule == "bulyan" else P - f
    assert tuple(sels[DEV].shape) == (4, T)
    _assert_same(outs[DEV], outs["cpu"], rule)
    assert torch.equal(outs[DEV][:d].view(torch.int32), outs["cpu"][:d].view(torch.int32))
    honest = payload_cpu[[p for p in range(P) if p != adversary], :d]
    assert bool((outs[DEV][:d] >= honest.min(0).values).all())
    assert bool((outs[DEV][:d] <= honest.max(0).values).all())
    assert bool((outs[DEV][d:] == 0).all())


# ------------------------------------------------------------ 6. trainer steps
@pytest.mark.parametrize("mode", ["multi_krum", "bulyan"])
def test_gpu_trainer_steps(tmp_path, mode):
    from draco_amd.config import Config
    from draco_amd.parallel.trainer import Trainer

    cfg = Config(network="LeNet", dataset="MNIST", batch_size=32, device="cuda", lr=0.02,
                 max_steps=60, eval_freq=0, log_dir="", train_dir=str(tmp_path / "ckpt"),
                 approach="baseline", mode=mode, worker_fail=1, err_mode="rev_grad",
                 workers_per_rank=7)
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    assert t.agg.name == mode and t.P == 7 and t.agg.f == 1
    losses = [t.train_step()["loss"] for _ in range(2)]
    assert np.isfinite(losses).all()
    assert t.skipped_updates == 0
    t.close()
