"""ops.column_mean_around on the MI355X: the HIP kernel against the fp32 fallback, bit
for bit — both sort the same values, compute the centre, count the window start and
add the kept ranks in the same order, so bit-exactness is the claim (NaN positions
must be equal; the sign of a zero result is not compared).

Layout facts the shapes are chosen for (ops/csrc/draco_kernels.hip): one column per
lane, 256-thread blocks, grid capped at 2048 blocks, so one grid-stride trip covers
2048*256 = 524 288 columns; the column is sorted in registers padded with +inf to
N in {4, 8, 12, 16, 24, 32, 48, 64} rows, the smallest N >= P; the window start
compares s[j] with s[j + keep] through a log2(N)-stage shifter driven by the bits of
keep, so every P (hence every keep) takes its own path through the stages.
"""
import numpy as np
import pytest
import torch

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


def _gpu(x, keep, clo, chi):
    out = torch.full((x.shape[1],), -7.0, dtype=torch.float32, device=DEV)
    ops.column_mean_around(x.to(DEV), keep, clo, chi, out)
    torch.cuda.synchronize()
    return out.cpu()


def _cpu(x, keep, clo, chi):
    out = torch.empty(x.shape[1], dtype=torch.float32)
    fb.column_mean_around(x, keep, clo, chi, out)
    return out


def _assert_same(got, ref, what):
    nan_g, nan_r = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(nan_g, nan_r), (what, "NaN positions differ")
    ok = (got == ref) | nan_r
    assert bool(ok.all()), (what, int((~ok).sum()), int((~ok).nonzero()[0]))


# ------------------------------------------------------------ 1. kernel == fallback
# every padded size at its lower edge, its upper edge and (where there is room) inside
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48,
                               49, 63, 64])
def test_kernel_equals_fallback_bitwise(P):
    base = data(P, 4096, seed=P)
    for b in legal_bs(P):
        x = base.clone()
        plant(x, b, col0=1024)  # every window start 0..b, far outliers on both sides
        xg = x.to(DEV)
        for center in CENTERS:
            keep, clo, chi = bounds(P, b, center)
            _, _, w = fb.mean_around_window(x, keep, clo, chi)
            assert set(w.tolist()) == set(range(b + 1)), (P, b, center)
            out = torch.full((x.shape[1],), -7.0, dtype=torch.float32, device=DEV)
            ops.column_mean_around(xg, keep, clo, chi, out)
            _assert_same(out.cpu(), _cpu(x, keep, clo, chi), (P, b, center))
    # keep = P with a centre of its own, and the full-range centre
    _assert_same(_gpu(base, P, 0, P), _cpu(base, P, 0, P), (P, "keep=P"))
    if P >= 2:
        _assert_same(_gpu(base, 1, 0, 1), _cpu(base, 1, 0, 1), (P, "keep=1"))


# ------------------------------------------------------------ 2. grid-stride second trip
def test_second_grid_stride_trip_and_smallest_shape():
    P, b, d = 3, 1, TRIP + 8  # one full trip of 2048x256 lanes plus 8 columns of a second
    x = data(P, d, seed=77)
    x[:, TRIP] = torch.tensor([1000.0, 3100.0, 2000.0])      # top is farther: w = 0
    x[:, d - 1] = torch.tensor([-6200.0, -4000.0, -5000.0])  # bottom is farther: w = 1
    ref = {}
    for center in CENTERS:
        keep, clo, chi = bounds(P, b, center)
        ref[center] = _cpu(x, keep, clo, chi)
        got = _gpu(x, keep, clo, chi)
        _assert_same(got, ref[center], center)
        assert float(got[TRIP]) == 1500.0 and float(got[d - 1]) == -4500.0
    xs = data(P, 4, seed=78)
    _assert_same(_gpu(xs, 2, 1, 2), _cpu(xs, 2, 1, 2), "d=4")
    _assert_same(_gpu(xs, 3, 1, 2), _cpu(xs, 3, 1, 2), "d=4")


# ------------------------------------------------------------ 3. planted non-finites
D_NF = 1024
NF_COLS = [0, 63, 64, 255, 256, D_NF - 1]  # lane, wave and block edges
NF_CASES = [bounds(5, 2, c) for c in CENTERS]


@pytest.fixture(scope="module")
def clean_nf():
    x = data(5, D_NF, seed=5)
    return x, {case: _gpu(x, *case) for case in NF_CASES}


@pytest.mark.parametrize("bad", BADS)
@pytest.mark.parametrize("row", [0, 4])
def test_planted_nonfinite(clean_nf, bad, row):
    clean, clean_out = clean_nf
    x = clean.clone()
    x[row, NF_COLS] = bad
    other = torch.ones(D_NF, dtype=torch.bool)
    other[NF_COLS] = False
    for case, ref_clean in clean_out.items():
        got = _gpu(x, *case)
        assert torch.equal(got[other].view(torch.int32), ref_clean[other].view(torch.int32))
        _assert_same(got, _cpu(x, *case), (bad, row, case))
        assert bool(torch.isfinite(got).all())  # one bad row, b = 2


def test_opposite_nonfinite_rows_stay_outside_the_window(clean_nf):
    clean, _ = clean_nf
    for hi_bad in (float("nan"), INF):
        x = clean.clone()
        x[0, NF_COLS] = hi_bad
        x[4, NF_COLS] = -INF
        for case in NF_CASES:
            got = _gpu(x, *case)
            assert bool(torch.isfinite(got).all())
            _assert_same(got, _cpu(x, *case), (hi_bad, case))


def test_more_nonfinite_rows_than_b_match_the_fallback(clean_nf):
    clean, _ = clean_nf
    x = clean.clone()
    x[0, NF_COLS] = INF
    x[2, NF_COLS] = float("nan")
    x[4, NF_COLS] = -INF
    x[1, NF_COLS[:3]] = -INF
    for case in NF_CASES:
        _assert_same(_gpu(x, *case), _cpu(x, *case), case)


# ------------------------------------------------------------ 4. host-side rejections
def test_host_rejections():
    def call(P, d, keep, clo, chi, out=None, x=None):
        x = torch.zeros(P, d, device=DEV) if x is None else x
        out = torch.zeros(d, device=DEV) if out is None else out
        ops.column_mean_around(x, keep, clo, chi, out)

    call(4, 8, 3, 1, 3)  # the shape the rejections below vary
    bad_calls = [
        dict(P=65, d=8, keep=64, clo=0, chi=1),   # P outside 1..64
        dict(P=4, d=8, keep=0, clo=1, chi=3),     # keep outside 1..P
        dict(P=4, d=8, keep=5, clo=1, chi=3),
        dict(P=4, d=8, keep=-1, clo=1, chi=3),
        dict(P=4, d=8, keep=3, clo=2, chi=2),     # bad clo / chi
        dict(P=4, d=8, keep=3, clo=3, chi=1),
        dict(P=4, d=8, keep=3, clo=0, chi=5),
        dict(P=4, d=8, keep=3, clo=-1, chi=2),
        dict(P=4, d=6, keep=3, clo=1, chi=3),     # d % 4 != 0
        dict(P=4, d=8, keep=3, clo=1, chi=3, out=torch.zeros(12, device=DEV)),
        dict(P=4, d=8, keep=3, clo=1, chi=3, out=torch.zeros(8)),  # out not on the GPU
        dict(P=4, d=8, keep=3, clo=1, chi=3,
             out=torch.zeros(8, device=DEV, dtype=torch.float64)),
        dict(P=4, d=8, keep=3, clo=1, chi=3,
             x=torch.zeros(4, 8, device=DEV, dtype=torch.float64)),
        dict(P=4, d=8, keep=3, clo=1, chi=3,
             x=torch.zeros(4, 8, device=DEV, dtype=torch.bfloat16)),
    ]
    for kw in bad_calls:
        with pytest.raises(RuntimeError):
            call(**kw)
    with pytest.raises(RuntimeError):  # P = 0
        call(0, 8, 1, 0, 1)
    out = torch.zeros(0, device=DEV)
    call(4, 0, 3, 1, 3, out=out)  # d = 0: no launch
    torch.cuda.synchronize()
    assert out.numel() == 0


# ------------------------------------------------------------ 5. aggregator, GPU == CPU
@pytest.mark.parametrize("center", CENTERS)
def test_gpu_aggregator_matches_cpu(center):
    import torch.nn as nn

    from draco_amd.parallel.aggregators import MeanAroundAggregator
    from draco_amd.parallel.comm import Communicator
    from draco_amd.parallel.flat import FlatSpace

    P, b = 6, 1
    payload_cpu = None
    outs = {}
    for dev in ("cpu", DEV):
        device = torch.device(dev)
        torch.manual_seed(5)
        model = nn.Sequential(nn.Linear(300, 40), nn.Linear(40, 9)).to(device)
        space = FlatSpace(model, 1, device)
        agg = MeanAroundAggregator(Communicator(0, 1, device), space, num_workers=P, b=b,
                                   center=center)
        if payload_cpu is None:
            torch.manual_seed(9)
            payload_cpu = torch.randn(P, space.d_pad)
            payload_cpu[:, space.d:] = 0.0  # pad tail is always zero in production
            payload_cpu[5] += 100.0  # the adversary
        payload = space.alloc_payload(P)
        payload.copy_(payload_cpu.to(device))
        outs[dev] = agg.aggregate(payload, step=0).cpu()
    d = space.d
    _assert_same(outs[DEV], outs["cpu"], center)
    assert torch.equal(outs[DEV][:d].view(torch.int32), outs["cpu"][:d].view(torch.int32))
    # the +100 row is the farthest value of every coordinate: the five honest rows remain
    honest = payload_cpu[:5, :d]
    assert bool((outs[DEV][:d] >= honest.min(0).values).all())
    assert bool((outs[DEV][:d] <= honest.max(0).values).all())
    assert bool((outs[DEV][d:] == 0).all())


# ------------------------------------------------------------ 6. trainer steps
@pytest.mark.parametrize("mode", ["meamed", "phocas"])
def test_gpu_trainer_steps(tmp_path, mode):
    from draco_amd.config import Config
    from draco_amd.parallel.trainer import Trainer

    cfg = Config(network="ResNet18", dataset="Cifar10", batch_size=32, device="cuda",
                 lr=0.02, dtype="bf16", max_steps=60, eval_freq=0, log_dir="",
                 train_dir=str(tmp_path / "ckpt"), approach="baseline", mode=mode,
                 worker_fail=1, err_mode="rev_grad", workers_per_rank=3)
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    assert t.agg.name == mode and t.P == 3
    losses = [t.train_step()["loss"] for _ in range(2)]
    assert np.isfinite(losses).all()
    assert t.skipped_updates == 0
    t.close()
