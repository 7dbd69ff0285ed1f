"""ops.column_trimmed_mean on the MI355X: the HIP kernel against the fp32 fallback,
bit for bit — both sort the same values and add the kept ranks in the same ascending
order, so bit-exactness is the claim (the sign of a zero result is not compared).

Layout facts the shapes are chosen for (ops/csrc/draco_kernels.hip): one column per
lane, 256-thread blocks, grid capped at 2048 blocks, so one grid-stride trip covers
2048*256 = 524 288 columns; the column is sorted in registers padded with +inf to
N in {4, 8, 12, 16, 24, 32, 48, 64} rows, the smallest N >= P.
"""
import numpy as np
import pytest
import torch

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


def _median_bounds(P):
    return (P - 1) // 2, P // 2 + 1


def _data(P, d, seed):
    """Gaussian columns, with every third column drawn from a 16-value grid (ties)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, d, generator=g, dtype=torch.float32)
    grid = (torch.randint(0, 16, (P, d), generator=g).float() - 8.0) / 4.0
    x[:, ::3] = grid[:, ::3]
    return x


def _gpu(x, lo, hi):
    out = torch.full((x.shape[1],), -7.0, dtype=torch.float32, device=DEV)
    ops.column_trimmed_mean(x.to(DEV), lo, hi, out)
    torch.cuda.synchronize()
    return out.cpu()


def _cpu(x, lo, hi):
    out = torch.empty(x.shape[1], dtype=torch.float32)
    fb.column_trimmed_mean(x, lo, hi, out)
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
    x = _data(P, 4096, seed=P)
    cases = {_median_bounds(P), (0, P)}
    if P >= 3:
        cases.add((1, P - 1))
    for lo, hi in sorted(cases):
        _assert_same(_gpu(x, lo, hi), _cpu(x, lo, hi), (P, lo, hi))


# ------------------------------------------------------------ 2. grid-stride second trip
def test_second_grid_stride_trip_and_smallest_shape():
    P, d = 3, TRIP + 8  # one full trip of 2048x256 lanes plus 8 columns of a second
    x = _data(P, d, seed=77)
    x[:, TRIP] = torch.tensor([1000.0, 3000.0, 2000.0])
    x[:, d - 1] = torch.tensor([-6000.0, -4000.0, -5000.0])
    for lo, hi in [_median_bounds(P), (0, P)]:
        got = _gpu(x, lo, hi)
        _assert_same(got, _cpu(x, lo, hi), (lo, hi))
    med = _gpu(x, *_median_bounds(P))
    assert float(med[TRIP]) == 2000.0 and float(med[d - 1]) == -5000.0
    xs = _data(P, 4, seed=78)
    _assert_same(_gpu(xs, 1, 2), _cpu(xs, 1, 2), "d=4")
    _assert_same(_gpu(xs, 0, 3), _cpu(xs, 0, 3), "d=4")


# ------------------------------------------------------------ 3. planted non-finites
D_NF = 1024
NF_COLS = [0, 63, 64, 255, 256, D_NF - 1]  # lane, wave and block edges


@pytest.fixture(scope="module")
def clean_nf():
    x = _data(5, D_NF, seed=5)
    return x, {b: _gpu(x, *b) for b in [(1, 4), _median_bounds(5)]}


@pytest.mark.parametrize("bad", BADS)
@pytest.mark.parametrize("row", [0, 4])
def test_planted_nonfinite(clean_nf, bad, row):
    clean, clean_out = clean_nf
    x = clean.clone()
    x[row, NF_COLS] = bad
    other = torch.ones(D_NF, dtype=torch.bool)
    other[NF_COLS] = False
    for (lo, hi), ref_clean in clean_out.items():
        got = _gpu(x, lo, hi)
        assert torch.equal(got[other].view(torch.int32), ref_clean[other].view(torch.int32))
        _assert_same(got, _cpu(x, lo, hi), (bad, row, lo, hi))
        assert bool(torch.isfinite(got).all())  # one bad row, at least one trimmed per end


def test_opposite_nonfinite_rows_are_both_trimmed(clean_nf):
    clean, _ = clean_nf
    for hi_bad in (float("nan"), INF):
        x = clean.clone()
        x[0, NF_COLS] = hi_bad
        x[4, NF_COLS] = -INF
        got = _gpu(x, 1, 4)
        assert bool(torch.isfinite(got).all())
        _assert_same(got, _cpu(x, 1, 4), hi_bad)


def test_both_infinities_in_kept_range_give_nan(clean_nf):
    clean, _ = clean_nf
    x = clean.clone()
    x[0, NF_COLS] = INF
    x[4, NF_COLS] = -INF
    got, ref = _gpu(x, 0, 5), _cpu(x, 0, 5)
    assert bool(torch.isnan(ref[NF_COLS]).all())
    _assert_same(got, ref, "inf-inf")


# ------------------------------------------------------------ 4. host-side rejections
def test_host_rejections():
    def call(P, d, lo, hi, out=None, x=None):
        x = torch.zeros(P, d, device=DEV) if x is None else x
        out = torch.zeros(d, device=DEV) if out is None else out
        ops.column_trimmed_mean(x, lo, hi, out)

    with pytest.raises(RuntimeError):
        call(65, 8, 0, 1)
    with pytest.raises(RuntimeError):
        call(4, 8, 2, 2)
    with pytest.raises(RuntimeError):
        call(4, 8, 3, 1)
    with pytest.raises(RuntimeError):
        call(4, 8, 0, 5)
    with pytest.raises(RuntimeError):
        call(4, 6, 0, 4)
    with pytest.raises(RuntimeError):
        call(4, 8, 0, 4, out=torch.zeros(12, device=DEV))
    with pytest.raises(RuntimeError):
        call(4, 8, 0, 4, out=torch.zeros(8))
    with pytest.raises(RuntimeError):
        call(4, 8, 0, 4, x=torch.zeros(4, 8, device=DEV, dtype=torch.float64))
    out = torch.zeros(0, device=DEV)
    call(4, 0, 0, 4, out=out)
    torch.cuda.synchronize()
    assert out.numel() == 0


# ------------------------------------------------------------ 5. aggregator, GPU == CPU
@pytest.mark.parametrize("trim", [None, 1])
def test_gpu_aggregator_matches_cpu(trim):
    import torch.nn as nn

    from draco_amd.parallel.aggregators import TrimmedMeanAggregator
    from draco_amd.parallel.comm import Communicator
    from draco_amd.parallel.flat import FlatSpace

    P = 6
    payload_cpu = None
    outs = {}
    for dev in ("cpu", DEV):
        device = torch.device(dev)
        torch.manual_seed(5)
        model = nn.Sequential(nn.Linear(300, 40), nn.Linear(40, 9)).to(device)
        space = FlatSpace(model, 1, device)
        agg = TrimmedMeanAggregator(Communicator(0, 1, device), space, num_workers=P, trim=trim)
        if payload_cpu is None:
            torch.manual_seed(9)
            payload_cpu = torch.randn(P, space.d_pad)
            payload_cpu[:, space.d:] = 0.0  # pad tail is always zero in production
            payload_cpu[5] += 100.0  # the adversary
        payload = space.alloc_payload(P)
        payload.copy_(payload_cpu.to(device))
        outs[dev] = agg.aggregate(payload, step=0).cpu()
    d = space.d
    _assert_same(outs[DEV], outs["cpu"], trim)
    honest = payload_cpu[:5, :d]
    assert bool((outs[DEV][:d] >= honest.min(0).values).all())
    assert bool((outs[DEV][:d] <= honest.max(0).values).all())
    assert bool((outs[DEV][d:] == 0).all())


# ------------------------------------------------------------ 6. trainer steps
@pytest.mark.parametrize("mode", ["median", "trimmed_mean"])
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
