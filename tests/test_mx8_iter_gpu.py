"""ops.mx8_clip_step_ and ops.mx8_weiszfeld_step on the MI355X, then the Trainer.  The clip
step: the fp64 oracle of tests/centered_clip_util.py on the decoded rows, and clip_step_'s bits
on the decoded block.  The Weiszfeld step, against fp64 on the decoded rows: |z - z64| <=
(P+1) * 2^-24 * sum_p |w x| (a chain of P fmaf); the distances at the kernel's own z,
|part - ref| <= (len + 4) * 2^-24 * ref (non-negative terms: the difference and the square
round once each, a sum of len terms in any order adds (len - 1) * 2^-24).
Layout (ops/csrc/draco_kernels.hip): a unit is 256 columns, four per lane; in k_mx8_weiszfeld
a wave owns a run of ceil(units / 4096) consecutive units, so chunk = 4097 * 256 = 1 048 832
is the smallest at which a wave walks more than one unit.
"""
import numpy as np
import pytest
import torch

from tests import mx8_util as U
from tests.centered_clip_util import KINDS, bits, check_step, make_case, weight_patterns

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops import fallback as fb

DEV = "cuda:0"
PS = [1, 5, 24, 25, 33, 64]  # padded-size edges, both sides of the 32 / 48 boundary
SEG = [3, 3, 70, 129, 321, 570]  # chunk 576: empty segment, gaps at both ends, bounds in units
SENTINEL, EPS = -12345.0, 2.0 ** -24


def decoded_gpu(packed_d, chunk):  # the two-launch path's own first kernel
    block = torch.empty(packed_d.shape[0], chunk, device=DEV)
    ops.mx8_unpack(packed_d, block)
    return block


@pytest.mark.parametrize("P", PS)
def test_clip_step_against_fp64_oracle(P):
    for n in [4096] + ([64] if P == 5 else []):
        for k, kind in enumerate(KINDS):
            rows, v0 = make_case(kind, P, n, seed=100 * P + k)
            packed = U.pack(fb, rows.reshape(-1), n).view(P, -1)
            x, pd = torch.from_numpy(U.decode(packed.numpy(), n)), packed.to(DEV)
            nan_row = pd.clone()
            nan_row[0, n:] = 0xFF  # row 0: every scale the NaN scale
            for name, w in weight_patterns(P, seed=P).items():
                what, wd, v = (P, n, kind, name), w.to(DEV), v0.to(DEV)
                d2 = ops.mx8_clip_step_(pd, v, wd)
                check_step(x, v0, w, v.cpu(), d2.cpu(), what)
                v_two, v_again, v_only, v_nan = (v0.to(DEV) for _ in range(4))
                ops.clip_step_(decoded_gpu(pd, n), v_two, wd)
                assert torch.equal(bits(v_two), bits(v)), (what, "v differs from clip_step_'s")
                d2_again = ops.mx8_clip_step_(pd, v_again, wd)
                assert torch.equal(bits(d2_again), bits(d2)), (what, "d2 not repeatable")
                assert ops.mx8_clip_step_(pd, v_only, wd, dist=False) is None
                assert torch.equal(bits(v_only), bits(v)), (what, "dist=False moved v elsewhere")
                if float(w[0]) == 0.0:  # a zero-weight row of NaNs reaches its own distance only
                    d2_nan = ops.mx8_clip_step_(nan_row, v_nan, wd)
                    assert torch.equal(bits(v_nan), bits(v)), (what, "a NaN row with w = 0 moved v")
                    assert bool(torch.isnan(d2_nan[0])) and torch.equal(bits(d2_nan[1:]), bits(d2[1:]))


def check_part(part, x64, z, seg, what):
    """part against fp64 at the kernel's own z; a non-finite reference must come out NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = (x64 - z.double().numpy()[None, :]) ** 2
    for l, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        ref, got = d2[:, lo:hi].sum(axis=1), part[:, l].double().numpy()
        fin = np.isfinite(ref)
        assert np.isnan(got[~fin]).all(), (what, l, "a non-finite distance came out finite")
        # an empty segment has ref = 0: exactly 0
        assert (np.abs(got[fin] - ref[fin]) <= (hi - lo + 4) * EPS * ref[fin]).all(), (what, l)


@pytest.mark.parametrize("chunk,seg", [(576, SEG), (1088, [0, 5, 1030, 1088])])
@pytest.mark.parametrize("P", PS)
def test_weiszfeld_step_against_fp64(P, chunk, seg):
    """Update, measuring pass (w None: z only read), dist=False; then a NaN scale on block
    [96, 128), inside one segment of either case, in row P // 2."""
    L, segd = len(seg) - 1, torch.tensor(seg, device=DEV)
    packed = U.pack(fb, U.random_case(P * chunk, seed=P), chunk).view(P, -1).clone()
    x64, pd = U.decode(packed.numpy(), chunk).astype(np.float64), packed.to(DEV)
    w = torch.rand(P, L, generator=torch.Generator().manual_seed(P)) + 0.05
    w = (w / w.sum(dim=0, keepdim=True)).contiguous()
    z = torch.full((chunk,), SENTINEL, device=DEV)
    part = ops.mx8_weiszfeld_step(pd, w.to(DEV), segd, z).cpu()
    z_two = torch.full((chunk,), SENTINEL, device=DEV)
    ops.segment_weighted_mean(decoded_gpu(pd, chunk), w.to(DEV), segd, z_two)
    assert torch.equal(bits(z), bits(z_two)), "z differs from segment_weighted_mean's"
    zc, inside = z.cpu(), np.zeros(chunk, dtype=bool)
    for l, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        wl = w[:, l].double().numpy()[:, None]
        err = np.abs(zc[lo:hi].double().numpy() - (wl * x64[:, lo:hi]).sum(axis=0))
        assert (err <= (P + 1) * EPS * np.abs(wl * x64[:, lo:hi]).sum(axis=0)).all(), l
        inside[lo:hi] = True
    assert bool((zc[torch.from_numpy(~inside)] == SENTINEL).all()), "a column outside was written"
    check_part(part, x64, zc, seg, "update")
    check_part(ops.mx8_weiszfeld_step(pd, None, segd, z).cpu(), x64, zc, seg, "measure")
    z_only = torch.full((chunk,), SENTINEL, device=DEV)
    assert ops.mx8_weiszfeld_step(pd, w.to(DEV), segd, z_only, dist=False) is None
    assert torch.equal(bits(z), bits(zc.to(DEV))) and torch.equal(bits(z_only), bits(z))
    r, l_nan = P // 2, next(l for l in range(L) if seg[l] <= 96 and 128 <= seg[l + 1])
    pd[r, chunk + 3], x64[r, 96:128] = 0xFF, np.nan
    got = ops.mx8_weiszfeld_step(pd, None, segd, z).cpu()
    check_part(got, x64, zc, seg, "NaN block, measure")
    assert int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got[r, l_nan]))
    z_nan = torch.full((chunk,), SENTINEL, device=DEV)
    got = ops.mx8_weiszfeld_step(pd, w.to(DEV), segd, z_nan).cpu()
    zn = z_nan.cpu()
    assert bool(torch.isnan(zn[96:128]).all()) and bool(torch.isnan(got[:, l_nan]).all())
    zn[96:128] = zc[96:128]  # every other column keeps its bits
    assert torch.equal(bits(zn), bits(zc)) and int(torch.isnan(got).sum()) == P


def test_weiszfeld_multi_unit_run_is_exact():
    """chunk = 4097 * 256 (module docstring): every wave but the last owns two units.  Bounds at
    256 (between wave 0's two units: a flush of the register accumulators), at 700 (inside wave
    1's first unit) and 300 / 100 columns before the end (the last two units, a gap behind).
    Small integers around every bound and dyadic weights: every sum is exact in fp32."""
    P, chunk = 3, 4097 * 256
    seg = [0, 256, 700, chunk - 300, chunk - 100]
    cols = [0, 255, 256, 511, 512, 699, 700, 767, 768, 1023, 500_000, chunk - 301, chunk - 300,
            chunk - 257, chunk - 256, chunk - 101, chunk - 100, chunk - 1]
    g = torch.Generator().manual_seed(0)
    rows = torch.zeros(P, chunk)
    rows[:, cols] = torch.randint(-3, 4, (P, len(cols)), generator=g).float()
    pd = U.pack(ops, rows.reshape(-1).to(DEV), chunk).view(P, -1)
    assert torch.equal(decoded_gpu(pd, chunk).cpu(), rows)  # small integers survive the wire
    w = torch.tensor([[0.5, 0.25, 0.25, 0.5], [0.25, 0.5, 0.25, 0.25], [0.25, 0.25, 0.5, 0.25]])
    z = torch.full((chunk,), SENTINEL, device=DEV)
    part = ops.mx8_weiszfeld_step(pd, w.to(DEV), torch.tensor(seg, device=DEV), z).cpu().double()
    z, x64 = z.cpu().double(), rows.double()
    for l, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        z64 = (w[:, l].double()[:, None] * x64[:, lo:hi]).sum(dim=0)
        assert torch.equal(z[lo:hi], z64), l
        assert torch.equal(part[:, l], ((x64[:, lo:hi] - z64) ** 2).sum(dim=1)), l
    assert bool((z[chunk - 100:] == SENTINEL).all()) and float(part.sum()) > 0


def test_host_rejections():
    u8, f = torch.zeros(65 * 80, dtype=torch.uint8, device=DEV), torch.zeros(128, device=DEV)
    p2, seg = u8[:160].view(2, 80), torch.tensor([0, 64], device=DEV)
    w1, w2 = torch.zeros(2, device=DEV), torch.zeros(2, 1, device=DEV)
    cases = [(u8.view(65, 80), f[:64], torch.zeros(65, device=DEV), torch.zeros(65, 1, device=DEV)),
             (u8[:192].view(2, 96), f[:64], w1, w2),                     # a wrong record length
             (p2.int(), f[:64], w1, w2), (p2, f[:64].double(), w1, w2),  # dtypes
             (p2, f[:64], torch.zeros(3, device=DEV), torch.zeros(2, 2, device=DEV)),  # w shape
             (p2, f, w1, w2), (p2, f[:64].cpu(), w1, w2)]                # v / z length, a CPU v / z
    for packed, vz, w, ws in cases:
        with pytest.raises(RuntimeError):
            ops.mx8_clip_step_(packed, vz, w)
        with pytest.raises(RuntimeError):
            ops.mx8_weiszfeld_step(packed, ws, seg, vz)
    many = torch.zeros(2001, dtype=torch.long, device=DEV)  # 2000 x 64 LDS partials
    with pytest.raises(RuntimeError):
        ops.mx8_weiszfeld_step(u8[:64 * 80].view(64, 80), None, many, f[:64])
    empty = u8[:0].view(2, 0)  # chunk = 0: no launch
    assert ops.mx8_clip_step_(empty, f[:0], w1).tolist() == [0.0, 0.0]
    assert ops.mx8_weiszfeld_step(empty, w2, seg, f[:0]).tolist() == [[0.0], [0.0]]


@pytest.mark.parametrize("mode", ["geometric_median", "centered_clip"])
def test_trainer_runs_the_rule_on_the_records(mode, tmp_path):
    from draco_amd.config import Config
    from draco_amd.parallel.trainer import Trainer
    t = Trainer(Config(network="ResNet18", dataset="Cifar10", batch_size=32, device="cuda", lr=0.02,
                       dtype="bf16", eval_freq=0, log_dir="", train_dir=str(tmp_path / "ckpt"),
                       approach="baseline", mode=mode, compress_grad="mx8", worker_fail=1,
                       err_mode="rev_grad", workers_per_rank=4, max_steps=60))
    t.logger.stdout_every = 0
    losses = [t.train_step()["loss"] for _ in range(2)]
    assert t.agg.wire == "mx8" and t.agg._recv32 is None
    assert np.isfinite(losses).all() and t.skipped_updates == 0
    t.close()
