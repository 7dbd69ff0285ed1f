"""HIP kernels at their edges, against float64 references built from each op's
definition (the fp32 fallback is the oracle only where bit-exactness is the claim).

Layout facts these shapes are chosen for (ops/csrc/draco_kernels.hip): blocks are 256
threads = 4 waves of 64 lanes, one float4 per lane per trip; grids are capped at 2048
blocks, so the float4 elementwise kernels take a second grid-stride trip only past
d = 4*2048*256 = 2 097 152 floats (k_seg_wmean, one float per lane: past 524 288).
The two row-max kernels launch d/32/256 blocks: d = 65 536 gives 8 blocks x 8 trips.

Error bounds (u = 2^-24, the fp32 unit roundoff):
  * linear combinations of m rows: |got - ref| <= (m+1) u sum_i|w_i x_i| per element
    (m chained FMAs, one rounding each, plus one for a rounded weight);
  * reductions of length n: |got - ref| <= (n+4) u sum|terms| per output;
  * optimizers: 4x the fp32 fallback's own max error against the float64 reference on
    the same inputs (FMA contraction and operation order differ by a few roundings in
    either direction) — computed inside each test and printed.
"""
import numpy as np
import pytest
import torch

from tests.test_vote_security import NONFINITE, NONFINITE_GRID, nonfinite_vote_case

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops import fallback as fb
    from draco_amd.ops.native import available, require_extension

    assert available(), "HIP extension must be built and importable on the GPU box"

DEV = "cuda:0"
U = 2.0 ** -24
INF = float("inf")
BADS = (float("nan"), INF, -INF)

D_ROW = 65536
# 0 / 3: first float4 of lane 0; 255: last lane of wave 0; 256: wave 1; 1023: last
# lane of wave 3 (LDS cross-wave step); 1024: block 1; 8192: first element of the
# second grid-stride trip (8 blocks x 256 lanes x 4 floats); d-1
ROW_POS = [0, 3, 4 * 63 + 3, 4 * 64, 4 * 255 + 3, 4 * 256, 4 * 8 * 256, D_ROW - 1]

# leading gap [0,64), trailing gap [8000,8192), an empty segment, a length-1 segment,
# boundaries on (64, 128, 4096, 8000) and off (129, 200) multiples of the wave
SEG = [64, 128, 129, 129, 200, 4096, 8000]
D_SEG = 8192

D_CAP = 2_098_180  # 524 545 float4: one full trip of 2048x256 plus a partial second
CAP_TAIL = 4 * 2048 * 256


def _u(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float32) * 2 - 1


def _r(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _bits_equal(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32),
                       b.cpu().contiguous().view(torch.int32))


def _check_bound(name, got, ref64, bound64):
    """assert |got - ref| <= bound elementwise; print the worst error/bound ratio."""
    err = (got.detach().cpu().double() - ref64).abs()
    nz = bound64 > 0
    ratio = float((err[nz] / bound64[nz]).max()) if bool(nz.any()) else 0.0
    print(f"[edges] {name}: worst err/bound = {ratio:.4f}")
    assert bool((err <= bound64).all()), (name, ratio, float(err.max()))


# ============================================================ C1: planted maxima
_PA = torch.tensor([0, 1, 0, 3])
_PB = torch.tensor([2, 2, 2, 3])  # pair 2 repeats pair 0; pair 3 is a == b


@pytest.fixture(scope="module")
def rows_cpu():
    return _u(5, D_ROW, seed=100)


@pytest.mark.parametrize("p", ROW_POS)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_row_max_kernels_find_planted_maximum(rows_cpu, p, sign):
    x = rows_cpu.clone()
    x[0, p] = sign * 10.0
    x[2, p] = 0.0  # pair (0, 2) then differs by exactly 10 at p
    xg = x.to(DEV)
    got = ops.row_absmax(xg).cpu()
    assert float(got[0]) == 10.0
    assert _bits_equal(got, fb.row_absmax(x))
    got = ops.pair_maxdiff(xg, _PA, _PB).cpu()
    assert got.tolist()[0] == 10.0 and got.tolist()[2] == 10.0 and got.tolist()[3] == 0.0
    assert _bits_equal(got, fb.pair_maxdiff(x, _PA, _PB))


@pytest.mark.parametrize("d", [4, 36])
def test_row_max_kernels_single_partial_wave(d):
    x = _u(3, d, seed=101)
    a, b = torch.tensor([0, 1, 2]), torch.tensor([1, 2, 2])
    for p in (0, d - 1):
        y = x.clone()
        y[1, p] = -10.0
        y[2, p] = 0.0
        got = ops.row_absmax(y.to(DEV)).cpu()
        assert float(got[1]) == 10.0 and _bits_equal(got, fb.row_absmax(y))
        got = ops.pair_maxdiff(y.to(DEV), a, b).cpu()
        assert float(got[1]) == 10.0 and float(got[2]) == 0.0
        assert _bits_equal(got, fb.pair_maxdiff(y, a, b))


def test_row_max_kernels_single_row_and_pair(rows_cpu):
    x = rows_cpu[:2].clone()
    x[0, 777] = 10.0
    x[1, 777] = 0.0
    got = ops.row_absmax(x[:1].contiguous().to(DEV)).cpu()
    assert got.shape == (1,) and float(got[0]) == 10.0
    got = ops.pair_maxdiff(x.to(DEV), torch.tensor([1]), torch.tensor([0])).cpu()
    assert got.shape == (1,) and float(got[0]) == 10.0


@pytest.mark.parametrize("p", ROW_POS)
def test_rows_equal_one_ulp_and_nan(rows_cpu, p):
    x = rows_cpu[:3].clone()
    x[1] = x[0]
    x[1, p] = torch.nextafter(x[0, p], torch.tensor(2.0))  # 1 ulp, < 1.2e-7 on [-1, 1]
    a, b = torch.tensor([0, 0, 0]), torch.tensor([1, 0, 2])
    xg = x.to(DEV)
    assert ops.rows_equal(xg, a, b, 0.0).cpu().tolist() == [0, 1, 0]
    assert ops.rows_equal(xg, a, b, 1e-6).cpu().tolist() == [1, 1, 0]
    x[1, p] = float("nan")
    xg = x.to(DEV)
    for atol in (0.0, 1e-6, 1e9):
        got = ops.rows_equal(xg, a, b, atol).cpu()
        assert got.tolist()[:2] == [0, 1], atol
        assert torch.equal(got, fb.rows_equal(x, a, b, atol))


# ============================================================ C2: non-finite rule
@pytest.mark.parametrize("p", ROW_POS)
def test_row_max_kernels_nonfinite_rule(rows_cpu, p):
    clean_row = fb.row_absmax(rows_cpu)
    clean_pair = fb.pair_maxdiff(rows_cpu, _PA, _PB)
    for bad in BADS:
        x = rows_cpu.clone()
        x[0, p] = bad
        xg = x.to(DEV)
        got = ops.row_absmax(xg).cpu()
        exp = clean_row.clone()
        exp[0] = INF
        assert _bits_equal(got, exp), (bad, got)
        assert _bits_equal(got, fb.row_absmax(x))
        got = ops.pair_maxdiff(xg, _PA, _PB).cpu()
        exp = clean_pair.clone()
        exp[0] = exp[2] = INF
        assert _bits_equal(got, exp), (bad, got)
        assert _bits_equal(got, fb.pair_maxdiff(x, _PA, _PB))
    # Inf at the same column of both rows of the pair: Inf - Inf counts as non-finite
    x = rows_cpu.clone()
    x[0, p] = x[2, p] = INF
    got = ops.pair_maxdiff(x.to(DEV), _PA, _PB).cpu()
    assert got.tolist()[0] == INF and got.tolist()[1] == INF and got.tolist()[3] == 0.0
    assert _bits_equal(got, fb.pair_maxdiff(x, _PA, _PB))


@pytest.fixture(scope="module")
def seg_rows_cpu():
    return _u(4, D_SEG, seed=102)


def _seg_of(c):
    for l in range(len(SEG) - 1):
        if SEG[l] <= c < SEG[l + 1]:
            return l
    return None


# whole wave in one segment (register pre-reduce path): lanes 0 and 63 of wave
# [64,128) = segment 0, of wave [256,320) and of wave [4096,4160) (second trip);
# waves straddling a boundary (per-lane LDS path): 128 | 129..191 and 199 | 200;
# gaps: 0, 63, 8000, 8191
SEG_POS = [64, 127, 256, 319, 4096, 4159, 7999, 128, 129, 191, 192, 199, 200, 255,
           0, 63, 8000, 8191]


@pytest.mark.parametrize("c", SEG_POS)
def test_segment_max_kernels_nonfinite_rule(seg_rows_cpu, c):
    seg = torch.tensor(SEG, dtype=torch.int64)
    a, b = torch.tensor([0, 1, 0]), torch.tensor([2, 3, 2])
    clean_max = fb.segment_absmax(seg_rows_cpu, seg)
    clean_diff = fb.segment_pair_maxdiff(seg_rows_cpu, a, b, seg)
    assert _bits_equal(ops.segment_absmax(seg_rows_cpu.to(DEV), seg), clean_max)
    assert _bits_equal(ops.segment_pair_maxdiff(seg_rows_cpu.to(DEV), a, b, seg), clean_diff)
    l = _seg_of(c)
    for bad in BADS:
        x = seg_rows_cpu.clone()
        x[2, c] = bad
        xg = x.to(DEV)
        exp_max, exp_diff = clean_max.clone(), clean_diff.clone()
        if l is not None:  # in a gap the plant must have no effect at all
            exp_max[2, l] = INF
            exp_diff[0, l] = exp_diff[2, l] = INF
        got = ops.segment_absmax(xg, seg).cpu()
        assert _bits_equal(got, exp_max), (bad, c)
        assert _bits_equal(got, fb.segment_absmax(x, seg))
        got = ops.segment_pair_maxdiff(xg, a, b, seg).cpu()
        assert _bits_equal(got, exp_diff), (bad, c)
        assert _bits_equal(got, fb.segment_pair_maxdiff(x, a, b, seg))
    x = seg_rows_cpu.clone()
    x[0, c] = x[2, c] = INF  # Inf - Inf inside the pair
    got = ops.segment_pair_maxdiff(x.to(DEV), a, b, seg).cpu()
    assert _bits_equal(got, fb.segment_pair_maxdiff(x, a, b, seg))
    if l is not None:
        assert float(got[0, l]) == INF


@pytest.mark.parametrize("granularity,rtol,bad,plant,slot", NONFINITE_GRID)
def test_nonfinite_adversary_loses_the_vote_on_device(granularity, rtol, bad, plant, slot):
    out, g, agg = nonfinite_vote_case(DEV, granularity, rtol, [slot], NONFINITE[bad], plant)
    assert out.is_cuda
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, g), float((out - g).abs().max())
    assert agg.degenerate_steps == 0


# ============================================================ optimizers (C3, C4)
def _sgd_ref64(p, g, buf, *, lr, momentum, dampening, weight_decay, nesterov, first_step):
    d_p = g + weight_decay * p
    if momentum != 0.0:
        buf = momentum * buf + (1.0 if first_step else 1.0 - dampening) * d_p
        d_p = d_p + momentum * buf if nesterov else buf
    return p - lr * d_p, buf


def _adam_ref64(p, g, m, v, vmax, *, step, lr, beta1, beta2, eps, weight_decay, amsgrad):
    g = g + weight_decay * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    if amsgrad:
        vmax = torch.maximum(vmax, v)
        denom = vmax.sqrt() + eps
    else:
        denom = v.sqrt() + eps
    step_size = lr * (1.0 - beta2 ** step) ** 0.5 / (1.0 - beta1 ** step)
    return p - step_size * m / denom, m, v, vmax


def _assert_4x_fallback(tag, names, kernel, fallback, ref64):
    """kernel error <= 4x the fallback's own max error vs float64, per state array."""
    for name, k, f, r in zip(names, kernel, fallback, ref64):
        e_fb = float((f.double() - r).abs().max())
        e_k = float((k.cpu().double() - r).abs().max())
        print(f"[edges] {tag} {name}: fallback_err={e_fb:.3e} kernel_err={e_k:.3e} "
              f"allowed={4 * e_fb:.3e}")
        assert e_k <= 4 * e_fb, (tag, name, e_k, e_fb)


def _run_sgd(d, firsts, cfg, seed, buf0_random=False):
    p0 = _r(d, seed=seed)
    buf0 = _r(d, seed=seed + 1) if buf0_random else torch.zeros(d)
    grads = [_r(d, seed=seed + 2 + t) for t in range(len(firsts))]
    use_buf = cfg["momentum"] != 0.0
    pf, bf = p0.clone(), buf0.clone()
    pk, bk = p0.to(DEV), buf0.to(DEV)
    pr, br = p0.double(), buf0.double()
    for g, first in zip(grads, firsts):
        fb.fused_sgd_step(pf, g, bf if use_buf else None, first_step=first, **cfg)
        ops.fused_sgd_step(pk, g.to(DEV), bk if use_buf else None, first_step=first, **cfg)
        pr, br = _sgd_ref64(pr, g.double(), br, first_step=first, **cfg)
    return p0, buf0, (pk, bk), (pf, bf), (pr, br)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("dampening", [0.0, 0.1])
def test_sgd_instances_and_state(momentum, nesterov, wd, dampening):
    """Three steps, the first with first_step=True (no (1-dampening) factor: the
    reference's first-step quirk, reproduced by the float64 reference)."""
    cfg = dict(lr=0.1, momentum=momentum, dampening=dampening, weight_decay=wd,
               nesterov=nesterov)
    _, buf0, kern, fall, ref = _run_sgd(4096 + 64, (True, False, False), cfg, seed=200)
    tag = f"sgd mom={momentum} nest={nesterov} wd={wd} damp={dampening}"
    if momentum == 0.0:  # k_sgd<false,false>: buf is never touched
        assert torch.equal(kern[1].cpu(), buf0)
        _assert_4x_fallback(tag, ["p"], kern[:1], fall[:1], ref[:1])
    else:
        _assert_4x_fallback(tag, ["p", "buf"], kern, fall, ref)


def _run_adam(d, steps, cfg, seed, state_random=False, guard=None):
    p0 = _r(d, seed=seed)
    if state_random:
        m0 = _r(d, seed=seed + 1) * 0.1
        v0 = _r(d, seed=seed + 2).square() * 0.1
        x0 = torch.maximum(v0, _r(d, seed=seed + 3).square() * 0.1)
    else:
        m0, v0, x0 = torch.zeros(d), torch.zeros(d), torch.zeros(d)
    init = (p0, m0, v0, x0)
    fall = [t.clone() for t in init]
    kern = [t.to(DEV) for t in init]
    ref = [t.double() for t in init]
    ams = cfg["amsgrad"]
    for t in steps:
        g = _r(d, seed=seed + 10 + t)
        fb.fused_adam_step(fall[0], g, fall[1], fall[2], fall[3] if ams else None,
                           step=t, **cfg)
        ops.fused_adam_step(kern[0], g.to(DEV), kern[1], kern[2], kern[3] if ams else None,
                            step=t, guard=guard, **cfg)
        ref = list(_adam_ref64(ref[0], g.double(), ref[1], ref[2], ref[3], step=t, **cfg))
    return init, kern, fall, ref


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_instances_and_state(amsgrad, wd):
    cfg = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, amsgrad=amsgrad)
    init, kern, fall, ref = _run_adam(4096 + 64, (1, 2, 3), cfg, seed=300)
    tag = f"adam ams={amsgrad} wd={wd}"
    if amsgrad:
        _assert_4x_fallback(tag, ["p", "m", "v", "vmax"], kern, fall, ref)
    else:  # k_adam<false>: max_exp_avg_sq is never touched
        assert torch.equal(kern[3].cpu(), init[3])
        _assert_4x_fallback(tag, ["p", "m", "v"], kern[:3], fall[:3], ref[:3])


@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam_guard(amsgrad):
    cfg = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, amsgrad=amsgrad)
    off = torch.tensor(False, device=DEV)
    init, kern, _, _ = _run_adam(4096 + 64, (4,), cfg, seed=310, state_random=True, guard=off)
    for name, k, t0 in zip(["p", "m", "v", "vmax"], kern, init):
        assert _bits_equal(k, t0), f"guard=False changed {name}"
    on = torch.tensor(True, device=DEV)
    init, kern, fall, ref = _run_adam(4096 + 64, (4,), cfg, seed=310, state_random=True,
                                      guard=on)
    n = 4 if amsgrad else 3
    _assert_4x_fallback(f"adam guard=True ams={amsgrad}", ["p", "m", "v", "vmax"][:n],
                        kern[:n], fall[:n], ref[:n])
    assert not torch.equal(kern[0].cpu(), init[0])


# ============================================================ C3: past the grid cap
@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
def test_sgd_past_grid_cap(momentum, nesterov):
    cfg = dict(lr=0.1, momentum=momentum, dampening=0.1, weight_decay=0.01, nesterov=nesterov)
    p0, buf0, kern, fall, ref = _run_sgd(D_CAP, (False,), cfg, seed=400, buf0_random=True)
    n = 2 if momentum != 0.0 else 1
    _assert_4x_fallback(f"sgd d={D_CAP} mom={momentum} nest={nesterov}", ["p", "buf"][:n],
                        kern[:n], fall[:n], ref[:n])
    assert bool((kern[0].cpu()[CAP_TAIL:] != p0[CAP_TAIL:]).any())
    if n == 2:
        assert bool((kern[1].cpu()[CAP_TAIL:] != buf0[CAP_TAIL:]).any())


@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam_past_grid_cap(amsgrad):
    cfg = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, amsgrad=amsgrad)
    init, kern, fall, ref = _run_adam(D_CAP, (3,), cfg, seed=410, state_random=True)
    n = 4 if amsgrad else 3
    _assert_4x_fallback(f"adam d={D_CAP} ams={amsgrad}", ["p", "m", "v", "vmax"][:n],
                        kern[:n], fall[:n], ref[:n])
    for k, t0 in zip(kern[:3], init[:3]):
        assert bool((k.cpu()[CAP_TAIL:] != t0[CAP_TAIL:]).any())


@pytest.mark.parametrize("mode,cyclic,a,b", [("rev_grad", False, -100.0, 0.0),
                                             ("constant", True, 1.0, -100.0)])
def test_inject_past_grid_cap(mode, cyclic, a, b):
    g0 = _r(D_CAP, seed=420)
    g = g0.to(DEV)
    ops.inject_(g, mode, cyclic)
    ref = a * g0.double() + b
    # one FMA: a single rounding of the exact a*y + b
    _check_bound(f"inject {mode} cyclic={cyclic} d={D_CAP}", g, ref, ref.abs() * U * (1 + 1e-6))
    assert bool((g.cpu()[CAP_TAIL:] != g0[CAP_TAIL:]).all())


def _combine_ref_bound(x, rows, w):
    terms = w.double()[:, None] * x.double()[rows]
    return terms.sum(0), (len(rows) + 1) * U * terms.abs().sum(0)


def test_combine_rows_past_grid_cap():
    x = _r(3, D_CAP, seed=430)
    rows, w = torch.tensor([2, 0]), _r(2, seed=431)
    out = torch.full((D_CAP,), 12345.0, device=DEV)
    ops.combine_rows(x.to(DEV), rows, w, out)
    ref, bound = _combine_ref_bound(x, rows, w)
    _check_bound(f"combine_rows d={D_CAP}", out, ref, bound)
    assert bool((out[CAP_TAIL:] != 12345.0).all())


def test_cyclic_encode_past_grid_cap():
    g = _r(3, D_CAP, seed=440)
    wre, wim = _r(3, seed=441), _r(3, seed=442)
    out = torch.full((2, D_CAP), 12345.0, device=DEV)
    ops.cyclic_encode(g.to(DEV), wre, wim, out)
    for plane, w in enumerate((wre, wim)):
        ref, bound = _combine_ref_bound(g, torch.arange(3), w)
        _check_bound(f"cyclic_encode plane {plane} d={D_CAP}", out[plane], ref, bound)
    assert bool((out[:, CAP_TAIL:] != 12345.0).all())


def test_rows_equal_past_grid_cap():
    x = _u(2, D_CAP, seed=450)
    x[1] = x[0]
    a, b = torch.tensor([0]), torch.tensor([1])
    assert ops.rows_equal(x.to(DEV), a, b, 0.0).cpu().tolist() == [1]
    x[1, D_CAP - 1] = torch.nextafter(x[0, D_CAP - 1], torch.tensor(2.0))
    assert ops.rows_equal(x.to(DEV), a, b, 0.0).cpu().tolist() == [0]
    assert ops.rows_equal(x.to(DEV), a, b, 1e-6).cpu().tolist() == [1]


def _wmean_ref_bound(x, w, seg):
    """float64 reference and (P+1) u sum|w x| bound; NaN outside every segment."""
    P, d = x.shape
    ref = torch.full((d,), float("nan"), dtype=torch.float64)
    bound = torch.zeros(d, dtype=torch.float64)
    for l in range(len(seg) - 1):
        lo, hi = int(seg[l]), int(seg[l + 1])
        if hi > lo:
            terms = w.double()[:, l : l + 1] * x.double()[:, lo:hi]
            ref[lo:hi] = terms.sum(0)
            bound[lo:hi] = (P + 1) * U * terms.abs().sum(0)
    return ref, bound


def _check_wmean(name, x, w, seg):
    d = x.shape[1]
    out = torch.full((d,), 12345.0, device=DEV)
    ops.segment_weighted_mean(x.to(DEV), w.to(DEV), seg, out)
    ref, bound = _wmean_ref_bound(x, w, seg)
    inside = ~torch.isnan(ref)
    _check_bound(name, out.cpu()[inside], ref[inside], bound[inside])
    # outside every segment `out` must survive bit-exactly
    assert bool((out.cpu()[~inside] == 12345.0).all())
    return out


def test_segment_weighted_mean_past_grid_cap():
    d = 524_288 + 300
    x = _r(2, d, seed=460)
    seg = torch.tensor([0, 1000, 524_288 - 7, d], dtype=torch.int64)
    w = _r(2, 3, seed=461)
    out = _check_wmean(f"segment_weighted_mean d={d}", x, w, seg)
    assert bool((out[524_288:] != 12345.0).all())


# ============================================================ C5: linear kernels
D_LIN = 4096 + 64
ROWSETS = {1: [2], 2: [4, 4], 7: [5, 1, 5, 0, 3, 1, 2]}  # non-monotone, repeated


@pytest.fixture(scope="module")
def lin_x():
    return _r(6, D_LIN, seed=500)


@pytest.mark.parametrize("m", [1, 2, 7])
def test_combine_rows_and_slices(lin_x, m):
    rows, w = torch.tensor(ROWSETS[m]), _r(m, seed=501 + m)
    xg = lin_x.to(DEV)
    whole = torch.empty(D_LIN, device=DEV)
    ops.combine_rows(xg, rows, w, whole)
    ref, bound = _combine_ref_bound(lin_x, rows, w)
    _check_bound(f"combine_rows m={m}", whole, ref, bound)
    # bucketed encode claim: a slice is bit-identical to the same columns of the
    # whole-row combine
    for col_off in (0, 64, D_LIN - 64):
        n = min(1024, D_LIN - col_off)
        part = torch.full((n,), 12345.0, device=DEV)
        ops.combine_rows_slice(xg, rows, w, part, col_off)
        assert torch.equal(part, whole[col_off : col_off + n]), (m, col_off)


@pytest.mark.parametrize("m", [1, 2, 7])
def test_mean_rows(lin_x, m):
    rows = torch.tensor(ROWSETS[m])
    out = torch.empty(D_LIN, device=DEV)
    ops.mean_rows(lin_x.to(DEV), rows, out)
    x64 = lin_x.double()[rows]
    _check_bound(f"mean_rows m={m}", out, x64.mean(0), (m + 1) * U * x64.abs().sum(0) / m)


@pytest.mark.parametrize("m", [1, 2, 7])
def test_sum_rows(m):
    x = _r(m, D_LIN, seed=510 + m)
    out = torch.empty(D_LIN, device=DEV)
    ops.sum_rows(x.to(DEV), out)
    _check_bound(f"sum_rows m={m}", out, x.double().sum(0), (m + 1) * U * x.double().abs().sum(0))


@pytest.mark.parametrize("m", [1, 2, 7])
def test_cyclic_encode(m):
    g = _r(m, D_LIN, seed=520 + m)
    wre, wim = _r(m, seed=530 + m), _r(m, seed=540 + m)
    out = torch.empty(2, D_LIN, device=DEV)
    ops.cyclic_encode(g.to(DEV), wre, wim, out)
    for plane, w in enumerate((wre, wim)):
        ref, bound = _combine_ref_bound(g, torch.arange(m), w)
        _check_bound(f"cyclic_encode m={m} plane {plane}", out[plane], ref, bound)


@pytest.mark.parametrize("n", [1, 2, 7])
def test_cyclic_recombine(n):
    r = _r(n, 2, D_LIN, seed=550 + n)
    vre, vim = _r(n, seed=560 + n), _r(n, seed=570 + n)
    out = torch.empty(D_LIN, device=DEV)
    ops.cyclic_recombine(r.to(DEV), vre, vim, out)
    t_re = vre.double()[:, None] * r.double()[:, 0]
    t_im = vim.double()[:, None] * r.double()[:, 1]
    ref = t_re.sum(0) - t_im.sum(0)
    bound = (2 * n + 1) * U * (t_re.abs().sum(0) + t_im.abs().sum(0))  # 2n combined rows
    _check_bound(f"cyclic_recombine n={n}", out, ref, bound)


@pytest.mark.parametrize("d", [4, 36, D_LIN, D_ROW])
def test_cyclic_project(d):
    rows, z = _r(5, d, seed=580), _r(d, seed=581)
    got = ops.cyclic_project(rows.to(DEV), z.to(DEV))
    terms = rows.double() * z.double()[None, :]
    _check_bound(f"cyclic_project d={d}", got, terms.sum(1), (d + 4) * U * terms.abs().sum(1))


# ============================================================ C6: segment kernels
def _check_sqdist(name, x, z, seg):
    got = ops.segment_sqdist(x.to(DEV), z.to(DEV), seg)
    L = len(seg) - 1
    ref = torch.zeros(x.shape[0], L, dtype=torch.float64)
    bound = torch.zeros_like(ref)
    for l in range(L):
        lo, hi = int(seg[l]), int(seg[l + 1])
        if hi > lo:
            sq = (x.double()[:, lo:hi] - z.double()[lo:hi]) ** 2
            ref[:, l] = sq.sum(1)
            bound[:, l] = (hi - lo + 4) * U * sq.sum(1)
    _check_bound(name, got, ref, bound)  # empty segments: bound 0 -> exactly 0


@pytest.mark.parametrize("case", ["edges", "L1-100", "L1-256", "L1-10000"])
def test_segment_sqdist_and_weighted_mean_edges(case):
    if case == "edges":
        d, seg = D_SEG, torch.tensor(SEG, dtype=torch.int64)
    else:
        d = int(case.split("-")[1])
        seg = torch.tensor([0, d], dtype=torch.int64)
    P, L = 3, len(seg) - 1
    x, z = _r(P, d, seed=600), _r(d, seed=601)
    _check_sqdist(f"segment_sqdist {case}", x, z, seg)
    out = _check_wmean(f"segment_weighted_mean {case}", x, _r(P, L, seed=602), seg)
    if case == "edges":
        assert bool((out[:64] == 12345.0).all()) and bool((out[8000:] == 12345.0).all())


@pytest.mark.parametrize("P", [1, 2, 32])
def test_segment_gram_lengths(P):
    """1/3/4/5: the 4-way unroll and its remainder; 255/256/257/513: one chunk, a
    full chunk, a split with a 1-element tail, two full chunks plus one."""
    lengths = [1, 3, 0, 4, 5, 255, 256, 0, 257, 513]
    bounds = np.concatenate([[8], 8 + np.cumsum(lengths)])  # leading gap of 8
    d = int(bounds[-1]) + 24  # trailing gap
    seg = torch.tensor(bounds, dtype=torch.int64)
    x = _r(P, d, seed=610 + P)
    got = ops.segment_gram(x.to(DEV), seg).cpu()
    assert got.shape == (len(lengths), P, P)
    for l, n in enumerate(lengths):
        lo = int(seg[l])
        xs = x.double()[:, lo : lo + n]
        prods = xs[:, None, :] * xs[None, :, :]  # (P, P, n)
        if n == 0:
            assert bool((got[l] == 0).all()), "empty segment must give a zero matrix"
            continue
        _check_bound(f"segment_gram P={P} len={n}", got[l], prods.sum(2),
                     (n + 4) * U * prods.abs().sum(2))


# ============================================================ D: host-side rejections
# Every call below must raise from a host-side check BEFORE any kernel is launched.
def _g(*shape):
    return torch.zeros(*shape, device=DEV)


def _adam(p, g, m, v, x, amsgrad=True):
    ops.fused_adam_step(p, g, m, v, x, step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                        weight_decay=0.0, amsgrad=amsgrad)


def _sgd(p, g, buf, momentum=0.9):
    ops.fused_sgd_step(p, g, buf, lr=0.1, momentum=momentum, dampening=0.0,
                       weight_decay=0.0, nesterov=False, first_step=True)


_I = lambda *v: torch.tensor(v, dtype=torch.int64, device=DEV)  # noqa: E731


def _seg_over_lds():
    """8194 bounds = 8193 segments: the bounds alone take 8194 * 8 = 65 552 B of LDS,
    more than the 65 536 B a block may request (all segments empty but the last)."""
    seg = torch.zeros(8194, dtype=torch.int64, device=DEV)
    seg[-1] = 8
    return seg


REJECTED = {
    # length not a multiple of 4
    "sgd d%4": lambda: _sgd(_g(6), _g(6), _g(6)),
    "adam d%4": lambda: _adam(_g(6), _g(6), _g(6), _g(6), _g(6)),
    "inject d%4": lambda: ops.inject_(_g(6), "rev_grad"),
    "pair_maxdiff d%4": lambda: ops.pair_maxdiff(_g(2, 6), _I(0), _I(1)),
    "row_absmax d%4": lambda: ops.row_absmax(_g(2, 6)),
    "rows_equal d%4": lambda: ops.rows_equal(_g(2, 6), _I(0), _I(1), 0.0),
    "cyclic_project d%4": lambda: ops.cyclic_project(_g(2, 6), _g(6)),
    "cyclic_encode d%4": lambda: ops.cyclic_encode(_g(3, 6), _g(3), _g(3), _g(2, 6)),
    "combine_rows d%4": lambda: ops.combine_rows(_g(3, 6), _I(0, 1), _g(2), _g(6)),
    "combine_rows_slice off%4": lambda: ops.combine_rows_slice(_g(3, 16), _I(0, 1), _g(2), _g(8), 2),
    # argument lengths that disagree
    "sgd grad length": lambda: _sgd(_g(8), _g(4), _g(8)),
    "sgd buf length": lambda: _sgd(_g(8), _g(8), _g(4)),
    "adam grad length": lambda: _adam(_g(8), _g(4), _g(8), _g(8), _g(8)),
    "adam exp_avg length": lambda: _adam(_g(8), _g(8), _g(4), _g(8), _g(8)),
    "adam exp_avg_sq length": lambda: _adam(_g(8), _g(8), _g(8), _g(4), _g(8)),
    "adam max_exp_avg_sq length": lambda: _adam(_g(8), _g(8), _g(8), _g(8), _g(4)),
    "combine_rows w length": lambda: ops.combine_rows(_g(3, 8), _I(0, 1), _g(3), _g(8)),
    "combine_rows_slice w length": lambda: ops.combine_rows_slice(_g(3, 8), _I(0, 1), _g(1), _g(4), 0),
    "combine_rows out too long": lambda: ops.combine_rows(_g(3, 8), _I(0, 1), _g(2), _g(12)),
    "combine_rows_slice out of range": lambda: ops.combine_rows_slice(_g(3, 8), _I(0, 1), _g(2), _g(8), 4),
    "mean_rows out too long": lambda: ops.mean_rows(_g(3, 8), _I(0, 1), _g(12)),
    "sum_rows out too long": lambda: ops.sum_rows(_g(3, 8), _g(12)),
    "cyclic_recombine v length": lambda: ops.cyclic_recombine(_g(3, 2, 8), _g(2), _g(3), _g(8)),
    "cyclic_encode w_re length": lambda: ops.cyclic_encode(_g(3, 8), _g(2), _g(3), _g(2, 8)),
    "cyclic_encode w_im length": lambda: ops.cyclic_encode(_g(3, 8), _g(3), _g(4), _g(2, 8)),
    "cyclic_encode grads too short": lambda: ops.cyclic_encode(_g(3, 8), _g(3), _g(3), _g(2, 12)),
    "cyclic_encode out planes": lambda: ops.cyclic_encode(_g(3, 8), _g(3), _g(3), _g(3, 8)),
    "cyclic_project z length": lambda: ops.cyclic_project(_g(2, 8), _g(4)),
    "pair_maxdiff index lengths": lambda: ops.pair_maxdiff(_g(2, 8), _I(0, 1), _I(1)),
    "rows_equal index lengths": lambda: ops.rows_equal(_g(2, 8), _I(0, 1), _I(1), 0.0),
    "segment_pair_maxdiff index lengths": lambda: ops.segment_pair_maxdiff(
        _g(2, 8), _I(0, 1), _I(1), _I(0, 8)),
    "segment_sqdist z length": lambda: ops.segment_sqdist(_g(2, 8), _g(4), _I(0, 8)),
    "segment_weighted_mean w shape": lambda: ops.segment_weighted_mean(
        _g(2, 8), _g(2, 2), _I(0, 8), _g(8)),
    "segment_weighted_mean out too short": lambda: ops.segment_weighted_mean(
        _g(2, 8), _g(2, 1), _I(0, 8), _g(4)),
    # CHECK_IN: contiguity, and device for tensors the python wrapper does not move
    "rows_equal x non-contiguous": lambda: ops.rows_equal(_g(2, 16)[:, ::2], _I(0), _I(1), 0.0),
    "row_absmax x non-contiguous": lambda: ops.row_absmax(_g(8, 2).t()),
    "combine_rows x non-contiguous": lambda: ops.combine_rows(_g(3, 16)[:, ::2], _I(0, 1), _g(2), _g(8)),
    "combine_rows w non-contiguous": lambda: ops.combine_rows(_g(3, 8), _I(0, 1), _g(4)[::2], _g(8)),
    "combine_rows rows non-contiguous": lambda: ops.combine_rows(
        _g(3, 8), _I(0, 1, 2, 0)[::2], _g(2), _g(8)),
    "cyclic_encode w_re non-contiguous": lambda: ops.cyclic_encode(
        _g(3, 8), _g(6)[::2], _g(3), _g(2, 8)),
    "cyclic_encode w_im non-contiguous": lambda: ops.cyclic_encode(
        _g(3, 8), _g(3), _g(6)[::2], _g(2, 8)),
    "cyclic_encode w_re on host": lambda: require_extension().cyclic_encode(
        _g(3, 8), torch.zeros(3), _g(3), _g(2, 8)),
    "combine_rows w on host": lambda: require_extension().combine_rows(
        _g(3, 8), _I(0, 1), torch.zeros(2), _g(8)),
    "combine_rows rows on host": lambda: require_extension().combine_rows(
        _g(3, 8), torch.tensor([0, 1]), _g(2), _g(8)),
    # limits and dtypes
    "segment_gram P=33": lambda: ops.segment_gram(_g(33, 8), _I(0, 8)),
    "rows_equal int32 index": lambda: ops.rows_equal(_g(2, 8), _I(0).int(), _I(1).int(), 0.0),
    "combine_rows int32 index": lambda: ops.combine_rows(_g(3, 8), _I(0, 1).int(), _g(2), _g(8)),
    "inject unknown mode": lambda: require_extension().inject(_g(8), "bogus", False),
    # segment bounds that do not fit the LDS of a block, and malformed x / seg
    "segment_absmax seg over LDS": lambda: ops.segment_absmax(_g(2, 8), _seg_over_lds()),
    "segment_pair_maxdiff seg over LDS": lambda: ops.segment_pair_maxdiff(
        _g(2, 8), _I(0), _I(1), _seg_over_lds()),
    "segment_sqdist seg over LDS": lambda: ops.segment_sqdist(_g(2, 8), _g(8), _seg_over_lds()),
    "segment_weighted_mean seg over LDS": lambda: ops.segment_weighted_mean(
        _g(2, 8), _g(2, 8193), _seg_over_lds(), _g(8)),
    "segment_mean_around seg over LDS": lambda: ops.segment_mean_around(
        _g(2, 8), torch.zeros(8193, 1, dtype=torch.int64, device=DEV), _seg_over_lds(), 1, 0, 1,
        _g(8)),
    "segment_absmax x 1D": lambda: ops.segment_absmax(_g(8), _I(0, 8)),
    "segment_sqdist seg 2D": lambda: ops.segment_sqdist(_g(2, 8), _g(8), _I(0, 8).reshape(1, 2)),
}


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_host_side_rejection(name):
    with pytest.raises(RuntimeError):
        REJECTED[name]()
