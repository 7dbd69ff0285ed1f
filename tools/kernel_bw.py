"""Achieved-bandwidth microbench for every draco HIP kernel at bench-realistic
shapes.  All of these are HBM-bound streaming kernels (RESULTS.md design note), so
GB/s vs the ~8 TB/s HBM3E peak is the speed-of-light scorecard.

  gpurun -- 'python tools/kernel_bw.py > gpurun_out/kernel_bw.txt 2>&1'
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from draco_amd import ops

DEV = "cuda:0"


def t_ms(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def report(name, ms, bytes_moved):
    print(f"{name:34} {ms*1e3:9.1f} us  {bytes_moved/ms/1e6:8.1f} GB/s")


def main():
    d = 11_173_952  # ResNet-18 flat space (d_pad at world=1)
    d = (d + 63) // 64 * 64
    rows = 24  # r=3 x world=8 recv rows
    x = torch.randn(rows, d, device=DEV)
    out = torch.empty(d, device=DEV)
    shard_out = torch.empty(d, device=DEV)
    z = torch.randn(d, device=DEV)
    seg = torch.linspace(0, d, 63, dtype=torch.int64).to(DEV)
    pa = torch.arange(0, 12, device=DEV, dtype=torch.int64)
    pb = torch.arange(12, 24, device=DEV, dtype=torch.int64)

    B = 4 * rows * d  # fp32 bytes in the full payload

    ms = t_ms(lambda: ops.row_absmax(x))
    report("row_absmax (24 x 11.2M)", ms, B)
    ms = t_ms(lambda: ops.pair_maxdiff(x, pa, pb))
    report("pair_maxdiff (12 pairs)", ms, B)
    ms = t_ms(lambda: ops.segment_absmax(x, seg))
    report("segment_absmax (62 segs)", ms, B)
    ms = t_ms(lambda: ops.segment_pair_maxdiff(x, pa, pb, seg))
    report("segment_pair_maxdiff", ms, B)
    ms = t_ms(lambda: ops.cyclic_project(x, z))
    report("cyclic_project (24 rows)", ms, B + 4 * d)
    ms = t_ms(lambda: ops.mean_rows(x, pa, out))
    report("mean_rows (12 rows)", ms, 4 * 12 * d + 4 * d)
    ms = t_ms(lambda: ops.sum_rows(x, out))
    report("sum_rows (24 rows)", ms, B + 4 * d)
    w = torch.randn(rows, device=DEV)
    ms = t_ms(lambda: ops.combine_rows(x, torch.arange(rows, device=DEV), w, out))
    report("combine_rows (24 rows)", ms, B + 4 * d)
    g5 = torch.randn(5, d, device=DEV)
    wre, wim = torch.randn(5, device=DEV), torch.randn(5, device=DEV)
    enc = torch.empty(2, d, device=DEV)
    ms = t_ms(lambda: ops.cyclic_encode(g5, wre, wim, enc))
    report("cyclic_encode (5 rows->2)", ms, 4 * 5 * d + 8 * d)
    p = torch.randn(d, device=DEV)
    gr = torch.randn(d, device=DEV)
    buf = torch.zeros(d, device=DEV)
    ms = t_ms(lambda: ops.fused_sgd_step(p, gr, buf, lr=0.01, momentum=0.9, dampening=0.0,
                                         weight_decay=0.0, nesterov=False, first_step=False))
    report("fused_sgd (momentum)", ms, 4 * d * 4)  # r p,g,buf + w p,buf ~ 4-5 streams
    m1 = torch.zeros(d, device=DEV)
    v1 = torch.zeros(d, device=DEV)
    ms = t_ms(lambda: ops.fused_adam_step(p, gr, m1, v1, None, step=5, lr=1e-3, beta1=0.9,
                                          beta2=0.999, eps=1e-8, weight_decay=0.0,
                                          amsgrad=False))
    report("fused_adam", ms, 4 * d * 7)
    ms = t_ms(lambda: ops.inject_(gr, "rev_grad"))
    report("inject rev_grad", ms, 4 * d * 2)
    part = t_ms(lambda: ops.segment_sqdist(x, z, seg))
    report("segment_sqdist (geomed)", part, B + 4 * d)
    wt = torch.rand(rows, 62, device=DEV)
    wt = wt / wt.sum(0, keepdim=True)
    ms = t_ms(lambda: ops.segment_weighted_mean(x, wt, seg, out))
    report("segment_weighted_mean", ms, B + 4 * d)
    ms = t_ms(lambda: ops.segment_gram(x, seg))
    report("segment_gram (krum)", ms, B)
    ms = t_ms(lambda: ops.column_trimmed_mean(x, 11, 13, out))
    report("column_trimmed_mean (median)", ms, B + 4 * d)
    ms = t_ms(lambda: ops.column_trimmed_mean(x, 1, 23, out))
    report("column_trimmed_mean (b=1)", ms, B + 4 * d)
    ms = t_ms(lambda: ops.column_mean_around(x, 23, 11, 13, out))
    report("column_mean_around (meamed b=1)", ms, B + 4 * d)
    ms = t_ms(lambda: ops.column_mean_around(x, 23, 1, 23, out))
    report("column_mean_around (phocas b=1)", ms, B + 4 * d)


def mean_around_compare(rounds=3):
    """column_mean_around (mean around median / Phocas) on the same shape as its
    yardsticks: combine_rows (same bytes read and written: the streaming ceiling),
    column_trimmed_mean (the same load + register sort without the window step) and
    the torch route to the same result (fallback.column_mean_around on GPU tensors:
    sort, compare, gather).  The arms alternate inside each round; min-max over the
    rounds is printed per arm."""
    from draco_amd.ops import fallback as fb
    d = 11_173_952
    d = (d + 63) // 64 * 64
    rows = 24
    x = torch.randn(rows, d, device=DEV)
    out = torch.empty(d, device=DEV)
    ref = torch.empty(d, device=DEV)
    B = 4 * rows * d + 4 * d
    idx = torch.arange(rows, device=DEV)
    w = torch.randn(rows, device=DEV)
    arms = [
        ("combine_rows (24 rows)", lambda: ops.combine_rows(x, idx, w, out), {}),
        ("column_trimmed_mean (b=1)", lambda: ops.column_trimmed_mean(x, 1, 23, out), {}),
        ("column_mean_around (meamed b=1)", lambda: ops.column_mean_around(x, 23, 11, 13, out), {}),
        ("column_mean_around (meamed b=5)", lambda: ops.column_mean_around(x, 19, 11, 13, out), {}),
        ("column_mean_around (phocas b=1)", lambda: ops.column_mean_around(x, 23, 1, 23, out), {}),
        ("torch route (meamed b=1)", lambda: fb.column_mean_around(x, 23, 11, 13, ref),
         dict(iters=3, warmup=1)),
    ]
    # same result first (sign of zero aside): a faster kernel that computes something
    # else is not a comparison
    for keep, clo, chi in ((23, 11, 13), (19, 11, 13), (23, 1, 23)):
        ops.column_mean_around(x, keep, clo, chi, out)
        fb.column_mean_around(x, keep, clo, chi, ref)
        torch.cuda.synchronize()
        assert bool((out == ref).all()), (keep, clo, chi)
    times = {name: [] for name, _, _ in arms}
    for r in range(rounds):
        print(f"# round {r}")
        for name, fn, kw in arms:
            ms = t_ms(fn, **kw)
            times[name].append(ms)
            report(name, ms, B)
    print("# min - max over rounds")
    for name, _, _ in arms:
        lo, hi = min(times[name]), max(times[name])
        print(f"{name:34} {lo*1e3:9.1f} - {hi*1e3:9.1f} us")


def bulyan_compare(rounds=3, d=11_173_952):
    """segment_mean_around (Multi-Krum / Bulyan decode: T selected rows per segment,
    gathered through the index table) at two Bulyan shapes, against its yardsticks at
    the same bytes: column_mean_around on a contiguous (T, d) tensor (the same sort and
    window arithmetic without gather or segment search), combine_rows with T rows (the
    streaming ceiling) and the torch route to the same result (per segment:
    index_select, then one column_mean_around launch).  Results are asserted equal
    first; the arms alternate inside each round; min-max over the rounds per arm."""
    d = (d + 63) // 64 * 64
    nseg = 62
    seg_host = [int(v) // 64 * 64 for v in torch.linspace(0, d, nseg + 1).tolist()]
    seg_host[-1] = d
    seg = torch.tensor(seg_host, dtype=torch.int64, device=DEV)
    out = torch.empty(d, device=DEV)
    ref = torch.empty(d, device=DEV)
    gen = torch.Generator().manual_seed(0)
    times, order = {}, []
    shapes = []
    for P, f in ((24, 1), (23, 5)):
        T = P - 2 * f
        keep, clo, chi = T - 2 * f, (T - 1) // 2, T // 2 + 1
        x = torch.randn(P, d, device=DEV)
        xc = x[:T].contiguous()
        sel = torch.stack([torch.randperm(P, generator=gen)[:T] for _ in range(nseg)]).to(DEV)
        idx = torch.arange(T, device=DEV)
        w = torch.randn(T, device=DEV)

        def torch_route(x=x, sel=sel, keep=keep, clo=clo, chi=chi):
            for l in range(nseg):
                lo, hi = seg_host[l], seg_host[l + 1]
                ops.column_mean_around(torch.index_select(x[:, lo:hi], 0, sel[l]), keep, clo,
                                       chi, ref[lo:hi])

        # same result first: a faster kernel that computes something else is no comparison
        ops.segment_mean_around(x, sel, seg, keep, clo, chi, out)
        torch_route()
        torch.cuda.synchronize()
        assert bool((out == ref).all()), (P, f, "gather kernel != torch route")
        ops.segment_mean_around(x, idx.repeat(nseg, 1), seg, keep, clo, chi, out)
        ops.column_mean_around(xc, keep, clo, chi, ref)
        torch.cuda.synchronize()
        assert bool((out == ref).all()), (P, f, "identity selection != contiguous kernel")
        tag = f"P={P} f={f} T={T} keep={keep}"
        B = 4 * T * d + 4 * d
        shapes.append((tag, B, [
            (f"segment_mean_around ({tag})",
             lambda x=x, sel=sel, k=(keep, clo, chi): ops.segment_mean_around(x, sel, seg, *k, out),
             {}),
            (f"column_mean_around contiguous (T={T})",
             lambda xc=xc, k=(keep, clo, chi): ops.column_mean_around(xc, *k, out), {}),
            (f"combine_rows ({T} rows)",
             lambda xc=xc, idx=idx, w=w: ops.combine_rows(xc, idx, w, out), {}),
            (f"torch route: 62 x index_select+cma (T={T})", torch_route, dict(iters=5, warmup=2)),
        ]))
    for r in range(rounds):
        print(f"# round {r}")
        for tag, B, arms in shapes:
            for name, fn, kw in arms:
                ms = t_ms(fn, **kw)
                if name not in times:
                    times[name] = []
                    order.append(name)
                times[name].append(ms)
                report(name, ms, B)
    print("# min - max over rounds")
    for name in order:
        lo, hi = min(times[name]), max(times[name])
        print(f"{name:46} {lo*1e3:9.1f} - {hi*1e3:9.1f} us")


def trimmed_mean_compare():
    """column_trimmed_mean vs its two yardsticks on the same shape: the torch route to
    the same result (sort along dim 0, slice, mean) and combine_rows, which reads the
    same bytes and writes the same output (the streaming ceiling for this access
    pattern)."""
    d = 11_173_952
    d = (d + 63) // 64 * 64
    rows = 24
    x = torch.randn(rows, d, device=DEV)
    out = torch.empty(d, device=DEV)
    B = 4 * rows * d + 4 * d
    idx = torch.arange(rows, device=DEV)
    w = torch.randn(rows, device=DEV)
    ms = t_ms(lambda: ops.combine_rows(x, idx, w, out))
    report("combine_rows (24 rows)", ms, B)
    for name, lo, hi in (("median", 11, 13), ("b=1", 1, 23)):
        ms = t_ms(lambda: ops.column_trimmed_mean(x, lo, hi, out))
        report(f"column_trimmed_mean ({name})", ms, B)
        ms = t_ms(lambda: torch.mean(torch.sort(x, dim=0).values[lo:hi], dim=0, out=out),
                  iters=5, warmup=2)
        report(f"torch sort+mean ({name})", ms, B)


def collude_compare(rounds=3):
    """collude_ (colluding ALIE / inner-product adversaries: f rows of the 24 x 11.2M
    block overwritten with a*mu + b*sigma of the others) against its two yardsticks on
    the same shape: combine_rows with 24 rows (the same bytes with one row written) and
    column_trimmed_mean(x, 0, 24) (the same loads plus a register sort).  collude_ reads
    24-f rows and writes f.  The result is checked against the fp64 definition on a
    column sample first; the arms alternate inside each round; min-max over the rounds
    per arm."""
    d = 11_173_952
    d = (d + 63) // 64 * 64
    rows = 24
    x = torch.randn(rows, d, device=DEV)
    out = torch.empty(d, device=DEV)
    idx = torch.arange(rows, device=DEV)
    w = torch.randn(rows, device=DEV)
    arms = [
        ("combine_rows (24 rows)", lambda: ops.combine_rows(x, idx, w, out), 4 * (rows + 1) * d),
        ("column_trimmed_mean (0, 24)", lambda: ops.column_trimmed_mean(x, 0, rows, out),
         4 * (rows + 1) * d),
    ]
    for f in (1, 5):
        byz = list(range(rows - f, rows))
        for name, a, b in (("alie z=1.5", 1.0, -1.5), ("ipm eps=0.1", -0.1, 0.0)):
            # same result first: a fast kernel that computes something else is no comparison
            y = x.clone()
            ops.collude_(y, byz, a, b)
            H = x[: rows - f, :65536].double()
            ref = a * H.mean(0) + b * ((H - H.mean(0)) ** 2).mean(0).sqrt()
            tol = 8 * (abs(a) + abs(b)) * rows * 2.0 ** -24 * H.abs().amax(0)
            for r in byz:
                assert bool(((y[r, :65536].double() - ref).abs() <= tol).all()), (f, name, r)
            assert bool((y[: rows - f] == x[: rows - f]).all()), (f, name)
            del y
            # the timed calls overwrite the last f rows of x again and again: the
            # honest rows, the only ones read, never change
            arms.append((f"collude_ f={f} {name}",
                         lambda byz=byz, a=a, b=b: ops.collude_(x, byz, a, b), 4 * rows * d))
    times = {name: [] for name, _, _ in arms}
    for r in range(rounds):
        print(f"# round {r}")
        for name, fn, nbytes in arms:
            ms = t_ms(fn)
            times[name].append(ms)
            report(name, ms, nbytes)
    print("# min - max over rounds")
    for name, _, _ in arms:
        lo, hi = min(times[name]), max(times[name])
        print(f"{name:34} {lo*1e3:9.1f} - {hi*1e3:9.1f} us")


def centered_clip_compare(rounds=3, iters=3):
    """Centered clipping, `iters` iterations on 24 x 11.2M and 8 x 11.2M: the fused route
    (iters + 1 clip_step_ launches: iters + 1 passes over the block) against the
    existing-ops route on the same data (per iteration segment_sqdist over one segment +
    segment_weighted_mean + one add: 2 * iters passes).  Both routes compute the clip
    factors with the same P-element torch code on device (fixed radius sqrt(d), about
    the distance of a randn row from 0, so rows are clipped and unclipped), and their
    results are compared before timing.  Single clip_step_ passes and collude_ (ipm,
    f=1: the same row passes with one row written) give the per-pass level.  GB/s
    counts the block passes and the v / out traffic of each route; the arms alternate
    inside each round; min-max over the rounds per arm."""
    d = 11_173_952
    d = (d + 63) // 64 * 64
    tau = float(d) ** 0.5
    seg = torch.tensor([0, d], dtype=torch.int64, device=DEV)
    for rows in (24, 8):
        x = torch.randn(rows, d, device=DEV)
        x[rows // 2:] *= 3.0  # the far half is clipped
        v = torch.zeros(d, device=DEV)
        z = torch.zeros(d, device=DEV)
        zero_w = torch.zeros(rows, device=DEV)

        def factors(d2):
            dist = d2.double().sqrt()
            c = torch.where(dist <= tau, torch.ones_like(dist), tau / dist)
            return torch.where(torch.isfinite(dist), c, torch.zeros_like(dist))

        def fused():
            v.zero_()
            d2 = ops.clip_step_(x, v, zero_w)
            for it in range(1, iters + 1):
                d2 = ops.clip_step_(x, v, (factors(d2) / rows).float(), dist=it < iters)

        def composed():
            v.zero_()
            for it in range(iters):
                d2 = ops.segment_sqdist(x, v, seg).reshape(rows)
                w = (factors(d2) / rows).float()
                ops.segment_weighted_mean(x, w.reshape(rows, 1).contiguous(), seg, z)
                torch.addcmul(z, v, 1.0 - w.sum(), out=v)  # v = (1 - sum w) v + sum w_i x_i

        fused()
        got = v.clone()
        composed()
        torch.cuda.synchronize()
        err = float((got - v).abs().max())
        assert err <= 1e-4 * float(v.abs().max()), (rows, err)
        print(f"# {rows} rows: max |fused - composed| = {err:.3e}, max |v| = "
              f"{float(v.abs().max()):.3e}")
        w_fix = torch.full((rows,), 1.0 / rows, device=DEV)
        xc = x.clone()  # collude_ writes its row: not into the block the other arms read
        blk = 4 * rows * d
        arms = [
            (f"fused x{iters} ({rows} rows)", fused,
             (iters + 1) * blk + 4 * d * (1 + 1 + 2 * iters)),
            (f"composed x{iters} ({rows} rows)", composed,
             2 * iters * blk + 4 * d * (1 + iters * (1 + 1 + 3))),
            (f"clip_step_ dist ({rows} rows)", lambda: ops.clip_step_(x, v, w_fix),
             blk + 8 * d),
            (f"clip_step_ no dist ({rows} rows)",
             lambda: ops.clip_step_(x, v, w_fix, dist=False), blk + 8 * d),
            (f"clip_step_ measure ({rows} rows)", lambda: ops.clip_step_(x, v, zero_w),
             blk + 4 * d),
            (f"segment_sqdist ({rows} rows)", lambda: ops.segment_sqdist(x, v, seg),
             blk + 4 * d),
            (f"collude_ f=1 ipm ({rows} rows)",
             lambda: ops.collude_(xc, [rows - 1], -0.1, 0.0), blk),
        ]
        times = {name: [] for name, _, _ in arms}
        for r in range(rounds):
            print(f"# round {r}")
            for name, fn, nbytes in arms:
                ms = t_ms(fn, iters=20, warmup=5)
                times[name].append(ms)
                report(name, ms, nbytes)
        print("# min - max over rounds")
        for name, _, _ in arms:
            lo, hi = min(times[name]), max(times[name])
            print(f"{name:34} {lo*1e3:9.1f} - {hi*1e3:9.1f} us")
        del x, xc, v, z


def worker_momentum_compare(rounds=3, beta=0.9):
    """worker_momentum_ (worker-side momentum: m = beta*m + (1-beta)*g, g = m, one launch
    over one 11.2M-element payload row and its state row, 16 B per element) against the
    torch route to the same result without the non-finite rule (mul_ + add_, then
    copy_: three launches, 28 B per element), and against two kernels of the same
    streaming shape as yardsticks: inject rev_grad (k_axpb, 8 B per element) and
    fused_sgd with momentum (20 B per element).  The first-step instance reads g and
    writes m (8 B per element).  Results are compared against the fp64 definition
    first; the arms alternate inside each round; min-max over the rounds per arm."""
    d = 11_173_952
    d = (d + 63) // 64 * 64
    omb = 1.0 - beta
    g0 = torch.randn(d, device=DEV)
    m0 = torch.randn(d, device=DEV)
    g0[::1001] = float("nan")
    g, m = g0.clone(), m0.clone()
    ops.worker_momentum_(g, m, beta, False)
    fin = torch.isfinite(g0)
    exact = beta * m0.double() + omb * g0.double()
    tol = 4 * 2.0 ** -24 * ((beta * m0.double()).abs() + (omb * g0.double()).abs())
    assert bool(((m.double() - exact).abs()[fin] <= tol[fin]).all())
    assert bool((m[~fin] == m0[~fin]).all()) and bool(torch.isnan(g[~fin]).all())
    assert bool((g[fin] == m[fin]).all())
    # timed calls feed g = m back in: the values stay finite and settle
    g, m = torch.randn(d, device=DEV), torch.randn(d, device=DEV)
    tg, tm = g.clone(), m.clone()
    p, buf = torch.randn(d, device=DEV), torch.zeros(d, device=DEV)
    gs = torch.randn(d, device=DEV) * 1e-3

    def torch_route():
        tm.mul_(beta).add_(tg, alpha=omb)
        tg.copy_(tm)

    arms = [
        ("worker_momentum_", lambda: ops.worker_momentum_(g, m, beta, False), 16 * d),
        ("worker_momentum_ first", lambda: ops.worker_momentum_(g, m, beta, True), 8 * d),
        ("torch mul_+add_, copy_", torch_route, 28 * d),
        ("inject rev_grad (8 B/el)", lambda: ops.inject_(gs, "rev_grad"), 8 * d),
        ("fused_sgd momentum (20 B/el)",
         lambda: ops.fused_sgd_step(p, gs, buf, lr=0.0, momentum=0.5, dampening=0.0,
                                    weight_decay=0.0, nesterov=False, first_step=False), 20 * d),
    ]
    times = {name: [] for name, _, _ in arms}
    for r in range(rounds):
        print(f"# round {r}")
        for name, fn, nbytes in arms:
            ms = t_ms(fn, iters=200, warmup=20)
            times[name].append(ms)
            report(name, ms, nbytes)
    print("# min - max over rounds")
    for name, _, _ in arms:
        lo, hi = min(times[name]), max(times[name])
        print(f"{name:34} {lo*1e3:9.1f} - {hi*1e3:9.1f} us")


def gram_compare():
    """Hand-written k_seg_gram vs the rocBLAS route (62 torch.mm per-segment GEMMs
    — the brief's 'plain library GEMMs belong on MFMA' case)."""
    from draco_amd.ops import fallback as fb
    d = 11_173_952
    d = (d + 63) // 64 * 64
    rows = 24
    x = torch.randn(rows, d, device=DEV)
    seg = torch.linspace(0, d, 63, dtype=torch.int64).to(DEV)
    B = 4 * rows * d
    ms = t_ms(lambda: ops.segment_gram(x, seg), iters=10, warmup=3)
    report("segment_gram HIP kernel", ms, B)
    ms = t_ms(lambda: fb.segment_gram(x, seg), iters=10, warmup=3)
    report("segment_gram rocBLAS (62 mm)", ms, B)


def t_graph_ms(fn, reps=10, iters=20):
    """Per-call time of `fn` replayed from a hipGraph holding `reps` calls: device time
    without the Python and autograd launch overhead, which for a 10 us kernel is most of
    what t_ms would see (and is not there in the trainer, which replays graphs)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            keep = fn()  # noqa: F841 - outputs live until the capture ends
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (iters * reps) * 1e3


def fused_bn_compare(rounds=3):
    """Fused BatchNorm(+residual)+ReLU forward and backward against the torch bf16 op
    sequence they replace (F.batch_norm, add, relu and its autograd), at the four
    ResNet-18 stage shapes of the flagship (128 images, bf16 NHWC), with and without a
    residual.  Each arm (forward, and forward+backward) is timed as hipGraph replays
    (t_graph_ms); the arms alternate inside each round; min-max over the rounds per arm.
    GB/s is the MINIMUM traffic over the time: forward 2 reads of x (+1 of the residual)
    + 1 write; backward dy, y, x read twice + dx written (with a residual the fused
    kernels write and re-read dz instead of re-reading dy and y: the same bytes)."""
    import torch.nn as nn
    import torch.nn.functional as F

    from draco_amd.ops import fused_bn_act

    cl = torch.channels_last
    shapes = [(128, 64, 32, 32), (128, 128, 16, 16), (128, 256, 8, 8), (128, 512, 4, 4)]
    arms, times, numel = [], {}, {}
    for N, C, H, W in shapes:
        for has_res in (False, True):
            x = (torch.randn(N, C, H, W, device=DEV) + 3).to(torch.bfloat16).contiguous(memory_format=cl)
            res = torch.randn_like(x) if has_res else None
            dy = torch.randn_like(x)
            bn = nn.BatchNorm2d(C).to(DEV).train()
            nb = x.numel() * 2
            fwd_bytes = nb * (4 if has_res else 3)
            bwd_bytes = nb * 7

            def torch_fwd(xi, bn=bn, res=res):
                o = bn(xi)
                if res is not None:
                    o = o + res
                return F.relu(o)

            def fused_fwd(xi, bn=bn, res=res):
                return fused_bn_act(xi, bn, res, True)

            tag = f"{C}x{H}x{W}{' +res' if has_res else ''}"
            numel[tag] = x.numel()
            for kind, fwd in (("torch", torch_fwd), ("fused", fused_fwd)):
                xi = x.clone().requires_grad_()
                ri = res.clone().requires_grad_() if has_res else None
                f = (lambda fwd=fwd, xi=xi, ri=ri: fwd(xi, res=ri)) if has_res else \
                    (lambda fwd=fwd, xi=xi: fwd(xi))
                wrt = [xi, bn.weight, bn.bias] + ([ri] if has_res else [])
                # forward and backward are captured TOGETHER: autograd runs a node's
                # backward on the stream its forward ran on, so a backward whose
                # forward happened outside the capture would launch outside it too
                fb = lambda f=f, wrt=wrt, dy=dy: torch.autograd.grad(f(), wrt, dy)
                arms.append((f"{kind} fwd {tag}", f, fwd_bytes))
                arms.append((f"{kind} fwd+bwd {tag}", fb, fwd_bytes + bwd_bytes))
    for r in range(rounds):
        print(f"# round {r}")
        for name, fn, nbytes in arms:
            ms = t_graph_ms(fn)
            times.setdefault(name, []).append(ms)
            report(name, ms, nbytes)
    print("# min - max over rounds (us), GB/s at the min")
    for (name, _, nbytes) in arms:
        lo, hi = min(times[name]), max(times[name])
        print(f"{name:34} {lo*1e3:9.1f} - {hi*1e3:9.1f} us  {nbytes/lo/1e6:8.1f} GB/s")
    print("# backward alone = (fwd+bwd) - fwd at the min, against its 7 tensor passes")
    for (name, _, _) in arms:
        if " fwd+bwd " in name:
            us = (min(times[name]) - min(times[name.replace(" fwd+bwd ", " fwd ")])) * 1e3
            nbytes = numel[name.split(" fwd+bwd ")[1]] * 2 * 7
            print(f"{name.replace(' fwd+bwd ', ' bwd '):34} {us:9.1f} us  {nbytes/us/1e3:8.1f} GB/s")


if __name__ == "__main__":
    if os.environ.get("FUSED_BN_ONLY") == "1":
        fused_bn_compare()
        raise SystemExit(0)
    if os.environ.get("GRAM_ONLY") == "1":
        gram_compare()
        raise SystemExit(0)
    if os.environ.get("TRIMMED_MEAN_ONLY") == "1":
        trimmed_mean_compare()
        raise SystemExit(0)
    if os.environ.get("MEAN_AROUND_ONLY") == "1":
        mean_around_compare()
        raise SystemExit(0)
    if os.environ.get("COLLUDE_ONLY") == "1":
        collude_compare()
        raise SystemExit(0)
    if os.environ.get("CENTERED_CLIP_ONLY") == "1":
        centered_clip_compare()
        raise SystemExit(0)
    if os.environ.get("WORKER_MOMENTUM_ONLY") == "1":
        worker_momentum_compare()
        raise SystemExit(0)
    if os.environ.get("BULYAN_ONLY") == "1":
        bulyan_compare()
        raise SystemExit(0)
    main()
