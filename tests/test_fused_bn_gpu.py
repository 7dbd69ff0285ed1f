"""Fused BatchNorm(+residual)+ReLU HIP kernels against a float64 reference and against
the torch bf16 op sequence they replace, on the smallest shapes at which the indexing
can still go wrong; determinism, the fallback gate, hipGraph capture and the trainer."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
MOMENTUM = 0.1
CL = torch.channels_last

# (N, C, H, W)
SHAPES = [
    (2, 8, 1, 1),        # M=2, one vector of channels
    (3, 512, 1, 1),      # M=3, fewer rows than one block iteration covers
    (5, 24, 7, 7),       # M=245, C neither a power of two nor a multiple of 64
    (2, 64, 4, 4),       # small but aligned
    (5, 64, 13, 1),      # M=65 = 2*32+1: the row tail, three row chunks
    (4, 64, 9, 9),       # M=324: eleven row chunks, the last one short
    (5, 512, 29, 113),   # M=16385: several rows per thread, second load batch partly full
]
VARIANTS = ["relu", "res_relu", "plain"]  # BN+ReLU, BN+residual+ReLU, BN alone
BF16_OUT = ("y", "dx", "dres")
FP32_OUT = ("dgamma", "dbeta", "save_mean", "save_invstd", "running_mean", "running_var")


def _ext():
    from draco_amd.ops.native import require_extension

    return require_extension()


def _bn_module(C, gamma, beta, rm0, rv0):
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    return bn.train()


@functools.lru_cache(maxsize=None)
def _case(shape, variant):
    """Inputs, float64 reference, torch bf16 path and fused path for one case, computed
    once and shared (read-only) by the tests below."""
    from draco_amd.ops import fused_bn_act

    N, C, H, W = shape
    relu = variant != "plain"
    has_res = variant == "res_relu"
    gen = torch.Generator().manual_seed(1000 * SHAPES.index(shape) + VARIANTS.index(variant))

    def rnd(*s):
        return torch.randn(*s, generator=gen)

    # channel-dependent mean of up to ~30 with unit spread: a careless variance shows
    offs = torch.linspace(-30.0, 30.0, C)[torch.randperm(C, generator=gen)]
    x = (rnd(N, C, H, W) + offs.view(1, C, 1, 1)).to(DEV, torch.bfloat16).contiguous(memory_format=CL)
    res = rnd(N, C, H, W).to(DEV, torch.bfloat16).contiguous(memory_format=CL) if has_res else None
    dy = rnd(N, C, H, W).to(DEV, torch.bfloat16).contiguous(memory_format=CL)
    gamma, beta = rnd(C).to(DEV), rnd(C).to(DEV)
    rm0, rv0 = rnd(C).to(DEV), (torch.rand(C, generator=gen) + 0.5).to(DEV)
    M = N * H * W

    # --- float64 reference: the same maths from the same bf16 values, torch autograd
    x64 = x.double().requires_grad_()
    g64 = gamma.double().requires_grad_()
    b64 = beta.double().requires_grad_()
    r64 = res.double().requires_grad_() if has_res else None
    mean = x64.mean(dim=(0, 2, 3))
    var = x64.var(dim=(0, 2, 3), unbiased=False)
    invstd = (var + EPS).rsqrt()
    out = (x64 - mean.view(1, C, 1, 1)) * (invstd * g64).view(1, C, 1, 1) + b64.view(1, C, 1, 1)
    if has_res:
        out = out + r64
    if relu:
        out = F.relu(out)
    wrt = [x64, g64, b64] + ([r64] if has_res else [])
    grads = torch.autograd.grad(out, wrt, dy.double())
    ref = dict(
        y=out.detach(), dx=grads[0], dgamma=grads[1], dbeta=grads[2],
        dres=grads[3] if has_res else None,
        save_mean=mean.detach(), save_invstd=invstd.detach(),
        running_mean=(1 - MOMENTUM) * rm0.double() + MOMENTUM * mean.detach(),
        running_var=(1 - MOMENTUM) * rv0.double() + MOMENTUM * var.detach() * M / (M - 1),
    )

    # --- the parent's bf16 op sequence and its autograd
    def run(fn):
        bn = _bn_module(C, gamma, beta, rm0, rv0)
        xi = x.clone().requires_grad_()
        ri = res.clone().requires_grad_() if has_res else None
        yo = fn(xi, bn, ri)
        yo.backward(dy)
        return dict(
            y=yo.detach(), dx=xi.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad,
            dres=ri.grad if has_res else None,
            running_mean=bn.running_mean.detach(), running_var=bn.running_var.detach(),
            nbt=int(bn.num_batches_tracked.item()),
        )

    def torch_path(xi, bn, ri):
        o = F.batch_norm(xi, bn.running_mean, bn.running_var, bn.weight, bn.bias, True,
                         MOMENTUM, EPS)
        bn.num_batches_tracked += 1
        if ri is not None:
            o = o + ri
        return F.relu(o) if relu else o

    tor = run(torch_path)
    fused = [run(lambda xi, bn, ri: fused_bn_act(xi, bn, ri, relu)) for _ in range(2)]

    # the saved statistics are not visible through autograd: take them from the op
    ext = _ext()
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    y2, sm, si = ext.bn_act_forward(x, res if has_res else x.new_empty(0), gamma, beta, rm, rv,
                                    nbt, MOMENTUM, EPS, relu)
    for f in fused:
        f["save_mean"], f["save_invstd"] = sm, si
    direct = dict(y=y2, running_mean=rm, running_var=rv, nbt=int(nbt.item()))
    torch.cuda.synchronize()
    return dict(ref=ref, torch=tor, fused=fused, direct=direct, has_res=has_res)


def _err(a, ref):
    return float((a.double() - ref).abs().max())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy_vs_float64(shape, variant):
    """Per output: fused max-abs error vs float64 <= max(torch path's error vs the same
    reference, one bf16 ulp (2^-8) of max|ref|); 1e-5 of max|ref| for fp32 outputs."""
    c = _case(shape, variant)
    ref, tor, fused = c["ref"], c["torch"], c["fused"][0]
    failures = []
    for name in BF16_OUT + FP32_OUT:
        if ref[name] is None:
            continue
        floor = (2.0 ** -8 if name in BF16_OUT else 1e-5) * float(ref[name].abs().max())
        e_fused = _err(fused[name], ref[name])
        e_torch = _err(tor[name], ref[name]) if name in tor else 0.0
        bound = max(e_torch, floor)
        print(f"[fused_bn {shape} {variant}] {name:13} fused={e_fused:.3e} "
              f"torch={e_torch:.3e} floor={floor:.3e}")
        if not e_fused <= bound:
            failures.append((name, e_fused, bound))
    assert not failures, failures
    assert fused["nbt"] == 1 and tor["nbt"] == 1
    assert c["direct"]["nbt"] == 1


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_two_calls_bitwise_equal(shape, variant):
    c = _case(shape, variant)
    a, b = c["fused"]
    for name in ("y", "dx", "dres", "dgamma", "dbeta", "running_mean", "running_var"):
        if a[name] is None:
            continue
        assert torch.equal(a[name], b[name]), name
    # the op called directly computes what the autograd wrapper computes
    for name in ("y", "running_mean", "running_var"):
        assert torch.equal(c["direct"][name], a[name]), name


def test_shapes_cover_the_kernel_paths():
    """The shape table is tied to the launch geometry, so a retuned tile cannot quietly
    stop the cases from covering the tail, the cross-block and the multi-row paths."""
    ext = _ext()

    def geom(shape):
        N, C, H, W = shape
        rpc, chunks, ctiles, rows_per_iter = ext.bn_act_geometry(N * H * W, C)
        return N * H * W, rpc, chunks, ctiles, rows_per_iter

    M, rpc, chunks, ctiles, it = geom(SHAPES[1])
    assert M < it and ctiles > 1
    M, rpc, chunks, ctiles, it = geom(SHAPES[4])
    assert M % it == 1 and chunks > 1
    M, rpc, chunks, ctiles, it = geom(SHAPES[5])
    assert chunks > 1 and M % rpc not in (0, 1)
    M, rpc, chunks, ctiles, it = geom(SHAPES[6])
    assert rpc > 4 * it and chunks > 16 and ctiles > 1  # > one load batch, > finalize lanes
    # the grid depends on (M, C) alone
    assert ext.bn_act_geometry(131072, 64) == ext.bn_act_geometry(131072, 64)


def _composition(x, bn, residual, relu):
    out = bn(x)
    if residual is not None:
        out = out + residual
    return F.relu(out) if relu else out


@pytest.mark.parametrize("what", ["fp32", "nchw", "eval", "c4", "no_running_stats"])
def test_gate_failures_take_the_torch_path_bitwise(what):
    from draco_amd.ops import fused_bn_act

    torch.manual_seed(3)
    C = 4 if what == "c4" else 16
    dtype = torch.float32 if what == "fp32" else torch.bfloat16
    x = (torch.randn(4, C, 6, 6, device=DEV) * 2 + 1).to(dtype)
    res = torch.randn(4, C, 6, 6, device=DEV).to(dtype)
    if what != "nchw":
        x, res = x.contiguous(memory_format=CL), res.contiguous(memory_format=CL)
    dy = torch.randn_like(x)
    bn = nn.BatchNorm2d(C, track_running_stats=what != "no_running_stats").to(DEV)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    bn.train(what != "eval")
    results = []
    for fn in (fused_bn_act, _composition):
        m = copy.deepcopy(bn)
        xi, ri = x.clone().requires_grad_(), res.clone().requires_grad_()
        y = fn(xi, m, ri, True)
        assert type(y.grad_fn).__name__ != "_FusedBNActBackward"
        y.backward(dy)
        results.append([y.detach(), xi.grad, ri.grad, m.weight.grad, m.bias.grad]
                       + [b.clone() for b in m.buffers()])
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_native_path_is_taken_inside_the_gate():
    from draco_amd.ops import fused_bn_act

    x = torch.randn(2, 16, 3, 3, device=DEV).to(torch.bfloat16).contiguous(memory_format=CL)
    bn = nn.BatchNorm2d(16).to(DEV).train()
    y = fused_bn_act(x.requires_grad_(), bn)
    assert type(y.grad_fn).__name__ == "_FusedBNActBackward"
    assert y.is_contiguous(memory_format=CL) and y.dtype == torch.bfloat16


def test_bad_arguments_raise_host_side():
    """The launchers reject what the kernels cannot index, before any launch."""
    ext = _ext()

    def args(N=2, C=16, H=3, W=3, dtype=torch.bfloat16, cl=True):
        x = torch.randn(N, C, H, W, device=DEV).to(dtype)
        if cl:
            x = x.contiguous(memory_format=CL)
        f = lambda: torch.ones(C, device=DEV)
        return [x, x.new_empty(0), f(), f(), f(), f(),
                torch.zeros((), dtype=torch.int64, device=DEV), 0.1, 1e-5, True]

    ext.bn_act_forward(*args())  # the well-formed call passes
    bad = {
        "fp32 input": args(dtype=torch.float32),
        "NCHW input": args(cl=False),
        "C % 8 != 0": args(C=12),
        "M < 2": args(N=1, H=1, W=1),
    }
    a = args()
    a[1] = torch.zeros(2, 16, 3, 2, device=DEV, dtype=torch.bfloat16).contiguous(memory_format=CL)
    bad["residual shape"] = a
    a = args()
    a[2] = torch.ones(8, device=DEV)
    bad["gamma length"] = a
    a = args()
    a[4] = torch.ones(16, device=DEV, dtype=torch.float64)
    bad["running_mean dtype"] = a
    a = args()
    a[6] = torch.zeros((), dtype=torch.int32, device=DEV)
    bad["counter dtype"] = a
    for why, arg in bad.items():
        with pytest.raises(RuntimeError):
            ext.bn_act_forward(*arg)
            pytest.fail(f"accepted: {why}")

    x = args()[0]
    v = torch.ones(16, device=DEV)
    ext.bn_act_backward(x, x, x, v, v, v, True, True)
    for why, arg in {
        "dy shape": (x[:1].contiguous(memory_format=CL), x, x, v, v, v, True, False),
        "dy dtype": (x.float(), x, x, v, v, v, True, False),
        "y NCHW": (x, x, x.contiguous(), v, v, v, True, False),
        "save_mean length": (x, x, x, v, v[:8].contiguous(), v, False, False),
    }.items():
        with pytest.raises(RuntimeError):
            ext.bn_act_backward(*arg)
            pytest.fail(f"accepted: {why}")
    torch.cuda.synchronize()


def test_graph_capture_matches_eager_bitwise():
    """Forward+backward of one BasicBlock captured in a hipGraph (side-stream warm-up as
    the trainer does), replayed three times with fresh inputs: every replay equals an
    eager call on the same inputs bit for bit, and the counters advance once per replay."""
    from draco_amd.models import enable_fused_norm
    from draco_amd.models.resnet import BasicBlock

    torch.manual_seed(11)
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        block = enable_fused_norm(BasicBlock(64, 64)).to(DEV).to(memory_format=CL).train()
        # bf16 like a block's input inside the network (the stem's output under autocast)
        static_x = torch.randn(2, 64, 8, 8, device=DEV).to(torch.bfloat16).contiguous(
            memory_format=CL).requires_grad_()
        static_dy = torch.randn(2, 64, 8, 8, device=DEV).to(torch.bfloat16).contiguous(memory_format=CL)
        for p in block.parameters():
            p.grad = torch.zeros_like(p)
        static_x.grad = torch.zeros_like(static_x)

        def body(blk, x, dy):
            for p in blk.parameters():
                p.grad.zero_()
            x.grad.zero_()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = blk(x)
            assert type(out.grad_fn).__name__ == "_FusedBNActBackward"
            out.backward(dy)
            return out.detach()

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                body(block, static_x, static_dy)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = body(block, static_x, static_dy)
        torch.cuda.synchronize()

        eager = copy.deepcopy(block)  # same parameters, same running stats
        for p in eager.parameters():
            p.grad = torch.zeros_like(p)
        nbt0 = [int(m.num_batches_tracked) for m in block.modules() if isinstance(m, nn.BatchNorm2d)]
        assert len(nbt0) == 2
        for i in range(3):
            x = torch.randn(2, 64, 8, 8, device=DEV) * (i + 1) + i
            dy = torch.randn(2, 64, 8, 8, device=DEV)
            with torch.no_grad():
                static_x.copy_(x)
                static_dy.copy_(dy)
            graph.replay()
            ex = static_x.detach().clone().requires_grad_()
            ex.grad = torch.zeros_like(ex)
            e_out = body(eager, ex, static_dy.clone())
            torch.cuda.synchronize()
            assert torch.equal(static_out, e_out), f"replay {i}: output"
            assert torch.equal(static_x.grad, ex.grad), f"replay {i}: input grad"
            for (name, p), q in zip(block.named_parameters(), eager.parameters()):
                assert torch.equal(p.grad, q.grad), f"replay {i}: grad of {name}"
            for (name, b), c in zip(block.named_buffers(), eager.buffers()):
                assert torch.equal(b, c), f"replay {i}: buffer {name}"
        nbt1 = [int(m.num_batches_tracked) for m in block.modules() if isinstance(m, nn.BatchNorm2d)]
        assert [b - a for a, b in zip(nbt0, nbt1)] == [3, 3]


def test_trainer_with_fused_norm(tmp_path, monkeypatch):
    """The flagship configuration at test size with the fused path on: trains, no update
    skipped, no degenerate vote, and honest replicas agree within half the vote
    tolerance (the measurement of test_train_gpu.test_vote_tolerance_margin)."""
    from draco_amd.config import Config
    from draco_amd.parallel.trainer import Trainer

    def cfg(sub, **kw):
        base = dict(
            network="ResNet18", dataset="Cifar10", batch_size=32, device="cuda", lr=0.05,
            dtype="bf16", max_steps=60, eval_freq=0, log_dir="",
            train_dir=str(tmp_path / sub), approach="maj_vote", mode="maj_vote",
            group_size=3, fused_norm=True,
        )
        base.update(kw)
        return Config(**base)

    t = Trainer(cfg("a", worker_fail=1, err_mode="rev_grad"))
    t.logger.stdout_every = 0
    assert t.model.fused_norm and all(
        m.fused_norm for m in t.model.modules() if hasattr(m, "fused_norm"))
    losses = [t.train_step()["loss"] for _ in range(8)]
    torch.cuda.synchronize()
    assert np.isfinite(losses).all(), losses
    assert t.skipped_updates == 0
    assert t.agg.degenerate_steps == 0
    nbt = {int(m.num_batches_tracked) for m in t.model.modules() if isinstance(m, nn.BatchNorm2d)}
    assert min(nbt) >= 8, nbt  # the counters are maintained by the fused kernels
    t.close()

    from draco_amd.ops import fused_bn

    gate, taken = fused_bn._native_gate, []

    def recording_gate(*a):
        taken.append(gate(*a))
        return taken[-1]

    monkeypatch.setattr(fused_bn, "_native_gate", recording_gate)
    t = Trainer(cfg("b", worker_fail=0))
    t.logger.stdout_every = 0
    x, y = t.data.batch_for(0, 0)
    g1 = t.space.alloc_payload(1)[0]
    g2 = t.space.alloc_payload(1)[0]
    t._forward_backward(x, y, g1)
    assert len(taken) == 20 and all(taken), taken  # every BatchNorm of ResNet-18, natively
    t._forward_backward(x, y, g1)
    noise = 0.0
    for _ in range(5):
        t._forward_backward(x, y, g2)
        torch.cuda.synchronize()
        noise = max(noise, (g1 - g2).abs().max().item())
    scale = g1.abs().max().item()
    rtol = t.vote_rtol
    assert rtol > 0.0
    print(f"[fused vote margin] noise/scale={noise / scale:.3e} rtol={rtol}")
    assert noise <= 0.5 * rtol * scale, f"replica noise {noise:.3e} vs thresh {rtol * scale:.3e}"
    t.close()
