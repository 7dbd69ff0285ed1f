"""The gradient sink on the MI355X: k_scatter_grads against its definition
(fallback.scatter_grads_) bit for bit, the freshness of the bf16 parameter shadow, and
the flagship path (bf16, NHWC, hipGraphs, maj_vote r=3) with the sink on and off.

Layout facts the shapes are chosen for (ops/csrc/draco_kernels.hip, k_scatter_grads): a
block takes one 4096-element chunk of one range, 64 ranges per launch (gaps and the pad
tail are ranges too); the head up to the destination's first 16-byte boundary and the
tail are scalar, the body is 16-byte loads (4 fp32 / 8 bf16) when the source is 16-byte
aligned there and element loads otherwise.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from draco_amd import ops
    from draco_amd.ops import fallback
    from draco_amd.ops.native import available

    assert available(), "HIP extension must be built and importable on the GPU box"

DEV = "cuda:0"
CL = torch.channels_last
LENGTHS = (1, 3, 10, 1728, 4099)  # one lane; below a float4; head+body+tail; a conv; two chunks


def _bits(t):
    return t.view(torch.int32)


def _special(t):
    """NaN, +-Inf, -0.0 and (bf16) subnormals into the first elements of t, in place."""
    vals = [float("nan"), float("inf"), float("-inf"), -0.0, 9.2e-41, -9.2e-41]  # bf16 subnormal
    for k, v in enumerate(vals[: t.numel()]):
        t[k] = v
    return t


def _case():
    """70 sources: every length x every destination alignment (0, 4, 8, 12 bytes mod 16)
    x both dtypes, a slice whose pointer is 2-byte aligned, an fp32 slice that is 4-byte
    aligned, channels-last 4-D tensors, one NCHW 4-D tensor (the copy route), filler; a
    37-element gap in the middle and a 64-element pad tail."""
    gen = torch.Generator().manual_seed(7)
    srcs, offsets, pos = [], [], 0

    def place(t, align=None, gap=0):
        nonlocal pos
        pos += gap
        if align is not None:
            pos += (align - pos) % 4
        srcs.append(t)
        offsets.append(pos)
        pos += t.numel()

    for dtype in (torch.float32, torch.bfloat16):
        for n in LENGTHS:
            for align in range(4):
                t = torch.randn(n, generator=gen).to(dtype)
                place((_special(t) if n >= 10 else t).to(DEV), align)  # set on the host
    base16 = torch.randn(4200, generator=gen).bfloat16().to(DEV)
    place(base16[1:4100], 0, gap=37)              # pointer 2-byte aligned, destination aligned
    assert base16[1:4100].data_ptr() % 4 == 2
    base32 = torch.randn(1100, generator=gen).to(DEV)
    place(base32[1:1001], 3)                       # pointer 4-byte aligned
    for dtype in (torch.float32, torch.bfloat16):
        for shape in ((8, 4, 3, 3), (8, 4, 1, 1)):
            t = torch.randn(shape, generator=gen).to(dtype).to(DEV).contiguous(memory_format=CL)
            place(t)
    nchw = torch.randn(8, 4, 3, 3, generator=gen).to(DEV)
    assert nchw.is_contiguous() and not nchw.is_contiguous(memory_format=CL)
    place(nchw)
    while len(srcs) < 70:
        n = int(torch.randint(1, 40, (1,), generator=gen))
        place(torch.randn(n, generator=gen).to(torch.bfloat16 if n % 2 else torch.float32).to(DEV))
    d_pad = (pos + 63) // 64 * 64 + 64
    return srcs, offsets, d_pad, nchw


def test_kernel_matches_fallback_bitwise(monkeypatch):
    srcs, offsets, d_pad, nchw = _case()
    assert len(srcs) == 70
    assert {o % 4 for o in offsets} == {0, 1, 2, 3}
    ref = torch.full((d_pad,), float("nan"), device=DEV)
    fallback.scatter_grads_(srcs, offsets, ref, channels_last=True)

    calls = []
    ext = ops.require_extension()

    class Spy:
        @staticmethod
        def scatter_grads(dense, dense_off, skip_off, skip_len, out):
            calls.append((len(dense), list(skip_off), list(skip_len)))
            ext.scatter_grads(dense, dense_off, skip_off, skip_len, out)

    monkeypatch.setattr(ops, "_native_for", lambda t: Spy)
    out = torch.full((d_pad,), float("nan"), device=DEV)  # NaN: an unwritten element shows
    ops.scatter_grads_(srcs, offsets, out, channels_last=True)
    torch.cuda.synchronize()
    # the NCHW tensor, and only it, went through the strided copy
    assert calls == [(69, [offsets[[s is nchw for s in srcs].index(True)]], [nchw.numel()])]
    assert torch.equal(_bits(out), _bits(ref))
    # what the definition says, independent of the fallback: specials kept, gaps +0.0
    covered = torch.zeros(d_pad, dtype=torch.bool, device=DEV)
    for s, o in zip(srcs, offsets):
        covered[o : o + s.numel()] = True
        want = fallback.flat_order(s, True).float()
        assert torch.equal(_bits(out[o : o + s.numel()]), _bits(want))
    assert int((~covered).sum()) >= 37 + 64
    assert torch.equal(_bits(out[~covered]), torch.zeros(int((~covered).sum()), dtype=torch.int32,
                                                        device=DEV))
    assert bool(torch.isnan(out).any()) and bool(torch.isinf(out).any())  # the specials are there

    # an empty list zeroes the row
    ops.scatter_grads_([], [], out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), torch.zeros(d_pad, dtype=torch.int32, device=DEV))


def test_kernel_row_major_space():
    """channels_last=False: a channels-last 4-D source is the one that takes the copy."""
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(8, 4, 3, 3, generator=gen).to(DEV).contiguous(memory_format=CL)
    b = torch.randn(8, 4, 3, 3, generator=gen).bfloat16().to(DEV)
    c = torch.randn(6, 5, generator=gen).to(DEV).t()
    srcs, offsets = [a, b, c], [2, 300, 601]
    out = torch.full((704,), float("nan"), device=DEV)
    ref = torch.full((704,), float("nan"), device=DEV)
    ops.scatter_grads_(srcs, offsets, out)
    fallback.scatter_grads_(srcs, offsets, ref)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(ref))
    assert torch.equal(out[2:290], a.reshape(-1))


def test_rejections_on_device():
    out = torch.zeros(64, device=DEV)
    a = torch.ones(8, device=DEV)
    with pytest.raises(ValueError, match="overlaps"):
        ops.scatter_grads_([a, a], [0, 4], out)
    with pytest.raises(ValueError, match="beyond"):
        ops.scatter_grads_([a], [60], out)
    with pytest.raises(ValueError, match="fp32 or bf16"):
        ops.scatter_grads_([a.half()], [0], out)
    with pytest.raises(ValueError, match="device"):
        ops.scatter_grads_([a.cpu()], [0], out)
    ext = ops.require_extension()
    with pytest.raises(RuntimeError, match="overlaps"):
        ext.scatter_grads([a, a], [0, 4], [], [], out)
    with pytest.raises(RuntimeError, match="beyond"):
        ext.scatter_grads([a], [60], [], [], out)
    with pytest.raises(RuntimeError, match="overlaps"):
        ext.scatter_grads([a], [0], [4], [8], out)
    with pytest.raises(RuntimeError, match="fp32 or bf16"):
        ext.scatter_grads([a.half()], [0], [], [], out)
    with pytest.raises(RuntimeError, match="device"):
        ext.scatter_grads([a.cpu()], [0], [], [], out)
    with pytest.raises(RuntimeError, match="aligned"):
        ext.scatter_grads([a], [0], [], [], torch.zeros(65, device=DEV)[1:])
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros(64, device=DEV))


def _flagship(tmp_path, sub, **kw):
    from draco_amd.config import Config
    from draco_amd.parallel.trainer import Trainer

    base = dict(network="ResNet18", dataset="Cifar10", batch_size=8, device="cuda", dtype="bf16",
                channels_last=True, hip_graphs=True, approach="maj_vote", mode="maj_vote",
                group_size=3, worker_fail=1, err_mode="rev_grad", lr=0.05, max_steps=20,
                eval_freq=0, log_dir="", train_dir=str(tmp_path / sub))
    base.update(kw)
    t = Trainer(Config(**base))
    t.logger.stdout_every = 0
    return t


def test_shadow_follows_in_place_writes(tmp_path):
    """flat_param written in place between steps (a checkpoint load, a benchmark's rewind):
    the next step's replicas read the new values.  lr = 0 keeps flat_param where the write
    put it, so after the step the shadow is flat_param.bfloat16() bit for bit."""
    t = _flagship(tmp_path, "shadow", lr=0.0, worker_fail=0)
    space = t.space
    assert t.use_sink and space.shadow is not None and space.shadow.dtype == torch.bfloat16
    assert len(space.shadow_leaves) == 22  # 20 conv weights + the fc weight and bias
    t.train_step()  # capture
    other = torch.randn_like(space.flat_param) * 0.05
    space.flat_param.copy_(other)
    t.train_step()  # replay
    torch.cuda.synchronize()
    assert torch.equal(space.flat_param, other)
    assert torch.equal(space.shadow.view(torch.int16), space.flat_param.bfloat16().view(torch.int16))
    i, leaf = next(iter(space.shadow_leaves.items()))
    assert leaf.stride() == space.params[i].stride() and leaf.shape == space.params[i].shape
    t.close()


@pytest.mark.parametrize("sink", [True, False])
def test_flagship_path_small(tmp_path, sink):
    """Capture plus 3 replayed steps; with grad_sink=False the plain route stays alive.

    Not stable at this batch size, with the sink on and off alike (KNOWN_ISSUES 17 and
    11): of 10 fresh trainers of this configuration on the MI355X, 5 (2 of 5 with
    grad_sink=False, 3 of 5 with True) had one gradient element of 7.3e6 .. 7.1e31,
    the same in all three replicas, in the first replayed step, and NaN rows, a
    degenerate vote and a skipped update from the next step on; the other 5 were clean.
    This test with the sink on failed in 3 of 3 runs of this file alone and passed, as
    did the sink-off case, in a whole-suite run."""
    t = _flagship(tmp_path, f"flag_{sink}", grad_sink=sink)
    assert t.use_graphs and t.use_cl and t.use_sink == sink
    d = t.space.d
    assert t.space.d_pad > d  # there is a pad tail to look at
    losses = []
    for _ in range(4):
        losses.append(t.train_step()["loss"])
        torch.cuda.synchronize()
        assert torch.isfinite(t.payload).all()
        assert bool((t.payload[:, d:] == 0).all())  # the adversary's row holds -0.0 there
        assert float(t.payload.abs().max()) > 0.0
    assert np.isfinite(losses).all(), losses
    assert len(t._graphs) == 3
    assert t.agg.degenerate_steps == 0
    assert t.skipped_updates == 0
    if sink:
        assert all(p.grad is None for p in t.model.parameters())
    t.close()
