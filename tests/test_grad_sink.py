"""The gradient sink on the CPU: the definition of ops.scatter_grads_ (the fallback, the
oracle of the HIP kernel), its host-side rejections, and the trainer's rows with the sink
on against the rows of the plain route (p.grad views of a zeroed row + backward)."""
import pytest
import torch

from draco_amd import ops
from draco_amd.config import Config
from draco_amd.ops import fallback
from draco_amd.parallel.trainer import Trainer


def _loop_reference(srcs, offsets, d_pad, channels_last):
    """scatter_grads_ written out element by element."""
    out = [0.0] * d_pad
    for s, o in zip(srcs, offsets):
        if channels_last and s.dim() == 4:
            n, c, h, w = s.shape
            k = 0
            for a in range(n):
                for y in range(h):
                    for x in range(w):
                        for b in range(c):
                            out[o + k] = float(s[a, b, y, x])
                            k += 1
        else:
            for k, v in enumerate(s.reshape(-1).tolist()):
                out[o + k] = float(v)
    return torch.tensor(out, dtype=torch.float32)


def test_name_is_public():
    assert "scatter_grads_" in ops.__all__


@pytest.mark.parametrize("channels_last", [False, True])
def test_fallback_matches_loop(channels_last):
    gen = torch.Generator().manual_seed(0)
    srcs = [
        torch.randn(5, generator=gen),
        torch.randn(3, 2, generator=gen).bfloat16(),
        torch.randn(2, 3, 2, 2, generator=gen),                                     # NCHW
        torch.randn(2, 3, 2, 2, generator=gen).bfloat16().contiguous(memory_format=torch.channels_last),
        torch.randn(4, 3, generator=gen).t(),                                       # strided 2-D
    ]
    offsets = [1, 7, 13, 40, 70]  # gaps at 0, 6, 37..39, 64..69 and the tail
    out = torch.full((128,), float("nan"))
    ops.scatter_grads_(srcs, offsets, out, channels_last=channels_last)
    ref = _loop_reference(srcs, offsets, 128, channels_last)
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def test_fallback_special_values_and_empty_list():
    bits = torch.tensor([0x7FC1, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x8040], dtype=torch.int32)
    bf = bits.to(torch.int16).view(torch.bfloat16)
    fp = torch.tensor([float("nan"), float("inf"), -0.0, 1e-45])
    out = torch.full((16,), float("nan"))
    ops.scatter_grads_([bf, fp], [2, 8], out)
    assert torch.equal(out[2:8].view(torch.int32), bits << 16)  # exact widening
    assert torch.equal(out[8:12].view(torch.int32), fp.view(torch.int32))
    rest = torch.cat([out[:2], out[12:]])
    assert torch.equal(rest.view(torch.int32), torch.zeros(6, dtype=torch.int32))  # +0.0
    ops.scatter_grads_([], [], out)
    assert torch.equal(out.view(torch.int32), torch.zeros(16, dtype=torch.int32))


def test_rejections():
    out = torch.zeros(64)
    a, b = torch.ones(8), torch.ones(8)
    with pytest.raises(ValueError, match="overlaps"):
        ops.scatter_grads_([a, b], [0, 4], out)
    with pytest.raises(ValueError, match="overlaps"):
        ops.scatter_grads_([a, b], [10, 3], out)  # order of the list does not matter
    with pytest.raises(ValueError, match="beyond"):
        ops.scatter_grads_([a], [60], out)
    with pytest.raises(ValueError, match="beyond"):
        ops.scatter_grads_([a], [-1], out)
    with pytest.raises(ValueError, match="fp32 or bf16"):
        ops.scatter_grads_([a.half()], [0], out)
    with pytest.raises(ValueError, match="fp32 or bf16"):
        ops.scatter_grads_([a.double()], [0], out)
    with pytest.raises(ValueError, match="offsets"):
        ops.scatter_grads_([a, b], [0], out)
    with pytest.raises(ValueError, match="out must be"):
        ops.scatter_grads_([a], [0], out.double())
    with pytest.raises(ValueError, match="out must be"):
        ops.scatter_grads_([a], [0], torch.zeros(128)[::2])
    with pytest.raises(ValueError, match="device"):
        ops.scatter_grads_([a.to("meta")], [0], out)
    assert torch.equal(out, torch.zeros(64))  # a rejected call writes nothing
    ops.scatter_grads_([a, b], [8, 0], out)   # touching ranges are fine
    assert torch.equal(out[:16], torch.ones(16))


def _trainer(tmp_path, network, dataset, sink):
    cfg = Config(network=network, dataset=dataset, batch_size=4, device="cpu", lr=0.05,
                 approach="maj_vote", mode="maj_vote", group_size=3, worker_fail=0,
                 max_steps=10, eval_freq=0, log_dir="",
                 train_dir=str(tmp_path / f"{network}_{sink}"), grad_sink=sink)
    t = Trainer(cfg)
    t.logger.stdout_every = 0
    return t


@pytest.mark.parametrize("network,dataset", [("LeNet", "MNIST"), ("ResNet18", "Cifar10")])
def test_trainer_rows_bit_for_bit(tmp_path, network, dataset):
    """CPU autograd is reproducible: the sink's payload equals the plain route's bit for
    bit after one step, -0.0 and +0.0 taken as equal (the plain route adds the gradient
    to a zeroed row, and 0 + (-0) = +0); the parameters after 3 steps are equal bit for
    bit."""
    on, off = (_trainer(tmp_path, network, dataset, s) for s in (True, False))
    assert on.use_sink and not off.use_sink
    on.train_step(), off.train_step()
    a, b = on.payload.clone(), off.payload.clone()
    assert torch.isfinite(b).all() and float(b.abs().max()) > 0.0
    assert torch.equal(a, b)  # value equality: NaN-free, and -0.0 == +0.0
    a[a == 0] = 0.0
    b[b == 0] = 0.0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(p.grad is None for p in on.model.parameters())
    assert all(p.grad is not None for p in off.model.parameters())
    for _ in range(2):
        on.train_step(), off.train_step()
    assert torch.equal(on.space.flat_param.view(torch.int32), off.space.flat_param.view(torch.int32))
    on.close(), off.close()


def test_sink_gating(tmp_path):
    """Off under --compile (and on the bucketed path, covered by the gloo tests, which
    run with the default grad_sink=True and keep their hooks)."""
    cfg = Config(network="LeNet", dataset="MNIST", batch_size=4, device="cpu", compile=True,
                 approach="baseline", mode="normal", worker_fail=0, max_steps=2, eval_freq=0,
                 log_dir="", train_dir=str(tmp_path / "c"))
    t = Trainer(cfg)
    assert not t.use_sink and t.space.shadow is None
    t.close()
