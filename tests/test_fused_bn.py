"""The fused-norm switch of the ResNets on CPU: off by default, and on CPU (where the
gate of ops.fused_bn_act never opens) bit-identical to the plain
relu(bn(conv(x)) [+ skip]) composition, with unchanged parameters and state_dict."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from draco_amd.models import build_model, enable_fused_norm
from draco_amd.models.resnet import BasicBlock, ResNet18


def _plain_forward(model, x):
    """ResNet-18 written out with torch ops only, from the model's own submodules."""
    out = F.relu(model.stem[1](model.stem[0](x)))
    for stage in model.stages:
        for blk in stage:
            assert isinstance(blk, BasicBlock)
            h = F.relu(blk.body1[1](blk.body1[0](out)))
            h = blk.body2[1](blk.body2[0](h))
            if isinstance(blk.skip, nn.Identity):
                skip = out
            else:
                skip = blk.skip[1](blk.skip[0](out))
            out = F.relu(h + skip)
    out = F.adaptive_avg_pool2d(out, 1).flatten(1)
    return model.fc(out)


def _run(model, x, y, forward):
    model.zero_grad(set_to_none=True)
    logits = forward(model, x)
    F.cross_entropy(logits, y).backward()
    return logits.detach(), [p.grad.clone() for p in model.parameters()]


def _reference():
    torch.manual_seed(0)
    base = ResNet18()
    x = torch.randn(4, 3, 32, 32)
    y = torch.tensor([1, 3, 5, 7])
    ref = copy.deepcopy(base).train()
    logits, grads = _run(ref, x, y, _plain_forward)
    return base, x, y, ref, logits, grads


def test_switch_defaults_off():
    model = build_model("ResNet18", "Cifar10")
    assert not any(getattr(m, "fused_norm", False) for m in model.modules())
    enable_fused_norm(model)
    flagged = [m for m in model.modules() if hasattr(m, "fused_norm")]
    assert len(flagged) == 9 and all(m.fused_norm for m in flagged)  # 8 blocks + the net
    enable_fused_norm(model, False)
    assert not any(m.fused_norm for m in flagged)
    # models without ResNet blocks: a no-op
    enable_fused_norm(build_model("LeNet", "MNIST"))


def test_cpu_forward_backward_equal_plain_composition():
    base, x, y, ref, ref_logits, ref_grads = _reference()
    for on in (False, True):
        model = copy.deepcopy(base).train()
        enable_fused_norm(model, on)
        logits, grads = _run(model, x, y, lambda m, inp: m(inp))
        assert torch.equal(logits, ref_logits), f"logits differ with switch {on}"
        assert len(grads) == len(ref_grads)
        for (name, _), g, r in zip(model.named_parameters(), grads, ref_grads):
            assert torch.equal(g, r), f"grad of {name} differs with switch {on}"
        for (name, b), (_, rb) in zip(model.named_buffers(), ref.named_buffers()):
            assert torch.equal(b, rb), f"buffer {name} differs with switch {on}"


def test_switch_keeps_parameters_and_state_dict():
    torch.manual_seed(0)
    for net in ("ResNet18", "ResNet50"):
        model = build_model(net, "Cifar10")
        keys = list(model.state_dict().keys())
        names = [n for n, _ in model.named_parameters()]
        ids = [id(p) for p in model.parameters()]
        enable_fused_norm(model)
        assert list(model.state_dict().keys()) == keys
        assert [n for n, _ in model.named_parameters()] == names
        assert [id(p) for p in model.parameters()] == ids


def test_bottleneck_cpu_equal():
    """Bottleneck and the ImageNet stem take the same wrapper: same bits on CPU."""
    torch.manual_seed(1)
    base = build_model("ResNet50", "Cifar10").train()
    x = torch.randn(2, 3, 32, 32)
    on = enable_fused_norm(copy.deepcopy(base))
    assert torch.equal(on(x), base(x))


def test_eval_mode_ignores_switch():
    torch.manual_seed(2)
    base = ResNet18()
    x = torch.randn(4, 3, 32, 32)
    base.train()
    base(x)  # move the running stats off their initial values
    base.eval()
    on = enable_fused_norm(copy.deepcopy(base))
    before = {k: v.clone() for k, v in on.state_dict().items()}
    with torch.no_grad():
        assert torch.equal(on(x), base(x))
        assert torch.equal(on(x), _plain_forward(base, x))
    for k, v in on.state_dict().items():
        assert torch.equal(v, before[k]), f"eval forward changed {k}"
