"""CIFAR ResNet-18/34/50/101/152 (capability parity with
/root/reference/src/model_ops/resnet.py:14-113 — itself vendored kuangliu/pytorch-cifar
boilerplate) plus an ImageNet-geometry ResNet-50 for the 224x224 synthetic config
(BASELINE config 5).

Written fresh in idiomatic PyTorch; runs on PyTorch-ROCm (MIOpen/hipBLASLt kernels).
The architecture spec (block structure, stage widths, stride schedule, projection
shortcut rule) is the public ResNet design and is the capability being reproduced.
"""
import torch.nn as nn
import torch.nn.functional as F

from ..ops import fused_bn_act


def _conv_bn(width_in: int, width_out: int, k: int, stride: int = 1) -> nn.Sequential:
    return nn.Sequential(
        nn.Conv2d(width_in, width_out, k, stride=stride, padding=k // 2, bias=False),
        nn.BatchNorm2d(width_out),
    )


def _skip_path(width_in: int, width_out: int, stride: int) -> nn.Module:
    """Identity when shapes line up, else the standard 1x1 projection."""
    if stride == 1 and width_in == width_out:
        return nn.Identity()
    return _conv_bn(width_in, width_out, 1, stride)


def _conv_bn_act(seq: nn.Sequential, x, residual=None, relu=True):
    """A _conv_bn pair with the BatchNorm, the residual add and the ReLU as one op."""
    return fused_bn_act(seq[0](x), seq[1], residual, relu)


def enable_fused_norm(model: nn.Module, on: bool = True) -> nn.Module:
    """Route the BatchNorm(+add)+ReLU of every ResNet block and stem of `model` through
    ops.fused_bn_act (native kernels for bf16 channels_last training on GPU, the plain
    torch expression otherwise).  Off by default; parameters, buffers and state_dict
    keys are the same either way."""
    for m in model.modules():
        if isinstance(m, (BasicBlock, Bottleneck, ResNet)):
            m.fused_norm = bool(on)
    return model


class BasicBlock(nn.Module):
    expansion = 1
    fused_norm = False

    def __init__(self, width_in: int, width: int, stride: int = 1):
        super().__init__()
        self.body1 = _conv_bn(width_in, width, 3, stride)
        self.body2 = _conv_bn(width, width, 3)
        self.skip = _skip_path(width_in, width * self.expansion, stride)

    def _skip_fused(self, x):
        if isinstance(self.skip, nn.Identity):
            return x
        return _conv_bn_act(self.skip, x, relu=False)

    def forward(self, x):
        if self.fused_norm:
            out = _conv_bn_act(self.body1, x)
            return _conv_bn_act(self.body2, out, residual=self._skip_fused(x))
        out = self.body2(F.relu(self.body1(x)))
        return F.relu(out + self.skip(x))


class Bottleneck(nn.Module):
    expansion = 4
    fused_norm = False

    def __init__(self, width_in: int, width: int, stride: int = 1):
        super().__init__()
        self.body1 = _conv_bn(width_in, width, 1)
        self.body2 = _conv_bn(width, width, 3, stride)
        self.body3 = _conv_bn(width, width * self.expansion, 1)
        self.skip = _skip_path(width_in, width * self.expansion, stride)

    _skip_fused = BasicBlock._skip_fused

    def forward(self, x):
        if self.fused_norm:
            out = _conv_bn_act(self.body1, x)
            out = _conv_bn_act(self.body2, out)
            return _conv_bn_act(self.body3, out, residual=self._skip_fused(x))
        out = F.relu(self.body1(x))
        out = F.relu(self.body2(out))
        out = self.body3(out)
        return F.relu(out + self.skip(x))


_STAGE_WIDTHS = (64, 128, 256, 512)


def _stages(block, depths):
    """The four ResNet stages as (width, depth, stride) with stride 1 first."""
    return [(w, d, 1 if i == 0 else 2)
            for i, (w, d) in enumerate(zip(_STAGE_WIDTHS, depths))]


class ResNet(nn.Module):
    """CIFAR geometry: 3x3 stem, 4 stages at 32x32 input."""

    fused_norm = False

    def __init__(self, block, depths, num_classes=10, in_channels=3):
        super().__init__()
        self.stem = _conv_bn(in_channels, 64, 3)
        width_in = 64
        stages = []
        for width, depth, stride in _stages(block, depths):
            blocks = []
            for s in [stride] + [1] * (depth - 1):
                blocks.append(block(width_in, width, s))
                width_in = width * block.expansion
            stages.append(nn.Sequential(*blocks))
        self.stages = nn.Sequential(*stages)
        self.fc = nn.Linear(width_in, num_classes)

    def _stem(self, x):
        if self.fused_norm:
            return _conv_bn_act(self.stem, x)
        return F.relu(self.stem(x))

    def forward(self, x):
        out = self._stem(x)
        out = self.stages(out)
        out = F.adaptive_avg_pool2d(out, 1).flatten(1)
        return self.fc(out)


class ResNetImageNet(ResNet):
    """ImageNet geometry (7x7 stride-2 stem + maxpool) for 224x224 synthetic runs."""

    def __init__(self, block, depths, num_classes=1000, in_channels=3):
        super().__init__(block, depths, num_classes, in_channels)
        self.stem = _conv_bn(in_channels, 64, 7, stride=2)
        self.pool = nn.MaxPool2d(3, stride=2, padding=1)

    def forward(self, x):
        out = self.pool(self._stem(x))
        out = self.stages(out)
        out = F.adaptive_avg_pool2d(out, 1).flatten(1)
        return self.fc(out)


def ResNet18(num_classes=10, in_channels=3):
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes, in_channels)


def ResNet34(num_classes=10, in_channels=3):
    return ResNet(BasicBlock, [3, 4, 6, 3], num_classes, in_channels)


def ResNet50(num_classes=10, in_channels=3):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, in_channels)


def ResNet101(num_classes=10, in_channels=3):
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes, in_channels)


def ResNet152(num_classes=10, in_channels=3):
    return ResNet(Bottleneck, [3, 8, 36, 3], num_classes, in_channels)


def ResNet50ImageNet(num_classes=1000, in_channels=3):
    return ResNetImageNet(Bottleneck, [3, 4, 6, 3], num_classes, in_channels)
