"""ResNeXt (aggregated residual transformations, Xie et al. 2017): the
bottleneck's 3x3 convolution is grouped (cardinality 32), which on the GPU
runs on ops/kernels/conv_group.hip through PsConv2d.

ResNeXt29_32x4d is the CIFAR layout: 3x3 stem of 64, three stages of three
bottlenecks (1x1 -> grouped 3x3 carrying the stride -> 1x1) with group
widths 128/256/512 and block outputs 256/512/1024 (4, 8 and 16 channels
per group), projection shortcuts, global average pool, linear classifier.

ResNeXt50_32x4d is resnet.py's ResNet with a bottleneck of cardinality 32
and base width 4 (widths 128/256/512/1024: 4, 8, 16 and 32 channels per
group) and the same ImageNet stem rule.
"""
from __future__ import annotations

import torch.nn as nn

from ..ops.conv import PsConv2d, conv_with_passthrough
from ..ops.linear import PsLinear
from ..ops.pool import global_avg_pool
from ..ops.modules import PsBatchNorm2d
from .resnet import ResNet, _imagenet


class GroupedBottleneck(nn.Module):
    """1x1 (in -> width), grouped 3x3 (width -> width, stride), 1x1
    (width -> out), each with BN; relu(bn3 + shortcut) fused in bn3."""

    def __init__(self, in_planes: int, width: int, out_planes: int,
                 stride: int, groups: int):
        super().__init__()
        self.conv1 = PsConv2d(in_planes, width, 1, bias=False)
        self.bn1 = PsBatchNorm2d(width, relu=True)
        self.conv2 = PsConv2d(width, width, 3, stride=stride, padding=1,
                              groups=groups, bias=False)
        self.bn2 = PsBatchNorm2d(width, relu=True)
        self.conv3 = PsConv2d(width, out_planes, 1, bias=False)
        self.bn3 = PsBatchNorm2d(out_planes, relu=True)
        self.shortcut = nn.Sequential()
        if stride != 1 or in_planes != out_planes:
            self.shortcut = nn.Sequential(
                PsConv2d(in_planes, out_planes, 1, stride=stride, bias=False),
                PsBatchNorm2d(out_planes),
            )

    def forward(self, x):
        # conv1 passes x through so the shortcut's gradient fuses into its
        # dgrad epilogue (see resnet.py)
        h, x_sc = conv_with_passthrough(self.conv1, x)
        out = self.bn1(h)
        out = self.bn2(self.conv2(out))
        return self.bn3(self.conv3(out), residual=self.shortcut(x_sc))


class ResNeXtBottleneck(GroupedBottleneck):
    """Block signature of resnet.py's ResNet: (in_planes, planes, stride)."""
    expansion = 4
    groups = 32
    base_width = 4

    def __init__(self, in_planes: int, planes: int, stride: int = 1):
        width = planes * self.base_width // 64 * self.groups
        super().__init__(in_planes, width, planes * self.expansion, stride,
                         self.groups)


class ResNeXtCifar(nn.Module):
    def __init__(self, num_blocks: int = 3, cardinality: int = 32,
                 base_width: int = 4, num_classes: int = 10,
                 in_channels: int = 3):
        super().__init__()
        self.conv1 = PsConv2d(in_channels, 64, 3, stride=1, padding=1,
                              bias=False)
        self.bn1 = PsBatchNorm2d(64, relu=True)
        in_planes, layers = 64, []
        for stage, stride in enumerate((1, 2, 2)):
            width = cardinality * base_width << stage
            blocks = []
            for i in range(num_blocks):
                blocks.append(GroupedBottleneck(
                    in_planes, width, 2 * width, stride if i == 0 else 1,
                    cardinality))
                in_planes = 2 * width
            layers.append(nn.Sequential(*blocks))
        self.layer1, self.layer2, self.layer3 = layers
        self.linear = PsLinear(in_planes, num_classes)

    def forward(self, x):
        out = self.bn1(self.conv1(x))
        out = self.layer3(self.layer2(self.layer1(out)))
        return self.linear(global_avg_pool(out))


def ResNeXt29_32x4d(num_classes=10, in_channels=3):
    return ResNeXtCifar(3, 32, 4, num_classes, in_channels)


def ResNeXt50_32x4d(num_classes=10, in_channels=3):
    return ResNet(ResNeXtBottleneck, [3, 4, 6, 3], num_classes, in_channels,
                  _imagenet(num_classes))
