"""MobileNetV1 (Howard et al. 2017): a 3x3 stem of 32 and 13 separable
blocks, each a depthwise 3x3 convolution (groups == channels) followed by a
pointwise 1x1, both with BN + ReLU. On the GPU the depthwise convolutions
run on ops/kernels/conv_dw.hip through PsConv2d; all widths are powers of
two, so every other layer stays on the dense hand kernels.

CIFAR layout: stem stride 1, depthwise stride 2 at the blocks that widen to
128, 256, 512 and the first 1024 (32x32 -> 2x2 before the pool). The
ImageNet layout (resnet.py's _imagenet rule) has stem stride 2 as well.
"""
from __future__ import annotations

import torch.nn as nn

from ..ops.conv import PsConv2d
from ..ops.linear import PsLinear
from ..ops.pool import global_avg_pool
from ..ops.modules import PsBatchNorm2d
from .resnet import _imagenet

# (output width, depthwise stride) of the 13 blocks
BLOCKS = [(64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2),
          (512, 1), (512, 1), (512, 1), (512, 1), (512, 1), (1024, 2),
          (1024, 1)]


class SeparableBlock(nn.Module):
    """depthwise 3x3 (stride) -> BN+ReLU -> pointwise 1x1 -> BN+ReLU"""

    def __init__(self, in_planes: int, out_planes: int, stride: int):
        super().__init__()
        self.conv1 = PsConv2d(in_planes, in_planes, 3, stride=stride,
                              padding=1, groups=in_planes, bias=False)
        self.bn1 = PsBatchNorm2d(in_planes, relu=True)
        self.conv2 = PsConv2d(in_planes, out_planes, 1, bias=False)
        self.bn2 = PsBatchNorm2d(out_planes, relu=True)

    def forward(self, x):
        out = self.bn1(self.conv1(x))
        return self.bn2(self.conv2(out))


class MobileNet(nn.Module):
    def __init__(self, num_classes: int = 10, in_channels: int = 3):
        super().__init__()
        self.conv1 = PsConv2d(in_channels, 32, 3,
                              stride=2 if _imagenet(num_classes) else 1,
                              padding=1, bias=False)
        self.bn1 = PsBatchNorm2d(32, relu=True)
        in_planes, blocks = 32, []
        for out_planes, stride in BLOCKS:
            blocks.append(SeparableBlock(in_planes, out_planes, stride))
            in_planes = out_planes
        self.layers = nn.Sequential(*blocks)
        self.linear = PsLinear(in_planes, num_classes)

    def forward(self, x):
        out = self.layers(self.bn1(self.conv1(x)))
        return self.linear(global_avg_pool(out))
