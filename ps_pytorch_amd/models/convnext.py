"""ConvNeXt (Liu et al. 2022) in a CIFAR-sized layout. A block is a
depthwise 7x7 convolution, a LayerNorm over the channels of each pixel, a 1x1
expansion to 4C, GELU, a 1x1 projection back to C, then layer scale plus the
residual. On the GPU the depthwise convolution runs on ops/kernels/conv_dw.hip
and the two 1x1 on the dense kernels, all through PsConv2d; LayerNorm, GELU
and the block tail run on ops/kernels/layernorm.hip. No stochastic depth.

Layout for 32x32 inputs: a 3x3 stride-1 stem to dims[0] followed by a
LayerNorm (the ImageNet 4x4 stride-4 patchify stem would leave 8x8); between
stages a LayerNorm, then a 2x2 stride-2 convolution (32 -> 16 -> 8 -> 4);
head: global average pool, LayerNorm, linear.
"""
from __future__ import annotations

import torch.nn as nn

from ..ops.conv import PsConv2d
from ..ops.linear import PsLinear
from ..ops.pool import global_avg_pool
from ..ops.modules import PsGELU, PsLayerNorm2d, PsLayerScaleAdd


class ConvNeXtBlock(nn.Module):
    """dw 7x7 -> LN -> 1x1 (4C) -> GELU -> 1x1 (C) -> x + lambda * y"""

    def __init__(self, dim: int, layer_scale_init: float = 1e-6):
        super().__init__()
        self.dwconv = PsConv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = PsLayerNorm2d(dim)
        self.pwconv1 = PsConv2d(dim, 4 * dim, 1)
        self.act = PsGELU()
        self.pwconv2 = PsConv2d(4 * dim, dim, 1)
        self.scale = PsLayerScaleAdd(dim, init=layer_scale_init)

    def forward(self, x):
        y = self.norm(self.dwconv(x))
        y = self.pwconv2(self.act(self.pwconv1(y)))
        return self.scale(y, x)


class ConvNeXt(nn.Module):
    def __init__(self, depths, dims, num_classes: int = 10,
                 in_channels: int = 3):
        super().__init__()
        self.stem = nn.Sequential(
            PsConv2d(in_channels, dims[0], 3, padding=1),
            PsLayerNorm2d(dims[0]))
        stages = []
        for i, (depth, dim) in enumerate(zip(depths, dims)):
            if i:
                stages += [PsLayerNorm2d(dims[i - 1]),
                           PsConv2d(dims[i - 1], dim, 2, stride=2)]
            stages += [ConvNeXtBlock(dim) for _ in range(depth)]
        self.stages = nn.Sequential(*stages)
        self.norm = PsLayerNorm2d(dims[-1])
        self.head = PsLinear(dims[-1], num_classes)

    def forward(self, x):
        out = global_avg_pool(self.stages(self.stem(x)))
        return self.head(self.norm(out[:, :, None, None]).flatten(1))


def convnext_param_count(depths, dims, num_classes: int = 10,
                         in_channels: int = 3) -> int:
    """Parameters of the layout above, term by term."""
    n = in_channels * 9 * dims[0] + dims[0] + 2 * dims[0]       # stem + LN
    for i, (depth, d) in enumerate(zip(depths, dims)):
        if i:
            p = dims[i - 1]
            n += 2 * p + p * 4 * d + d                          # LN + 2x2 conv
        # dw 7x7 + bias, LN, 1x1 up + bias, 1x1 down + bias, layer scale
        n += depth * (49 * d + d + 2 * d + 4 * d * d + 4 * d
                      + 4 * d * d + d + d)
    return n + 2 * dims[-1] + dims[-1] * num_classes + num_classes


def ConvNeXtTiny(num_classes: int = 10, in_channels: int = 3):
    return ConvNeXt((3, 3, 9, 3), (96, 192, 384, 768), num_classes, in_channels)


def ConvNeXtSmall(num_classes: int = 10, in_channels: int = 3):
    return ConvNeXt((3, 3, 27, 3), (96, 192, 384, 768), num_classes, in_channels)
