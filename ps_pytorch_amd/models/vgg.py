"""VGG family for CIFAR-shaped inputs (ref: src/model_ops/vgg.py:15-68).
BN variants use the fused PsBatchNorm2d (BN+ReLU in one NHWC kernel pass)."""
from __future__ import annotations

import torch.nn as nn

from ..ops.conv import PsConv2d
from ..ops.dropout import PsDropout, PsReLU
from ..ops.linear import PsLinear
from ..ops.modules import PsBatchNorm2d
from ..ops.pool import max_pool2d as ps_max_pool2d, global_avg_pool


class PsMaxPool2d(nn.Module):
    """nn.MaxPool2d(2,2) on the in-tree NHWC kernels (torch fallback on
    CPU); a module so make_layers stays an nn.Sequential."""

    def __init__(self, kernel_size: int, stride: int):
        super().__init__()
        self.kernel_size = kernel_size
        self.stride = stride

    def forward(self, x):
        return ps_max_pool2d(x, self.kernel_size, self.stride)


class PsGlobalAvgPool2d(nn.Module):
    """nn.AdaptiveAvgPool2d(1) on the in-tree NHWC kernels (torch fallback
    on CPU): [N,C,H,W] -> [N,C,1,1]. Parameter-free, so it keeps the
    reference's features index without touching the state_dict."""

    def forward(self, x):
        return global_avg_pool(x)[:, :, None, None]


_CFG = {
    'VGG11': [64, 'M', 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M'],
    'VGG13': [64, 64, 'M', 128, 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M'],
    'VGG16': [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M',
              512, 512, 512, 'M'],
    'VGG19': [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512,
              'M', 512, 512, 512, 512, 'M'],
}


def _make_layers(cfg, in_channels: int, batch_norm: bool) -> nn.Sequential:
    layers = []
    c = in_channels
    for v in cfg:
        if v == 'M':
            layers.append(PsMaxPool2d(2, 2))
        else:
            layers.append(PsConv2d(c, v, 3, padding=1, bias=not batch_norm))
            if batch_norm:
                layers.append(PsBatchNorm2d(v, relu=True))   # fused BN+ReLU
            else:
                layers.append(PsReLU())
            c = v
    layers.append(PsGlobalAvgPool2d())
    return nn.Sequential(*layers)


def _reference_head(num_classes: int) -> nn.Sequential:
    """The reference classifier (ref: src/model_ops/vgg.py:22-30): Dropout,
    Linear, ReLU, Dropout, Linear, ReLU, Linear — same indices, hence the
    same parameter keys classifier.{1,4,6}.{weight,bias}. The first ReLU is
    fused into the dropout behind it; entry 2 only holds its index."""
    return nn.Sequential(
        PsDropout(salt=0),
        PsLinear(512, 512),
        nn.Identity(),                  # ReLU fused into entry 3
        PsDropout(relu=True, salt=1),
        PsLinear(512, 512),
        PsReLU(),
        PsLinear(512, num_classes),
    )


class VGG(nn.Module):
    """classifier='lean': one PsLinear(512, nc). classifier='reference': the
    reference's three-layer dropout head (the *_ref factory names)."""

    def __init__(self, name: str, num_classes: int = 10, in_channels: int = 3,
                 batch_norm: bool = False, classifier: str = 'lean'):
        super().__init__()
        self.features = _make_layers(_CFG[name], in_channels, batch_norm)
        if classifier == 'lean':
            self.classifier = PsLinear(512, num_classes)
        elif classifier == 'reference':
            self.classifier = _reference_head(num_classes)
        else:
            raise ValueError(f"classifier must be 'lean' or 'reference', "
                             f"got {classifier!r}")

    def forward(self, x):
        x = self.features(x).flatten(1)
        return self.classifier(x)


def VGG11(num_classes=10, in_channels=3):
    return VGG('VGG11', num_classes, in_channels, False)


def VGG13(num_classes=10, in_channels=3):
    return VGG('VGG13', num_classes, in_channels, False)


def VGG16(num_classes=10, in_channels=3):
    return VGG('VGG16', num_classes, in_channels, False)


def VGG19(num_classes=10, in_channels=3):
    return VGG('VGG19', num_classes, in_channels, False)


def VGG11_BN(num_classes=10, in_channels=3):
    return VGG('VGG11', num_classes, in_channels, True)


def VGG13_BN(num_classes=10, in_channels=3):
    return VGG('VGG13', num_classes, in_channels, True)


def VGG16_BN(num_classes=10, in_channels=3):
    return VGG('VGG16', num_classes, in_channels, True)


def VGG19_BN(num_classes=10, in_channels=3):
    return VGG('VGG19', num_classes, in_channels, True)


def _ref_factory(name: str, batch_norm: bool):
    def make(num_classes=10, in_channels=3):
        return VGG(name, num_classes, in_channels, batch_norm,
                   classifier='reference')
    make.__name__ = f"{name}{'_BN' if batch_norm else ''}_ref"
    return make


# factory names with the reference classifier head: vggNN_ref maps to the BN
# variant, as vggNN does
REF_FACTORY = {}
for _n in ('VGG11', 'VGG13', 'VGG16', 'VGG19'):
    REF_FACTORY[f'{_n.lower()}_ref'] = _ref_factory(_n, True)
    REF_FACTORY[f'{_n.lower()}_bn_ref'] = _ref_factory(_n, True)
    REF_FACTORY[f'{_n.lower()}_plain_ref'] = _ref_factory(_n, False)


def convert_reference_vgg_state_dict(sd, name: str):
    """Map a reference VGG state_dict (ref: src/model_ops/vgg.py) onto the
    matching *_ref model here.

    The reference's BN variants index features as (conv, bn, relu) triples
    and their convs carry biases; here features are (conv, PsBatchNorm2d)
    pairs with bias-free convs. A conv bias b in front of a BatchNorm is
    folded exactly as running_mean -= b: in training mode it cancels in
    x - mean(x) anyway, in eval mode bn(conv + b) with mean m equals
    bn(conv) with mean m - b. Plain variants have the same key layout and
    come back unchanged."""
    key = name.lower()
    if key not in REF_FACTORY:
        raise ValueError(f"{name!r} is not a reference-head VGG name; "
                         f"have {sorted(REF_FACTORY)}")
    if key.endswith('_plain_ref'):
        return dict(sd)
    cfg = _CFG[key.split('_')[0].upper()]
    out = {k: v for k, v in sd.items() if not k.startswith('features.')}
    src = dst = 0
    for v in cfg:
        if v == 'M':
            src += 1
            dst += 1
            continue
        out[f'features.{dst}.weight'] = sd[f'features.{src}.weight']
        for k in ('weight', 'bias', 'running_var', 'num_batches_tracked'):
            if f'features.{src + 1}.{k}' in sd:
                out[f'features.{dst + 1}.{k}'] = sd[f'features.{src + 1}.{k}']
        mean = sd[f'features.{src + 1}.running_mean']
        b = sd.get(f'features.{src}.bias')
        out[f'features.{dst + 1}.running_mean'] = (
            mean - b.to(mean.dtype) if b is not None else mean.clone())
        src += 3
        dst += 2
    return out
