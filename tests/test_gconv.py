"""CPU half of the grouped-convolution tests: the lattice range condition,
the support predicate, the wgrad split rule and the ResNeXt models."""
import pytest
import torch

import conv_lattice as cl
import gconv_utils as gu
from ps_pytorch_amd.models import build_model
from ps_pytorch_amd.ops import conv as ps_conv

BF = torch.bfloat16


@pytest.mark.parametrize("case", gu.CASES)
def test_reference_stays_in_range(case):
    """|ref| <= 256 (plus the bias on the bias case), so the one bf16
    rounding of every output is exact."""
    x, w, b, dy, out, dx, dw = gu.gconv_case(case)
    refs = [out, dx, dw]
    if case == gu.BIAS_CASE:
        refs += [out + b.view(1, -1, 1, 1), dy.sum((0, 2, 3))]
    assert max(float(r.abs().max()) for r in refs) <= cl.RANGE


class _FakeCuda:
    """Just enough tensor surface for the support predicates."""

    def __init__(self, dtype, shape):
        self.dtype, self.shape, self.is_cuda = dtype, shape, True

    def dim(self):
        return len(self.shape)


def _gok(C, G, dtype=BF, R=3, stride=1, dil=1, K=None, is_cuda=True):
    x = _FakeCuda(dtype, (2, C, 8, 8))
    x.is_cuda = is_cuda
    w = torch.zeros(K or C, C // G, R, R, dtype=dtype)
    args = (x, w, (stride, stride), (1, 1), (dil, dil), G)
    return ps_conv._group_supported(*args), ps_conv._supported(*args)


def test_group_supported_is_the_envelope(monkeypatch):
    for C, G in ((64, 16), (128, 16), (192, 12), (64, 2), (128, 2)):
        assert _gok(C, G) == (True, False)      # _supported rejects groups
    assert _gok(128, 32, R=7, stride=2)[0]
    assert not _gok(128, 32, torch.float32)[0]
    assert not _gok(128, 64)[0]                 # Cg = 2
    assert not _gok(256, 2)[0]                  # Cg = 128
    assert not _gok(96, 6)[0]                   # C = 96
    assert not _gok(128, 32, dil=2)[0]
    assert not _gok(128, 32, stride=3)[0]
    assert not _gok(128, 32, K=256)[0]          # C != K
    assert not _gok(128, 32, is_cuda=False)[0]
    assert _gok(64, 1) == (False, True)         # dense stays dense
    monkeypatch.setattr(ps_conv, '_GCONV', False)
    assert not _gok(128, 32)[0]


def test_gconv_wgrad_split_corners():
    s = ps_conv._gconv_wgrad_split
    assert s(105, 64, 9) == 1                   # under 128 pixels
    assert s(1280, 128, 9) == 20                # 64-pixel chunk floor
    assert s(1 << 20, 64, 1) == 256             # chunk-count cap
    assert s(32768, 128, 9) == 28               # 512 // 18 tiles
    assert s(32768, 1024, 49) == 1              # more tiles than the target


@pytest.mark.parametrize("name,widths", [
    ('resnext29_32x4d', [128] * 3 + [256] * 3 + [512] * 3),
    ('resnext50_32x4d', [128] * 3 + [256] * 4 + [512] * 6 + [1024] * 3)])
def test_resnext_builds_and_trains_on_cpu(name, widths):
    net = build_model(name, num_classes=10)
    grouped = [m for m in net.modules()
               if isinstance(m, ps_conv.PsConv2d) and m.groups > 1]
    assert [tuple(m.weight.shape) for m in grouped] == \
        [(wd, wd // 32, 3, 3) for wd in widths]
    out = net(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10)
    out.sum().backward()
    assert all(m.weight.grad is not None and bool(m.weight.grad.any())
               for m in grouped)
