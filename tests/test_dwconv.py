"""CPU half of the depthwise-convolution tests: the lattice range condition,
the support predicate, the wgrad split rule and the MobileNet model."""
import pytest
import torch

import conv_lattice as cl
import dwconv_utils as du
from ps_pytorch_amd.models import build_model
from ps_pytorch_amd.ops import conv as ps_conv

BF = torch.bfloat16


@pytest.mark.parametrize("case", du.CASES)
def test_reference_stays_in_range(case):
    """|ref| <= 256 (plus the bias on the bias case), so the one rounding
    of every output is exact in bf16 as in f32."""
    x, w, b, dy, out, dx, dw = du.dwconv_case(case)
    refs = [out, dx, dw]
    if case == du.BIAS_CASE:
        refs += [out + b.view(1, -1, 1, 1), dy.sum((0, 2, 3))]
    assert max(float(r.abs().max()) for r in refs) <= cl.RANGE


class _FakeCuda:
    """Just enough tensor surface for the support predicates."""

    def __init__(self, dtype, shape, is_cuda=True):
        self.dtype, self.shape, self.is_cuda = dtype, shape, is_cuda

    def dim(self):
        return len(self.shape)


def _ok(C, dtype=BF, R=3, stride=1, dil=1, pad=1, K=None, G=None,
        is_cuda=True):
    x = _FakeCuda(dtype, (2, C, 8, 8), is_cuda)
    w = torch.zeros(K or C, C // (G or C), R, R, dtype=dtype)
    args = (x, w, (stride, stride), (pad, pad), (dil, dil), G or C)
    return (ps_conv._dw_supported(*args), ps_conv._supported(*args),
            ps_conv._group_supported(*args))


def test_dw_supported_is_the_envelope(monkeypatch):
    for dtype in (BF, torch.float32):
        for C, R, stride in ((8, 3, 1), (72, 5, 2), (1024, 7, 1)):
            # the dense and the grouped predicate keep rejecting depthwise
            assert _ok(C, dtype, R, stride, pad=R // 2) == (True, False, False)
    assert not _ok(12)[0]                       # C % 8
    assert not _ok(64, K=128)[0]                # channel multiplier
    assert not _ok(64, G=32)[0]                 # groups != C
    assert _ok(64, G=16) == (False, False, True)    # grouped stays grouped
    assert not _ok(64, R=1, pad=0)[0]
    assert not _ok(64, R=9, pad=4)[0]
    assert not _ok(64, dil=2)[0]
    assert not _ok(64, stride=3)[0]
    assert not _ok(64, pad=3)[0]                # pad >= R
    assert not _ok(64, is_cuda=False)[0]
    monkeypatch.setattr(ps_conv, '_F32', False)
    assert not _ok(64, torch.float32)[0] and _ok(64)[0]
    monkeypatch.setattr(ps_conv, '_DWCONV', False)
    assert not _ok(64)[0]


def test_dwconv_wgrad_split_corners():
    s = ps_conv._dwconv_wgrad_split
    assert s(105, 8, 3) == 1                    # under one 256-pixel chunk
    assert s(1280, 128, 3) == 5                 # 256-pixel chunk floor
    assert s(1 << 20, 32, 3) == 256             # chunk-count cap
    assert s(1 << 20, 512, 3) == 64             # 512 // 8 slabs
    assert s(1 << 20, 512, 3, 32) == 32         # f32: 32-channel slabs
    assert s(1 << 20, 72, 7) == 36              # 2 slabs x 7 tap rows
    assert s(1 << 20, 65536, 7) == 1            # more tiles than the target


def test_mobilenet_builds_and_trains_on_cpu():
    net = build_model('mobilenet', num_classes=10)
    dw = [m for m in net.modules()
          if isinstance(m, ps_conv.PsConv2d) and m.groups > 1]
    widths = [32, 64, 128, 128, 256, 256] + [512] * 6 + [1024]
    assert [tuple(m.weight.shape) for m in dw] == \
        [(wd, 1, 3, 3) for wd in widths]
    assert all(m.groups == m.in_channels == m.out_channels for m in dw)
    assert [m.stride[0] for m in dw] == [1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1]
    assert build_model('mobilenet', num_classes=1000).conv1.stride == (2, 2)
    out = net(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10)
    out.sum().backward()
    assert all(m.weight.grad is not None and bool(m.weight.grad.any())
               for m in dw)
