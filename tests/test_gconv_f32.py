"""CPU half of the f32 grouped-convolution tests: the support predicate,
the wgrad split rule and the range condition of the exact GPU test."""
import pytest
import torch

import gconv_f32_utils as gfu
from ps_pytorch_amd.ops import conv as ps_conv
from test_gconv import _FakeCuda

F32, BF = torch.float32, torch.bfloat16


def _ok(C, G, dtype=F32, R=3, stride=1, dil=1, K=None, is_cuda=True,
        wdtype=None):
    x = _FakeCuda(dtype, (2, C, 8, 8))
    x.is_cuda = is_cuda
    w = torch.zeros(K or C, C // G, R, R, dtype=wdtype or dtype)
    return ps_conv._group_f32_supported(
        x, w, (stride, stride), (1, 1), (dil, dil), G)


def test_group_f32_supported_is_the_envelope(monkeypatch):
    for C, G in ((64, 16), (128, 16), (192, 12), (64, 2), (128, 2)):
        assert _ok(C, G)
    assert _ok(128, 32, R=7, stride=2)
    assert not _ok(128, 32, BF)                 # bf16 has its own family
    assert not _ok(128, 32, wdtype=BF)
    assert not _ok(128, 64)                     # Cg = 2
    assert not _ok(256, 2)                      # Cg = 128
    assert not _ok(96, 6)                       # C = 96
    assert not _ok(128, 32, dil=2)
    assert not _ok(128, 32, stride=3)
    assert not _ok(128, 32, K=256)              # C != K
    assert not _ok(128, 32, is_cuda=False)
    assert not _ok(64, 1)                       # dense stays dense
    assert not _ok(64, 64)                      # depthwise: Cg = 1
    for switch in ('_GCONV', '_F32', '_ENABLED'):
        with monkeypatch.context() as m:
            m.setattr(ps_conv, switch, False)
            assert not _ok(128, 32)


def test_gconv_wgrad_split_f32_corners():
    s = ps_conv._gconv_wgrad_split_f32
    assert s(105, 64, 3, 4) == 1                # under 128 pixels
    assert s(1280, 128, 3, 4) == 20             # 64-pixel chunk floor
    assert s(1 << 20, 64, 3, 8) == 1024         # one-wave form: chunk cap
    assert s(1 << 20, 64, 5, 8) == 409          # tap rows in the grid
    assert s(1 << 20, 64, 1, 16) == 256         # block form: chunk cap
    assert s(32768, 128, 3, 32) == 28           # 512 // 18 tiles
    assert s(32768, 1024, 7, 64) == 1           # more tiles than the target


@pytest.mark.parametrize("case", gfu.CASES)
def test_exact_references_stay_in_range(case):
    gfu.assert_in_range(gfu.exact_case(case)[5:])
