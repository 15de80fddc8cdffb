"""CPU tests of PsLayerNorm2d, PsGELU, PsLayerScaleAdd (torch fallback), the
row plan of layernorm.hip and the ConvNeXt builder."""
import math

import pytest
import torch
import torch.nn.functional as F

from ps_pytorch_amd.models import build_model
from ps_pytorch_amd.models.convnext import convnext_param_count
from ps_pytorch_amd.ops import modules as pm


def test_modules_fall_back_on_cpu_and_match_float64():
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 24, 3, 5, generator=gen).contiguous(
        memory_format=torch.channels_last)
    res = torch.randn(2, 24, 3, 5, generator=gen)
    ln, ge, ls = pm.PsLayerNorm2d(24), pm.PsGELU(), pm.PsLayerScaleAdd(24, init=0.5)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(24, generator=gen))
        ln.bias.copy_(torch.randn(24, generator=gen))
    x64 = x.double()
    want = {
        ln: F.layer_norm(x64.permute(0, 2, 3, 1), (24,), ln.weight.double(),
                         ln.bias.double(), ln.eps).permute(0, 3, 1, 2),
        ge: 0.5 * x64 * (1 + torch.erf(x64 / math.sqrt(2))),
        ls: res.double() + 0.5 * x64,
    }
    got = {ln: ln(x), ge: ge(x), ls: ls(x, res)}
    for m in (ln, ge, ls):
        assert (m.kernel_calls, m.fallback_calls) == (0, 1)
        assert got[m].shape == x.shape
        torch.testing.assert_close(got[m].double(), want[m], rtol=1e-5, atol=1e-5)
    assert sorted(ln.state_dict()) == ['bias', 'weight']


def test_convnext_tiny_builds_and_trains_a_step_on_cpu():
    m = build_model('convnext_tiny', num_classes=10)
    # stem 3*9*96 + 96 and its LN; per block 49C + C, LN 2C, 4C^2 + 4C,
    # 4C^2 + C, C; per downsample LN 2C' + 4C'C + C; head LN + linear
    assert convnext_param_count((3, 3, 9, 3), (96, 192, 384, 768)) == 27_825_802
    assert sum(p.numel() for p in m.parameters()) == 27_825_802
    out = m(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10)
    F.cross_entropy(out, torch.tensor([1, 7])).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in m.parameters())


@pytest.mark.parametrize("M", [1, 63, 10 ** 6])
@pytest.mark.parametrize("C,elt", [(8, 2), (96, 2), (768, 4), (2048, 4)])
def test_ln_plan_covers_every_row_under_the_cap(M, C, elt):
    rpb, blocks = pm._ln_plan(M, C, elt)
    gran = C // (16 // elt)
    unit = 256 // min(64, max(8, 1 << (gran - 1).bit_length()))
    assert rpb % unit == 0 and blocks * rpb >= M
    assert 1 <= blocks <= pm._LN_MAX_BLOCKS and (blocks - 1) * rpb < M
