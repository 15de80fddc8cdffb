"""CPU tests of the GroupNorm layer: the torch fallback of PsGroupNorm2d, its
state-dict surface, the GN ResNet factory names, the resident / streamed plan
rule, and the case table of tests/gn_utils.py (lattice condition and mask
cap, from the float64 reference alone)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_utils as bu
import gn_utils as gu
from ps_pytorch_amd.models import build_model
from ps_pytorch_amd.ops.modules import PsGroupNorm2d, _gn_plan


@pytest.mark.parametrize("relu,with_res", bu.RR)
def test_fallback_equals_group_norm(relu, with_res):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 24, 5, 3, generator=gen)
    res = torch.randn(2, 24, 5, 3, generator=gen) if with_res else None
    m = PsGroupNorm2d(3, 24, eps=1e-4, relu=bool(relu))
    with torch.no_grad():
        m.weight.copy_(torch.randn(24, generator=gen))
        m.bias.copy_(torch.randn(24, generator=gen))
    ref = F.group_norm(x, 3, m.weight, m.bias, 1e-4)
    ref = ref + res if with_res else ref
    ref = F.relu(ref) if relu else ref
    for mod in (m.train(), m.eval()):
        assert torch.equal(mod(x, residual=res), ref)
    assert (m.kernel_calls, m.fallback_calls) == (0, 2)


def test_state_dict_is_group_norms():
    ours = PsGroupNorm2d(4, 32, relu=True).state_dict()
    theirs = nn.GroupNorm(4, 32).state_dict()
    assert list(ours) == list(theirs)
    assert all(ours[k].shape == theirs[k].shape for k in ours)
    nn.GroupNorm(4, 32).load_state_dict(ours)


def test_resnet18_gn_factory():
    gn, bn = build_model('resnet18_gn'), build_model('resnet18')
    count = lambda net: sum(p.numel() for p in net.parameters())
    assert count(gn) == count(bn) == 11173962
    assert list(gn.buffers()) == []
    assert [k for k, _ in gn.named_parameters()] == \
        [k for k, _ in bn.named_parameters()]
    norms = [m for m in gn.modules() if isinstance(m, PsGroupNorm2d)]
    assert len(norms) == 20 and all(m.num_groups == 32 for m in norms)
    for name in ('resnet34_gn', 'resnet50_gn', 'resnet101_gn', 'resnet152_gn'):
        assert not list(build_model(name).buffers())
    gn.eval()
    assert gn(torch.randn(2, 3, 32, 32)).shape == (2, 10)


# HW, C, Cg, elt, tiles -> slab channels (bytes per pixel = slab * elt)
PLAN_TABLE = [
    (512, 64, 2, 2, 1, 64), (513, 64, 2, 2, 1, 32), (1024, 64, 16, 2, 1, 32),
    (1025, 64, 16, 2, 1, 0),
    (256, 64, 2, 2, 2, 64), (257, 64, 4, 2, 2, 32), (512, 64, 2, 2, 2, 32),
    (513, 64, 4, 2, 2, 0),
    (256, 2048, 64, 4, 1, 64), (257, 2048, 64, 4, 1, 0),
    (128, 2048, 64, 4, 2, 64), (129, 2048, 64, 4, 2, 0),
    (512, 64, 2, 4, 1, 32), (1024, 64, 2, 4, 1, 16),     # f32: bytes decide
    (1024, 32, 2, 2, 1, 32), (1024, 8, 8, 2, 1, 8),      # C below a segment
    (50, 96, 32, 2, 1, 96), (50, 96, 32, 4, 1, 32),      # SC must divide C
    (16, 2008, 8, 2, 1, 2008), (8, 2008, 8, 4, 1, 0),    # 502 f32 lanes > 256
]


@pytest.mark.parametrize("HW,C,Cg,elt,tiles,slab", PLAN_TABLE)
def test_plan(HW, C, Cg, elt, tiles, slab):
    assert _gn_plan(HW, C, Cg, elt, tiles) == slab
    if slab:
        assert slab % Cg == 0 and slab % 8 == 0 and C % slab == 0
        assert tiles * HW * slab * elt <= 64 * 1024


@pytest.mark.parametrize("case", gu.CASES, ids=gu.CASE_IDS)
def test_case_table_row(case):
    """gn_case asserts the lattice condition; here the mask cap: at most
    0.1 % of a row's elements have a relu decision the bound leaves open."""
    _, N, HW, C, G, relu, res = case
    assert C // G in (2, 4, 8, 16, 32, 64) and C % 8 == 0
    gu.gn_case(case)
    und = sum(int(bu.undecided(o, fb).sum()) for o, fb in gu.fwd_ref(case))
    assert und <= 1e-3 * N * HW * C, und


def test_case_table_covers():
    rows = gu.CASES
    assert {c[3] // c[4] for c in rows} == {2, 4, 8, 16, 32, 64}
    assert {(c[5], c[6]) for c in rows} == set(bu.RR)
    assert {c[1] for c in rows} == {1, 3}
    for elt in (2, 4):
        forms = {tuple(bool(s) for s in gu.plans(c, elt)) for c in rows}
        assert forms == {(True, True), (True, False), (False, False)}
