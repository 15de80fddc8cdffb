"""CPU checks of the BatchNorm oracle (tests/bn_utils.py): the float64
reference against torch.nn.functional.batch_norm and autograd, the
PsBatchNorm2d CPU fallback against the reference, and for every row of the
case table the two conditions the GPU tests rest on: the lattice sums are
exact in f32, and at most 0.1 % of a case's elements lie inside the band in
which the bound on v leaves the relu decision open."""
import pytest
import torch
import torch.nn.functional as F

import bn_utils as bu
from ps_pytorch_amd.ops.modules import PsBatchNorm2d

F64 = torch.float64
SMALL = [c for c in bu.CASES if c[1] * c[2] <= 1 << 18]


def _nchw(t, N, H, W):
    return t.view(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('M', [1, 6, 35])
def test_oracle_matches_torch_float64(M, with_res, relu):
    C = 8
    gen = bu._gen('oracle_vs_torch', M, with_res, relu)
    x, dy = (torch.randn(M, C, generator=gen, dtype=F64) for _ in range(2))
    res = torch.randn(M, C, generator=gen, dtype=F64) if with_res else None
    gam, beta = bu.params(C, gen)
    rm = torch.randn(C, generator=gen, dtype=F64)
    rv = torch.rand(C, generator=gen, dtype=F64) + 0.5
    o = bu.ref_fwd(x, gam, beta, res, relu, rm, rv, momentum=0.1)

    xt, gt, bt = (t.clone().requires_grad_(True) for t in (x, gam, beta))
    rt = res.clone().requires_grad_(True) if with_res else None
    rm_t, rv_t = rm.clone(), rv.clone()
    if M > 1:       # torch refuses one value per channel in training
        y = F.batch_norm(_nchw(xt, 1, M, 1), rm_t, rv_t, gt, bt, True, 0.1,
                         bu.EPS)
        y = _rows(y)
    else:           # M = 1: var = 0 and the guarded unbiased factor
        y = (xt - xt.detach()) * gt / bu.EPS ** 0.5 + bt
        rm_t = 0.9 * rm + 0.1 * x[0]
        rv_t = 0.9 * rv
    if with_res:
        y = y + rt
    if relu:
        y = F.relu(y)
    torch.testing.assert_close(o['y'], y.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(o['running_mean'], rm_t, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(o['running_var'], rv_t, rtol=1e-12, atol=1e-12)
    if M == 1:
        return
    y.backward(dy)
    r = bu.ref_bwd(x, dy, gam, o['mean'], o['invstd'],
                   o['mask'] if relu else None)
    tol = dict(rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(r['dx'], xt.grad, **tol)
    torch.testing.assert_close(r['dgamma'], gt.grad, **tol)
    torch.testing.assert_close(r['dbeta'], bt.grad, **tol)
    if with_res:
        torch.testing.assert_close(r['dres'], rt.grad, **tol)


def test_oracle_eval_matches_torch_float64():
    gen = bu._gen('oracle_eval')
    M, C = 12, 8
    x, res = (torch.randn(M, C, generator=gen, dtype=F64) for _ in range(2))
    gam, beta = bu.params(C, gen)
    rm = torch.randn(C, generator=gen, dtype=F64)
    rv = torch.rand(C, generator=gen, dtype=F64) + 0.5
    o = bu.ref_fwd(x, gam, beta, res, True, rm, rv, training=False)
    y = F.relu(_rows(F.batch_norm(_nchw(x, 2, 3, 2), rm, rv, gam, beta, False,
                                  0.1, bu.EPS)) + res)
    torch.testing.assert_close(o['y'], y, rtol=1e-12, atol=1e-12)
    assert 'running_mean' not in o


def test_mask_unpack_bit_order():
    M, C = 3, 16
    bits = torch.zeros(M, C, dtype=torch.bool)
    bits[0, 0] = bits[1, 9] = bits[2, 7] = bits[2, 15] = True
    packed = torch.zeros(M * C // 8, dtype=torch.uint8)
    packed[0], packed[3], packed[4], packed[5] = 1, 2, 128, 128
    assert torch.equal(bu.unpack_mask(packed, M, C), bits)


@pytest.mark.parametrize('case', [bu.TAIL_CASE, bu.RAGGED_CASE,
                                  ('tail_lt_R', 8, 5, 1, 1),
                                  ('tail_edge', 64, 257, 1, 1)],
                         ids=lambda c: f"C{c[1]}-M{c[2]}")
def test_cpu_fallback_matches_oracle(case):
    """The module's torch path (f32: its running statistics are always f32)
    on lattice rows of the table. It is torch's arithmetic, not the
    kernel's contract, so the tolerance is the plain one of test_bn.py,
    1e-6 per unit of the largest reference value, times M / 64 + 1 for the
    longer sums here."""
    _, C, M, relu, _ = case
    x, res, dy, gam, beta = bu.bn_case(case)
    m = PsBatchNorm2d(C, eps=bu.EPS, momentum=bu.MOMENTUM, relu=bool(relu))
    with torch.no_grad():
        m.weight.copy_(gam)
        m.bias.copy_(beta)
    xt = _nchw(x.float(), 1, M, 1).requires_grad_(True)
    rt = (_nchw(res.float(), 1, M, 1).requires_grad_(True)
          if res is not None else None)
    y = m(xt, residual=rt)
    o = bu.ref_fwd(x, gam, beta, res, bool(relu), torch.zeros(C, dtype=F64),
                   torch.ones(C, dtype=F64))
    fb = bu.fwd_bounds(x, gam, beta, res, o)
    assert not bu.undecided(o, fb).any()    # torch's relu decides as we do
    y.backward(_nchw(dy.float(), 1, M, 1))
    r = bu.ref_bwd(x, dy, gam, o['mean'], o['invstd'],
                   o['mask'] if relu else None)

    def close(got, ref):
        tol = 1e-6 * (M / 64 + 1) * float(ref.abs().max().clamp_min(1))
        assert float((got.detach().to(F64) - ref).abs().max()) <= tol

    close(_rows(y), o['y'])
    close(m.running_mean, o['running_mean'])
    close(m.running_var, o['running_var'])
    close(_rows(xt.grad), r['dx'])
    close(m.weight.grad, r['dgamma'])
    close(m.bias.grad, r['dbeta'])
    if res is not None:
        close(_rows(rt.grad), r['dres'])


def test_table_covers_what_it_claims():
    groups = {}
    for grp, C, M, relu, res in bu.CASES:
        assert C in bu.ENVELOPE_C
        groups.setdefault(grp, set()).add((relu, res))
    for grp, combos in groups.items():
        want = {(1, 1)} if grp == 'capped' else set(bu.RR)
        assert combos == want, (grp, combos)
    assert {c[1] for c in bu.CASES if c[0] == 'envelope'} == set(bu.ENVELOPE_C)
    nb = sorted(bu.stats_blocks(c[2], c[1]) for c in bu.CASES if c[0] == 'fold')
    assert nb == [255, 256, 256, 258]
    for grp, C, M, *_ in bu.CASES:
        R, chunk = bu.rows_per_pass(C), 8 * bu.rows_per_pass(C)
        if grp == 'tail_lt_R':
            assert M < R
        if grp == 'capped':         # a second grid pass and a partial one
            assert M > 1024 * chunk and M % chunk
        if grp in ('ragged', 'envelope'):
            assert M % chunk and M > chunk and (R == 1 or M % R)


@pytest.mark.parametrize('case', bu.CASES, ids=bu.CASE_IDS)
def test_case_is_exact_and_decided(case):
    """bn_case asserts lattice exactness; here the sums are also formed in
    f32 in two different orders, and the undecided share is counted with
    the bound of the type whose band is widest (it is the same: the mask is
    taken on the f32 v in both)."""
    _, C, M, relu, _ = case
    x, res, dy, gam, beta = bu.bn_case(case)
    x32 = x.float()
    for t in (x32, x32 * x32, dy.float()):
        ref = t.to(F64).sum(0)
        assert torch.equal(t.sum(0).to(F64), ref)
        assert torch.equal(t.flip(0).cumsum(0)[-1].to(F64), ref)
    for t in (x, res, dy, gam, beta):
        if t is not None:
            assert torch.equal(t.bfloat16().to(F64), t)
    rm, rv = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    o = bu.ref_fwd(x, gam, beta, res, bool(relu), rm, rv)
    fb = bu.fwd_bounds(x, gam, beta, res, o, rm, rv)
    share = float(bu.undecided(o, fb).double().mean())
    print(f"{case}: undecided share {share:.3g}")
    assert share <= 1e-3


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_offset_case_is_exact_and_decided(bf16):
    x, res, dy, gam, beta = bu.offset_case(bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    assert torch.equal(x.to(dt).to(F64), x)
    x32 = x.float()
    assert torch.equal((x32 * x32).sum(0).to(F64), (x * x).sum(0))
    assert torch.equal((x32 * x32).flip(0).cumsum(0)[-1].to(F64), (x * x).sum(0))
    o = bu.ref_fwd(x, gam, beta, res, True)
    assert float(o['var'][4]) == 0.0
    assert abs(float(o['mean'][5]) - 2) < 1e-12 and abs(float(o['var'][5]) - 1) < 1e-12
    fb = bu.fwd_bounds(x, gam, beta, res, o)
    assert float(bu.undecided(o, fb).double().mean()) <= 1e-3


def test_bound_terms_have_the_documented_size():
    """The cancellation terms are in the bounds: at mean 64, std ~0.6 the
    bound on var is about 4u E[x^2] and the bound on v carries
    2u |mean scale|."""
    x, res, dy, gam, beta = bu.offset_case(False)
    o = bu.ref_fwd(x, gam, beta, None, False)
    fb = bu.fwd_bounds(x, gam, beta, None, o)
    c = 0
    assert 3.9 * bu.U * o['e2'][c] < fb['var'][c] < 4.1 * bu.U * o['e2'][c]
    floor = 2 * bu.U * (o['mean'][c] * o['scale'][c]).abs()
    assert bool((fb['v'][:, c] > floor).all())
    half = 0.5 * fb['var'][c] / (o['var'][c] + bu.EPS)
    assert half < fb['invstd'][c] / o['invstd'][c] < 1.1 * half
