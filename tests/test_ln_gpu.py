"""GPU tests of ops/kernels/layernorm.hip (channel LayerNorm, GELU, layer
scale + residual) through the raw entry points on NaN-filled outputs, then
through the modules and one ConvNeXt block. References are float64 torch on
the CPU, computed from the inputs as rounded to the io type.

LayerNorm bounds are gamma(k) times the formula in absolute values, k an
upper count of the f32 roundings on the path (contract in layernorm.hip):
  y      C adds of the row sum, the division, the two subtractions of the
         refined mean (its remainder sum is compensated: one rounding), C
         adds of the variance, division, + eps, rsqrt, three products/adds:
         2C + 11, under the 2C + 16 of the bound
  dx     the same centring and invstd, then gamma*dy, the two row sums of C
         adds each are counted through mean_C: 2C + 24
  dgamma x-hat (2C + 16 as above) and the M adds over the rows
  dbeta  the M adds over the rows (+ 16 for the two folds' extra levels)
bf16 adds 2^-8 of the value for the one rounding of the output. That holds
for dlambda as for dgamma and dbeta: the column sum is carried in f32 and
rounded once to the parameter type by the fold kernel, so its bf16 bound is
gamma(M + 16) * sum|dout*y| + 2^-8 * |dlambda|.

assert_within compares with err > bound, which a NaN passes; every output is
therefore also asserted finite, so an element the kernel never stored fails.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from f32_ref import U, assert_within, gamma as g
from ps_pytorch_amd.ops import current_stream_ptr, dtype_tag, require_lib
from ps_pytorch_amd.ops import modules as pm

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
EPS = 1e-6
CASES = [(1, 8), (7, 24), (65, 64), (33, 520), (5, 2048), 'blocks3', 'cap']
SHAPES = pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])


def _shape(case, dtype):
    elt = 2 if dtype == BF else 4
    if case == 'blocks3':       # three blocks, the last with one row
        return 2 * pm._ln_plan(1, 96, elt)[0] + 1, 96
    if case == 'cap':           # one row past where the floor fills the cap
        return pm._LN_MAX_BLOCKS * pm._ln_plan(1, 8, elt)[0] + 1, 8
    return case


def _inputs(M, C, dtype):
    """Seeded inputs rounded to dtype, as float64 CPU tensors: two [M, C]
    activations with a per-row offset of up to +-4, two gradients, three
    parameter vectors of order 1."""
    gen = torch.Generator().manual_seed(1000 * C + M % 1000)
    r = lambda *s: torch.randn(*s, generator=gen)
    off = lambda: (torch.rand(M, 1, generator=gen) * 8 - 4)
    ts = [r(M, C) + off(), r(M, C) + off(), r(M, C), r(M, C), r(C), r(C), r(C)]
    return [t.to(dtype).to(F64) for t in ts]


def _dev(t, dtype):
    return t.to(dtype).cuda()


def _nan(n, dtype):
    return torch.full((n,), float('nan'), dtype=dtype, device='cuda')


def _io(bound, ref, dtype):
    return bound + (2.0 ** -8) * ref.abs() if dtype == BF else bound


def _ln_raw(x, dy, gam, beta, dtype, plan=None):
    M, C = x.shape
    lib, tag, s = require_lib(), dtype_tag(dtype), current_stream_ptr()
    rpb, blocks = plan or pm._ln_plan(M, C, 2 if dtype == BF else 4)
    xd, dyd, gd, bd = (_dev(t, dtype) for t in (x, dy, gam, beta))
    o = {'y': _nan(M * C, dtype), 'dx': _nan(M * C, dtype),
         'dgamma': _nan(C, dtype), 'dbeta': _nan(C, dtype),
         'mean': _nan(M, F32), 'invstd': _nan(M, F32),
         'partial': _nan(blocks * 2 * C, F32), 'y_nostats': _nan(M * C, dtype)}
    p = {k: v.data_ptr() for k, v in o.items()}
    rc = (lib.ps_ln_fwd(xd.data_ptr(), p['y'], gd.data_ptr(), bd.data_ptr(),
                        p['mean'], p['invstd'], M, C, EPS, rpb, blocks, tag, s),
          lib.ps_ln_bwd(xd.data_ptr(), dyd.data_ptr(), gd.data_ptr(), p['mean'],
                        p['invstd'], p['dx'], p['dgamma'], p['dbeta'],
                        p['partial'], M, C, rpb, blocks, tag, s),
          # null statistics pointers: what the module passes under no_grad
          lib.ps_ln_fwd(xd.data_ptr(), p['y_nostats'], gd.data_ptr(),
                        bd.data_ptr(), None, None, M, C, EPS, rpb, blocks, tag, s))
    torch.cuda.synchronize()
    return rc, {k: v.cpu() for k, v in o.items()}


@DTYPES
@SHAPES
def test_layernorm(case, dtype):
    M, C = _shape(case, dtype)
    x, _, dy, _, gam, beta, _ = _inputs(M, C, dtype)
    rc, got = _ln_raw(x, dy, gam, beta, dtype)
    assert rc == (0, 0, 0)
    for k, v in got.items():    # y, dx, dgamma, dbeta, mean, invstd, partial
        assert torch.isfinite(v).all(), f"{k}: an element is NaN or was never stored"
    assert torch.equal(got['y_nostats'].view(torch.uint8), got['y'].view(torch.uint8))
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gam, beta))
    y = F.layer_norm(xr, (C,), gr, br, EPS)
    dx, dgam, dbeta = torch.autograd.grad(y, (xr, gr, br), dy)
    y = y.detach()
    invstd = (x.var(1, unbiased=False, keepdim=True) + EPS).rsqrt()
    xh = (x - x.mean(1, keepdim=True)) * invstd
    gg = gam * dy
    mc = lambda t: t.abs().mean(1, keepdim=True)
    tag = f"{case} {dtype}"
    assert_within(got['y'].view(M, C), y,
                  _io(g(2 * C + 16) * ((gam * xh).abs() + beta.abs()), y, dtype),
                  f"{tag} y")
    assert_within(got['dx'].view(M, C), dx,
                  _io(g(2 * C + 24) * invstd * (gg.abs() + mc(gg) + xh.abs() * mc(gg * xh)),
                      dx, dtype), f"{tag} dx")
    assert_within(got['dgamma'], dgam,
                  _io(g(M + 2 * C + 16) * (dy * xh).abs().sum(0), dgam, dtype),
                  f"{tag} dgamma")
    assert_within(got['dbeta'], dbeta,
                  _io(g(M + 16) * dy.abs().sum(0), dbeta, dtype), f"{tag} dbeta")


def _ls_raw(y, res, dout, lam, dtype, plan=None):
    M, C = y.shape
    lib, tag, s = require_lib(), dtype_tag(dtype), current_stream_ptr()
    rpb, blocks = plan or pm._ln_plan(M, C, 2 if dtype == BF else 4)
    yd, rd, dd, ld = (_dev(t, dtype) for t in (y, res, dout, lam))
    o = {'out': _nan(M * C, dtype), 'dy': _nan(M * C, dtype),
         'dlam': _nan(C, dtype), 'partial': _nan(blocks * C, F32)}
    rc = (lib.ps_lscale_fwd(yd.data_ptr(), rd.data_ptr(), ld.data_ptr(),
                            o['out'].data_ptr(), M, C, rpb, blocks, tag, s),
          lib.ps_lscale_bwd(yd.data_ptr(), dd.data_ptr(), ld.data_ptr(),
                            o['dy'].data_ptr(), o['dlam'].data_ptr(),
                            o['partial'].data_ptr(), M, C, rpb, blocks, tag, s))
    torch.cuda.synchronize()
    return rc, {k: v.cpu() for k, v in o.items()}


@DTYPES
@SHAPES
def test_layer_scale(case, dtype):
    M, C = _shape(case, dtype)
    y, res, dout, _, lam, _, _ = _inputs(M, C, dtype)
    rc, got = _ls_raw(y, res, dout, lam, dtype)
    assert rc == (0, 0)
    for k, v in got.items():    # out, dy, dlam, partial
        assert torch.isfinite(v).all(), f"{k}: an element is NaN or was never stored"
    u = 2.0 ** -8 if dtype == BF else U
    tag = f"{case} {dtype}"
    assert_within(got['out'].view(M, C), res + lam * y,
                  2 * u * (res.abs() + (lam * y).abs()), f"{tag} out")
    assert_within(got['dy'].view(M, C), lam * dout,
                  2 * u * (lam * dout).abs(), f"{tag} dy")
    dlam = (dout * y).sum(0)
    assert_within(got['dlam'], dlam,
                  _io(g(M + 16) * (dout * y).abs().sum(0), dlam, dtype),
                  f"{tag} dlam")


@DTYPES
@pytest.mark.parametrize("n", [8, 8 * 257, 8 * (1 << 15) + 8])
def test_gelu(n, dtype):
    """f32 bound: 4 x the largest error of torch's own f32 F.gelu on this
    GPU against float64, normalised by |x| + |y| (the device erff cannot be
    bounded from first principles); the same for dx against its autograd."""
    gen = torch.Generator().manual_seed(n)
    x = (torch.rand(n, generator=gen) * 16 - 8).to(dtype).to(F64)
    dy = torch.randn(n, generator=gen).to(dtype).to(F64)
    xr = x.clone().requires_grad_(True)
    y = 0.5 * xr * (1 + torch.erf(xr / math.sqrt(2)))
    (dx,) = torch.autograd.grad(y, xr, dy)
    y = y.detach()
    xt = x.float().cuda().requires_grad_(True)
    yt = F.gelu(xt)
    (dxt,) = torch.autograd.grad(yt, xt, dy.float().cuda())
    ey = ((yt.detach().cpu().double() - y).abs() / (x.abs() + y.abs()).clamp_min(1e-300)).max().item()
    ed = ((dxt.cpu().double() - dx).abs() / (dy.abs() + dx.abs()).clamp_min(1e-300)).max().item()
    print(f"torch f32 gelu n={n}: fwd {ey:.3g} bwd {ed:.3g} (normalised)")
    lib, tag, s = require_lib(), dtype_tag(dtype), current_stream_ptr()
    xd, dyd = _dev(x, dtype), _dev(dy, dtype)
    oy, od = _nan(n + 8, dtype), _nan(n + 8, dtype)
    assert lib.ps_gelu_fwd(xd.data_ptr(), oy.data_ptr(), n, tag, s) == 0
    assert lib.ps_gelu_bwd(xd.data_ptr(), dyd.data_ptr(), od.data_ptr(), n, tag, s) == 0
    torch.cuda.synchronize()
    assert torch.isnan(oy[n:]).all() and torch.isnan(od[n:]).all()
    assert torch.isfinite(oy[:n]).all() and torch.isfinite(od[:n]).all()
    assert_within(oy[:n], y, _io(4 * ey * (x.abs() + y.abs()), y, dtype), "gelu y")
    assert_within(od[:n], dx, _io(4 * ed * (dy.abs() + dx.abs()), dx, dtype), "gelu dx")


@DTYPES
def test_backward_bit_identical_across_runs(dtype):
    M, C = _shape('blocks3', dtype)
    x, y2, dy, _, gam, beta, lam = _inputs(M, C, dtype)
    a, b = (_ln_raw(x, dy, gam, beta, dtype)[1] for _ in range(2))
    c, d = (_ls_raw(x, y2, dy, lam, dtype)[1] for _ in range(2))
    for k in ('dx', 'dgamma', 'dbeta', 'partial'):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    for k in ('dy', 'dlam', 'partial'):
        assert torch.equal(c[k].view(torch.uint8), d[k].view(torch.uint8)), k


@pytest.mark.parametrize("C,short", [(12, 0), (2056, 0), (96, 1)])
def test_rejected_and_nothing_written(C, short):
    M = 300
    x, res, dy, _, gam, beta, lam = _inputs(M, C, F32)
    rpb, blocks = pm._ln_plan(M, 96, 4)
    bad = (rpb, blocks - short)
    rc, got = _ln_raw(x, dy, gam, beta, F32, plan=bad)
    assert all(r != 0 for r in rc), rc
    assert all(torch.isnan(v).all() for v in got.values())
    rc, got = _ls_raw(x, res, dy, lam, F32, plan=bad)
    assert all(r != 0 for r in rc), rc
    assert all(torch.isnan(v).all() for v in got.values())
    lib, tag, s = require_lib(), dtype_tag(F32), current_stream_ptr()
    xd, dyd, out = _dev(x, F32), _dev(dy, F32), _nan(M * C, F32)
    assert lib.ps_gelu_fwd(xd.data_ptr(), out.data_ptr(), 12, tag, s) != 0
    assert lib.ps_gelu_bwd(xd.data_ptr(), dyd.data_ptr(), out.data_ptr(), 12, tag, s) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


@DTYPES
def test_modules_equal_raw_entry_points(dtype):
    N, C, H, W = 2, 96, 5, 5
    M = N * H * W
    x, res, dy, _, gam, beta, lam = _inputs(M, C, dtype)
    nchw = lambda t: (_dev(t, dtype).view(N, H, W, C).permute(0, 3, 1, 2))
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1).cpu()
    same = lambda a, b: torch.equal(a.contiguous().view(torch.uint8),
                                    b.contiguous().view(torch.uint8))
    ln = pm.PsLayerNorm2d(C, eps=EPS).to('cuda', dtype)
    ls = pm.PsLayerScaleAdd(C).to('cuda', dtype)
    ge = pm.PsGELU()
    with torch.no_grad():
        ln.weight.copy_(gam), ln.bias.copy_(beta), ls.weight.copy_(lam)
    xm, rm = nchw(x).requires_grad_(True), nchw(res).requires_grad_(True)
    ln(xm).backward(nchw(dy))
    _, raw = _ln_raw(x, dy, gam, beta, dtype)
    assert same(rows(xm.grad), raw['dx']) and same(ln.weight.grad.cpu(), raw['dgamma'])
    assert same(ln.bias.grad.cpu(), raw['dbeta'])
    with torch.no_grad():
        assert same(rows(ln(xm)), raw['y'])
    xm.grad = None
    out = ls(xm, rm)
    out.backward(nchw(dy))
    _, raw = _ls_raw(x, res, dy, lam, dtype)
    assert same(rows(out.detach()), raw['out']) and same(rows(xm.grad), raw['dy'])
    assert same(ls.weight.grad.cpu(), raw['dlam']) and same(rm.grad, nchw(dy))
    xm.grad = None
    yg = ge(xm)
    yg.backward(nchw(dy))
    lib, tag, s = require_lib(), dtype_tag(dtype), current_stream_ptr()
    xd, dyd = _dev(x, dtype), _dev(dy, dtype)
    oy, od = _nan(M * C, dtype), _nan(M * C, dtype)
    lib.ps_gelu_fwd(xd.data_ptr(), oy.data_ptr(), M * C, tag, s)
    lib.ps_gelu_bwd(xd.data_ptr(), dyd.data_ptr(), od.data_ptr(), M * C, tag, s)
    assert same(rows(yg.detach()), oy.cpu()) and same(rows(xm.grad), od.cpu())
    # a dense view at an odd storage offset: the module realigns it
    odd = torch.cat([xd.reshape(-1)[:3], xd.reshape(-1)])[3:]
    assert odd.data_ptr() % 16 != 0 and same(ge(odd).cpu(), oy.cpu())
    assert [(m.kernel_calls, m.fallback_calls) for m in (ln, ls, ge)] == \
        [(2, 0), (1, 0), (2, 0)]


def test_convnext_block_matches_torch_ops(monkeypatch):
    """bf16 block on the kernels against the same block in f32 with
    PS_LN=0: within 3 % of the largest value, the standing bf16 tolerance."""
    from ps_pytorch_amd.models.convnext import ConvNeXtBlock
    torch.manual_seed(7)
    ref = ConvNeXtBlock(96, layer_scale_init=0.5).cuda()
    blk = ConvNeXtBlock(96, layer_scale_init=0.5).cuda()
    blk.load_state_dict(ref.state_dict())
    blk = blk.to(BF)
    x = torch.randn(2, 96, 8, 8, device='cuda').to(memory_format=torch.channels_last)
    dy = torch.randn_like(x)
    xb = x.to(BF).requires_grad_(True)
    ob = blk(xb)
    ob.backward(dy.to(BF))
    assert all(m.kernel_calls == 1 and m.fallback_calls == 0
               for m in (blk.norm, blk.act, blk.scale))
    monkeypatch.setenv('PS_LN', '0')
    xr = x.clone().requires_grad_(True)
    orf = ref(xr)
    orf.backward(dy)
    assert ref.norm.fallback_calls == 1
    pairs = [(ob.detach(), orf.detach()), (xb.grad, xr.grad)] + [
        (a.grad, b.grad) for a, b in zip(blk.parameters(), ref.parameters())]
    for got, want in pairs:
        err = (got.float() - want).abs().max().item()
        assert err <= 0.03 * want.abs().max().item(), (tuple(want.shape), err)


def test_trainer_convnext_tiny_runs_on_the_kernels():
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='convnext_tiny', dataset='Cifar10', batch_size=8,
                    lr=0.01, momentum=0.9, enable_gpu=True, seed=3)
    tr = NNTrainer(cfg, device=torch.device('cuda', 0))
    tr.build_model()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(8, 3, 32, 32, generator=gen).to('cuda', tr.compute_dtype)
    t = torch.randint(0, 10, (8,), generator=gen).to('cuda')
    losses = [tr.train_step(x, t) for _ in range(2)]
    assert all(math.isfinite(v) for v in losses), losses
    mods = [m for m in tr.network.modules() if isinstance(
        m, (pm.PsLayerNorm2d, pm.PsGELU, pm.PsLayerScaleAdd))]
    assert len(mods) == 18 * 3 + 5
    assert all((m.kernel_calls, m.fallback_calls) == (2, 0) for m in mods)
