"""GPU tests of the fused GroupNorm kernels (ops/kernels/groupnorm.hip)
through the raw entry points ps_gn_fwd / ps_gn_bwd and through
PsGroupNorm2d, against the float64 reference of tests/gn_utils.py and the
bounds of tests/bn_utils.py. Outputs are slices of NaN-filled buffers with
guard bands (0xA5 for mask bytes); inputs are compared with their originals.

On the lattice every sum of x, x^2, d and gamma * s_c is exact in f32 in any
order, so save_mean must equal the float64 quotient rounded to f32 and dbeta
the exact sum rounded once. y, invstd and the mask band take bn_utils'
forward bounds unchanged. The backward reference uses the kernel's own saved
mean, invstd and mask; its bounds are gamma(k) times the same formula with
absolute values, k the longest chain of roundings in groupnorm.hip:
  dgamma: 3 per term (xc, xc * invstd, d * that) + HW - 1 adds per sample
          + N - 1 adds of the parameter fold          -> k = HW + N + 1
  dx:     t_c (HW + 2), * gamma, Cg - 1 adds of B (HW + Cg + 2), invstd^2,
          * B, / m (HW + Cg + 5), xc and b * xc (HW + Cg + 7), the two adds
          of a * d + b * xc + k (contraction only removes roundings)
                                                      -> k = HW + Cg + 9
then one rounding to the io type (2^-8 of the value in bf16).
"""
import pytest
import torch

import bn_utils as bu
import conv_lattice as cl
import gn_utils as gu
from f32_ref import gamma as g
from ps_pytorch_amd.ops import current_stream_ptr, dtype_tag, require_lib
from ps_pytorch_amd.ops.modules import PsGroupNorm2d

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
BY_NAME = dict(zip(gu.CASE_IDS, gu.CASES))


def _guarded(n, dtype):
    fill = 0xA5 if dtype == torch.uint8 else float('nan')
    whole = torch.full((n + 2 * cl.GUARD,), fill, dtype=dtype, device='cuda')
    return whole, whole[cl.GUARD:cl.GUARD + n]


def _bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(
        torch.int16 if t.dtype == BF else torch.int32)


def _run(case, dtype):
    """ps_gn_fwd + ps_gn_bwd of one table row on guarded buffers, with the
    plan and the workspaces of _FusedGNFn. Returns CPU copies of every
    output; asserts guard bands intact and inputs unchanged."""
    _, N, HW, C, G, relu, _ = case
    lib, tag, strm = require_lib(), dtype_tag(dtype), current_stream_ptr()
    names = ('x', 'res', 'dy', 'gamma', 'beta')
    ins = {k: v.to(dtype).cuda() for k, v in zip(names, gu.gn_case(case))
           if v is not None}
    keep = {k: v.clone() for k, v in ins.items()}
    elt = ins['x'].element_size()
    slab_f, slab_b = gu.plans(case, elt)
    nws = lib.ps_gn_ws_floats(N, HW, C, G)
    sizes = {'y': (N * HW * C, dtype), 'dx': (N * HW * C, dtype),
             'dgamma': (C, dtype), 'dbeta': (C, dtype),
             'mean': (N * G, F32), 'invstd': (N * G, F32),
             'partial': (N * 2 * C, F32), 'ws_f': (nws, F32), 'ws_b': (nws, F32)}
    if relu:
        sizes['mask'] = (N * HW * C // 8, torch.uint8)
    if 'res' in ins:
        sizes['dres'] = (N * HW * C, dtype)
    bufs = {k: _guarded(*v) for k, v in sizes.items()}
    p = lambda k: bufs[k][1].data_ptr() if k in bufs else 0
    q = lambda k: ins[k].data_ptr() if k in ins else 0
    rc = lib.ps_gn_fwd(q('x'), p('y'), q('gamma'), q('beta'), q('res'),
                       p('mask'), p('mean'), p('invstd'),
                       0 if slab_f else p('ws_f'), N, HW, C, G, bu.EPS,
                       relu, slab_f, tag, strm)
    assert rc == 0
    rc = lib.ps_gn_bwd(q('x'), p('mask'), q('dy'), q('gamma'), p('mean'),
                       p('invstd'), p('dx'), p('dgamma'), p('dbeta'),
                       p('dres'), p('partial'), 0 if slab_b else p('ws_b'),
                       N, HW, C, G, relu, slab_b, tag, strm)
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    for k, (whole, view) in bufs.items():
        n = view.numel()
        for band in (whole[:cl.GUARD], whole[cl.GUARD + n:]):
            ok = (band == 0xA5).all() if whole.dtype == torch.uint8 \
                else torch.isnan(band).all()
            assert bool(ok), f"{k}: guard band written"
        out[k] = view.cpu()
    for k, v in ins.items():
        assert torch.equal(_bits(v), _bits(keep[k])), f"input {k} changed"
    return out


@DTYPES
@pytest.mark.parametrize("case", gu.CASES, ids=gu.CASE_IDS)
def test_case_table(case, dtype):
    _, N, HW, C, G, relu, has_res = case
    Cg, bf = C // G, dtype == BF
    x, res, dy, gam, beta = gu.gn_case(case)
    got = _run(case, dtype)
    mask = bu.unpack_mask(got['mask'], N * HW, C).view(N, HW, C) if relu else None
    y, dx = got['y'].view(N, HW, C), got['dx'].view(N, HW, C)
    s_sum, t_sum, t_abs = (torch.zeros(C, dtype=F64) for _ in range(3))
    for n, (o, fb) in enumerate(gu.fwd_ref(case)):
        tag = f"{case[0]} n={n}"
        per_group = lambda t: t.view(G, Cg)[:, 0]
        bu.check_exact(got['mean'].view(N, G)[n],
                       bu.once(per_group(o['mean']), F32), f"{tag} save_mean")
        bu.check_within(got['invstd'].view(N, G)[n], per_group(o['invstd']),
                        per_group(fb['invstd']), f"{tag} save_invstd")
        bu.check_within(y[n], o['y'], bu.io_bound(fb['v'], o['y'], bf), f"{tag} y")
        if relu:
            bad = (mask[n] != o['mask']) & ~bu.undecided(o, fb)
            assert not bad.any(), f"{tag}: {int(bad.sum())} decided bits wrong"
        # backward from the kernel's own statistics and mask
        kmean = got['mean'].view(N, G)[n].to(F64).repeat_interleave(Cg)
        kinv = got['invstd'].view(N, G)[n].to(F64).repeat_interleave(Cg)
        r = gu.ref_bwd_sample(x[n], dy[n], gam, kmean, kinv,
                              mask[n] if relu else None, G)
        bu.check_within(dx[n], r['dx'],
                        bu.io_bound(g(HW + Cg + 9) * r['dx_abs'], r['dx'], bf),
                        f"{tag} dx")
        if has_res:
            bu.check_exact(got['dres'].view(N, HW, C)[n], r['d'], f"{tag} dres")
        part = got['partial'].view(N, 2, C)[n].to(F64)
        bu.check_exact(part[0], r['s'], f"{tag} partial s_c")
        s_sum, t_sum, t_abs = s_sum + r['s'], t_sum + r['t'], t_abs + r['t_abs']
    bu.check_exact(got['dbeta'], bu.once(s_sum, dtype), f"{case[0]} dbeta")
    bu.check_within(got['dgamma'], t_sum,
                    bu.io_bound(g(HW + N + 1) * t_abs, t_sum, bf),
                    f"{case[0]} dgamma")


@DTYPES
@pytest.mark.parametrize("name", ['cg32_gl12', 'fwd_64B_first',
                                  'streamed_2chunks_1'])
def test_bit_identical_across_runs(name, dtype):
    a, b = _run(BY_NAME[name], dtype), _run(BY_NAME[name], dtype)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{name} {k}"


def _module(case, dtype):
    """PsGroupNorm2d on NCHW inputs that are contiguous in no layout."""
    _, N, HW, C, G, relu, _ = case
    x, res, dy, gam, beta = gu.gn_case(case)

    def nchw(t):
        wide = torch.zeros(N, C, HW, 2, dtype=dtype, device='cuda')
        v = wide[..., :1]
        v.copy_(t.to(dtype).view(N, HW, 1, C).permute(0, 3, 1, 2))
        return v

    m = PsGroupNorm2d(G, C, eps=bu.EPS, relu=bool(relu)).to('cuda', dtype)
    with torch.no_grad():
        m.weight.copy_(gam)
        m.bias.copy_(beta)
    xm = nchw(x).requires_grad_(True)
    rm = nchw(res).requires_grad_(True) if res is not None else None
    return m, xm, rm, nchw(dy)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1).contiguous().cpu()


@DTYPES
@pytest.mark.parametrize("name", ['cg32_gl12', 'fwd_64B_first',
                                  'streamed_2chunks_1'])
def test_module_equals_raw_entry_points(name, dtype):
    """Bit for bit, so test_case_table's verdict covers the module; also in
    eval() (same kernels) and, without grad, with no mask or statistics."""
    case = BY_NAME[name]
    raw = _run(case, dtype)
    m, xm, rm, dy = _module(case, dtype)
    y = m(xm, residual=rm)
    y.backward(dy)
    with torch.no_grad():
        y_eval = m.eval()(xm, residual=rm)
    torch.cuda.synchronize()
    assert (m.kernel_calls, m.fallback_calls) == (2, 0)
    got = {'y': y.detach(), 'dx': xm.grad}
    if rm is not None:
        got['dres'] = rm.grad
    for k, v in got.items():
        assert torch.equal(_bits(_rows(v)), _bits(raw[k])), f"{name} {k}"
    assert torch.equal(_bits(_rows(y_eval)), _bits(raw['y']))
    assert torch.equal(_bits(m.weight.grad.cpu()), _bits(raw['dgamma']))
    assert torch.equal(_bits(m.bias.grad.cpu()), _bits(raw['dbeta']))


def test_outside_envelope_is_rejected_and_falls_back():
    lib = require_lib()
    x = torch.zeros(2 * 4 * 24, device='cuda')
    p = x.data_ptr()
    # Cg = 1, Cg = 3, a slab that splits a group, a tile over the budget
    for C, G, HW, slab in ((8, 8, 4, 8), (24, 8, 4, 24), (64, 2, 4, 16),
                           (64, 32, 2048, 64)):
        assert lib.ps_gn_fwd(p, p, p, p, 0, 0, p, p, p, 1, HW, C, G, 1e-5, 0,
                             slab, 0, current_stream_ptr()) != 0
    m = PsGroupNorm2d(8, 8).cuda()
    m(torch.randn(2, 8, 3, 3, device='cuda'))
    assert (m.kernel_calls, m.fallback_calls) == (0, 1)


@DTYPES
def test_graph_replay_equals_eager(dtype):
    case = BY_NAME['cg32_gl12']
    m, xm, rm, dy = _module(case, dtype)

    def body():
        # detached: no autograd graph of an earlier run may stay alive, its
        # leaf nodes would keep the stream of that run and the engine would
        # sync the capture stream with it inside the capture
        y = m(xm, residual=rm)
        (dx,) = torch.autograd.grad(y, xm, dy)
        return y.detach(), dx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                 # eager, outside capture
            eager_y, eager_dx = body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gy, gdx = body()
    for _ in range(3):
        gy.zero_()
        gdx.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(gy), _bits(eager_y))
        assert torch.equal(_bits(gdx), _bits(eager_dx))


@pytest.mark.parametrize("compute_dtype", ['bf16', 'fp32'])
def test_trainer_resnet18_gn(compute_dtype):
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='resnet18_gn', dataset='Cifar10', batch_size=8,
                    lr=0.05, momentum=0.9, enable_gpu=True,
                    compute_dtype=compute_dtype, seed=3)
    tr = NNTrainer(cfg, device=torch.device('cuda', 0))
    tr.build_model()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(8, 3, 32, 32, generator=gen).to('cuda', tr.compute_dtype)
    t = torch.randint(0, 10, (8,), generator=gen).to('cuda')
    losses = [tr.train_step(x, t) for _ in range(3)]
    assert all(torch.isfinite(torch.tensor(losses))), losses
    norms = [m for m in tr.network.modules() if isinstance(m, PsGroupNorm2d)]
    assert len(norms) == 20
    assert all((m.kernel_calls, m.fallback_calls) == (3, 0) for m in norms)
