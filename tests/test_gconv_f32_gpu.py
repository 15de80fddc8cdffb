"""GPU tests of the f32 grouped convolution kernels
(ops/kernels/conv_group_f32.hip) against float64 CPU references: exact on
grid / integer inputs, the gamma(n) bound on random data, determinism and
routing."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import f32_ref
import gconv_f32_utils as gfu
import gconv_utils as gu
from ps_pytorch_amd.ops import conv as ps_conv
from ps_pytorch_amd.ops import current_stream_ptr, require_lib

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
GUARD = 256


def _fn(case, x, w, b, douts):
    """out and one (dx, dw, db) per upstream gradient, through
    _GroupConvF32Fn."""
    G, stride, pad = case[4], case[6], case[7]
    xd = x.cuda().contiguous(memory_format=_CL).requires_grad_(True)
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    out = ps_conv._GroupConvF32Fn.apply(xd, wd, bd, stride, pad, G)
    assert out.dtype == torch.float32
    res = [torch.autograd.grad(out, (xd, wd, bd), d.cuda(), retain_graph=True)
           for d in douts]
    return out.detach(), res


@pytest.mark.parametrize("case", gfu.CASES)
def test_exact_through_function(case):
    """Sums of multiples of 2**-8 under 2**24 units are exact in f32 in any
    order (asserted on the references), so the kernels must reproduce
    float64 bit for bit; a bf16 round trip, a wrong lane map, a dropped tap
    or a transposed weight cannot."""
    x, w, b, d_int, d_grid, out, dx, dw, db = gfu.exact_case(case)
    gfu.assert_in_range((out, dx, dw, db))
    got, (g_int, g_grid) = _fn(case, x, w, b, [d_int, d_grid])
    f32_ref.assert_exact(got, out, f"fwd {case}")
    f32_ref.assert_exact(g_grid[0], dx, f"dgrad {case}")
    f32_ref.assert_exact(g_int[1], dw, f"wgrad {case}")
    f32_ref.assert_exact(g_int[2], db, f"bias grad {case}")


def _guarded(n):
    whole = torch.full((n + 2 * GUARD,), float('nan'), device='cuda')
    return whole, whole[GUARD:GUARD + n]


def _check_guarded(whole, view, ref_nhwc, what):
    torch.cuda.synchronize()
    f32_ref.assert_exact(view.view(ref_nhwc.shape), ref_nhwc, what)
    n = view.numel()
    assert bool(torch.isnan(whole[:GUARD]).all()) and \
        bool(torch.isnan(whole[GUARD + n:]).all()), f"{what}: guard written"


@pytest.mark.parametrize("case", gu.RAW_CASES + [gu.CASES[0]])
def test_exact_raw_entry_points(case):
    """Outputs are slices of NaN-filled buffers with guard bands, the
    partials are NaN-filled and the split is forced to 2: unwritten
    elements and stray stores fail."""
    Nb, C, H, W, G, R, stride, pad = case
    P, Q = f32_ref.out_hw(H, W, R, stride, pad)
    x, w, b, d_int, d_grid, out, dx, dw, db = gfu.exact_case(case)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    xd, wd, di, dg = (nhwc(t).cuda() for t in (x, w, d_int, d_grid))
    lib, dims = require_lib(), (Nb, H, W, C, G, P, Q, R, stride, pad)
    strm = current_stream_ptr()
    whole, o = _guarded(out.numel())
    assert lib.ps_gconv_fwd_f32(xd.data_ptr(), wd.data_ptr(), 0,
                                o.data_ptr(), *dims, strm) == 0
    _check_guarded(whole, o, nhwc(out - b.double().view(1, -1, 1, 1)),
                   f"fwd {case}")
    whole, o = _guarded(dx.numel())
    assert lib.ps_gconv_dgrad_f32(dg.data_ptr(), wd.data_ptr(), o.data_ptr(),
                                  *dims, strm) == 0
    _check_guarded(whole, o, nhwc(dx), f"dgrad {case}")
    partial = torch.full((2 * dw.numel(),), float('nan'), device='cuda')
    whole, o = _guarded(dw.numel())
    assert lib.ps_gconv_wgrad_f32(di.data_ptr(), xd.data_ptr(),
                                  partial.data_ptr(), o.data_ptr(), *dims, 2,
                                  strm) == 0
    _check_guarded(whole, o, nhwc(dw), f"wgrad {case}")
    # outside the envelope: nonzero, nothing launched
    assert lib.ps_gconv_fwd_f32(xd.data_ptr(), wd.data_ptr(), 0, o.data_ptr(),
                                Nb, H, W, C, C // 2, P, Q, R, stride, pad,
                                strm) != 0


@pytest.mark.parametrize("case", [gu.CASES[i] for i in (0, 1, 3, 4, 5)])
def test_random_data_within_gamma_bound(case):
    """One case per Cg (4, 8, 16, 32, 64): |err| <= gamma(n + 2) * sum|a b|,
    n the contraction length."""
    Nb, C, H, W, G, R, stride, pad = case
    P, Q = f32_ref.out_hw(H, W, R, stride, pad)
    g = f32_ref.gen(1700 + C + G)
    x, w, b, dy = (torch.randn(s, generator=g) for s in (
        (Nb, C, H, W), (C, C // G, R, R), (C,), (Nb, C, P, Q)))
    got, ((dx, dw, db),) = _fn(case, x, w, b, [dy])
    refs = gfu.ref64(case, x, w, b, dy)
    mags = gfu.ref64(case, x.abs(), w.abs(), b.abs(), dy.abs())
    ns = (R * R * (C // G), R * R * (C // G), Nb * P * Q, Nb * P * Q)
    for name, a, r, m, n in zip(("fwd", "dgrad", "wgrad", "bias grad"),
                                (got, dx, dw, db), refs, mags, ns):
        f32_ref.assert_within(a, r, f32_ref.gamma(n + 2) * m,
                              f"{name} {case}")


def test_backward_bit_identical_across_runs():
    case = gu.SPLIT_CASE
    Nb, C, H, W, G, R, stride, pad = case
    assert ps_conv._gconv_wgrad_split_f32(Nb * H * W, C, R, C // G) > 1
    g = f32_ref.gen(1800)
    x, w, b, dy = (torch.randn(s, generator=g) for s in (
        (Nb, C, H, W), (C, C // G, R, R), (C,), (Nb, C, H, W)))
    _, (a, c) = _fn(case, x, w, b, [dy, dy])
    _, (d,) = _fn(case, x, w, b, [dy])
    for u, v, z in zip(a, c, d):
        assert torch.equal(u, v) and torch.equal(u, z)


def test_psconv2d_routes_f32_grouped_to_the_hand_path(monkeypatch):
    torch.manual_seed(5)
    conv = ps_conv.PsConv2d(128, 128, 3, padding=1, groups=32).to('cuda')
    x = torch.randn(2, 128, 9, 9, device='cuda').contiguous(memory_format=_CL)
    calls = []
    real = ps_conv._GroupConvF32Fn.apply
    monkeypatch.setattr(ps_conv._GroupConvF32Fn, 'apply',
                        lambda *a: calls.append(1) or real(*a))
    out = conv(x)
    assert calls == [1]
    xw = x.double().cpu(), conv.weight.detach().double().cpu(), \
        conv.bias.detach().double().cpu()
    ref = F.conv2d(*xw, padding=1, groups=32)
    mag = F.conv2d(*(t.abs() for t in xw), padding=1, groups=32)
    f32_ref.assert_within(out, ref, f32_ref.gamma(36 + 2) * mag, "routed fwd")
    for switch in ('_GCONV', '_F32'):
        with monkeypatch.context() as m:
            m.setattr(ps_conv, switch, False)
            off = conv(x)
        assert calls == [1]
        assert torch.equal(off, F.conv2d(x, conv.weight, conv.bias,
                                         padding=1, groups=32))


def test_resnext29_fp32_trainer_steps():
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='resnext29_32x4d', dataset='Cifar10',
                    batch_size=32, lr=0.02, momentum=0.9, enable_gpu=True,
                    compute_dtype='fp32')
    tr = NNTrainer(cfg, device=torch.device('cuda', 0))
    tr.build_model()
    assert tr.compute_dtype == torch.float32
    torch.manual_seed(13)
    x = torch.randn(32, 3, 32, 32, device='cuda')
    y = torch.randint(0, 10, (32,), device='cuda')
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        losses = [tr.train_step(x, y) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(l == l and abs(l) != float('inf') for l in losses), losses
    assert not [r for r in rec if 'outside flat_g' in str(r.message)]
    grouped = [m for m in tr.network.modules()
               if isinstance(m, ps_conv.PsConv2d) and m.groups > 1]
    assert len(grouped) == 9
    for m in grouped:
        pid = next(i for i, p in enumerate(tr.flat.params) if p is m.weight)
        assert m.weight.grad.data_ptr() == tr.flat._gptrs[pid]
        assert bool(m.weight.grad.any())
