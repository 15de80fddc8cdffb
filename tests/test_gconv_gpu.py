"""GPU tests of the grouped convolution kernels (ops/kernels/conv_group.hip)
against float64 CPU references: exact (torch.equal) on the integer lattice
of tests/gconv_utils.py, 3 % of the reference's maximum on random data (the
bound of tests/test_conv_gpu.py)."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import conv_lattice as cl
import gconv_utils as gu
from ps_pytorch_amd.ops import conv as ps_conv
from ps_pytorch_amd.ops import current_stream_ptr, require_lib

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
BF = torch.bfloat16


def _dev(t):
    """float64 CPU integers -> bf16 on the GPU (exact)."""
    d = t.to('cuda', BF)
    assert torch.equal(d.double().cpu(), t)
    return d


def _fn(case, x, w, b, dy):
    """(out, dx, dw, db) through _GroupConvFn, as float64 on the CPU."""
    G, stride, pad = case[4], case[6], case[7]
    xd = x.contiguous(memory_format=_CL).requires_grad_(True)
    wd = w.clone().requires_grad_(True)
    bd = b.clone().requires_grad_(True) if b is not None else None
    out = ps_conv._GroupConvFn.apply(xd, wd, bd, stride, pad, G)
    out.backward(dy)
    torch.cuda.synchronize()
    return [t.double().cpu() if t is not None else None
            for t in (out, xd.grad, wd.grad, bd.grad if b is not None else None)]


def _same(got, ref, what):
    bad = (got != ref).nonzero()
    assert got.shape == ref.shape and len(bad) == 0, (
        f"{what}: {len(bad)} of {ref.numel()} differ; first at "
        f"{tuple(bad[0].tolist())}: got {got[tuple(bad[0])]:g}, "
        f"want {ref[tuple(bad[0])]:g}")


@pytest.mark.parametrize("case", gu.CASES)
def test_lattice_exact_through_function(case):
    x, w, b, dy, out, dx, dw = gu.gconv_case(case)
    bias = b if case == gu.BIAS_CASE else None
    got = _fn(case, _dev(x), _dev(w), _dev(bias) if bias is not None else None,
              _dev(dy))
    _same(got[0], out + b.view(1, -1, 1, 1) if bias is not None else out,
          f"fwd {case}")
    _same(got[1], dx, f"dgrad {case}")
    _same(got[2], dw, f"wgrad {case}")
    if bias is not None:
        _same(got[3], dy.sum((0, 2, 3)), f"bias grad {case}")


def _guarded(n):
    whole = torch.full((n + 2 * cl.GUARD,), cl.NAN_BITS, dtype=torch.int16,
                       device='cuda').view(BF)
    return whole, whole[cl.GUARD:cl.GUARD + n]


def _check_guarded(whole, view, ref_nhwc, what):
    torch.cuda.synchronize()
    got = view.double().cpu().view(ref_nhwc.shape)
    assert not torch.isnan(got).any(), f"{what}: elements never written"
    _same(got, ref_nhwc, what)
    bits, n = whole.view(torch.int16), view.numel()
    for band in (bits[:cl.GUARD], bits[cl.GUARD + n:]):
        assert bool((band == cl.NAN_BITS).all()), f"{what}: guard band written"


@pytest.mark.parametrize("case", gu.RAW_CASES)
def test_lattice_exact_raw_entry_points(case):
    """Outputs are slices of NaN-filled buffers with guard bands: unwritten
    elements and stray stores fail. dw holds the group blocks only."""
    Nb, C, H, W, G, R, stride, pad = case
    P, Q = cl.out_hw(H, W, R, stride, pad)
    x, w, b, dy, out, dx, dw = gu.gconv_case(case)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    xd, wd, dyd = (_dev(nhwc(t)) for t in (x, w, dy))
    lib, dims = require_lib(), (Nb, H, W, C, G, P, Q, R, stride, pad)
    sg = max(C // G, 16)
    wimg = torch.empty(C * R * R * sg, dtype=BF, device='cuda')
    whole, o = _guarded(out.numel())
    assert lib.ps_gconv_fwd(xd.data_ptr(), wd.data_ptr(), 0, o.data_ptr(),
                            wimg.data_ptr(), *dims, current_stream_ptr()) == 0
    _check_guarded(whole, o, nhwc(out), f"fwd {case}")
    whole, o = _guarded(dx.numel())
    assert lib.ps_gconv_dgrad(dyd.data_ptr(), wd.data_ptr(), o.data_ptr(),
                              wimg.data_ptr(), *dims,
                              current_stream_ptr()) == 0
    _check_guarded(whole, o, nhwc(dx), f"dgrad {case}")
    split = 2
    partial = torch.full((split * C * R * R * sg,), float('nan'),
                         dtype=torch.float32, device='cuda')
    whole, o = _guarded(dw.numel())
    assert lib.ps_gconv_wgrad(dyd.data_ptr(), xd.data_ptr(),
                              partial.data_ptr(), o.data_ptr(), *dims, split,
                              current_stream_ptr()) == 0
    _check_guarded(whole, o, nhwc(dw), f"wgrad {case}")
    # outside the envelope: nonzero, nothing launched
    assert lib.ps_gconv_fwd(xd.data_ptr(), wd.data_ptr(), 0, o.data_ptr(),
                            wimg.data_ptr(), Nb, H, W, C, C // 2, P, Q, R,
                            stride, pad, current_stream_ptr()) != 0


def _rel_err(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


@pytest.mark.parametrize("case", [gu.CASES[i] for i in (0, 1, 3, 4, 5)])
def test_random_data_within_bf16_bound(case):
    """One case per Cg (4, 8, 16, 32, 64), bias included."""
    Nb, C, H, W, G, R, stride, pad = case
    P, Q = cl.out_hw(H, W, R, stride, pad)
    g = cl.gen('gconv_random', case)
    x, w, b, dy = (torch.randn(s, generator=g).to(BF) for s in (
        (Nb, C, H, W), (C, C // G, R, R), (C,), (Nb, C, P, Q)))
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = F.conv2d(xr, wr, br, stride=stride, padding=pad, groups=G)
    ref.backward(dy.double())
    got = _fn(case, x.cuda(), w.cuda(), b.cuda(), dy.cuda())
    for name, a, r in zip(("fwd", "dgrad", "wgrad", "bias grad"), got,
                          (ref.detach(), xr.grad, wr.grad, br.grad)):
        err = _rel_err(a, r)
        print(f"{name} {case}: rel err {err:.4g}")
        assert err < 0.03, f"{name} {err}"


def test_backward_bit_identical_across_runs():
    x, w, b, dy, *_ = gu.gconv_case(gu.SPLIT_CASE)
    Nb, C, H, W, G, R, stride, pad = gu.SPLIT_CASE
    assert ps_conv._gconv_wgrad_split(Nb * H * W, C, R * R) > 1
    g = cl.gen('gconv_det', gu.SPLIT_CASE)
    xs, ws, dys = (torch.randn(t.shape, generator=g).to(BF).cuda()
                   for t in (x, w, dy))
    a = _fn(gu.SPLIT_CASE, xs, ws, None, dys)
    c = _fn(gu.SPLIT_CASE, xs, ws, None, dys)
    assert torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])


def test_psconv2d_routes_grouped_to_the_hand_path(monkeypatch):
    torch.manual_seed(5)
    conv = ps_conv.PsConv2d(128, 128, 3, padding=1, groups=32).to('cuda', BF)
    x = torch.randn(2, 128, 9, 9, device='cuda', dtype=BF) \
        .contiguous(memory_format=_CL)
    calls = []
    real = ps_conv._GroupConvFn.apply
    monkeypatch.setattr(ps_conv._GroupConvFn, 'apply',
                        lambda *a: calls.append(1) or real(*a))
    out = conv(x)
    assert calls == [1]
    ref = F.conv2d(x.double().cpu(), conv.weight.double().cpu(),
                   conv.bias.double().cpu(), padding=1, groups=32)
    assert _rel_err(out.double().cpu(), ref) < 0.03
    monkeypatch.setattr(ps_conv, '_GCONV', False)
    off = conv(x)
    assert calls == [1]
    assert torch.equal(off, F.conv2d(x, conv.weight, conv.bias, padding=1,
                                     groups=32))


def test_dw_and_db_land_in_the_flat_slices_exactly():
    """Steal mode: the kernels write dw (as [K][R][S][Cg]) and db straight
    into flat_g; the values there are the lattice reference."""
    from ps_pytorch_amd.parallel.flat import FlatSpace, prep_model
    case = gu.BIAS_CASE
    Nb, C, H, W, G, R, stride, pad = case
    x, w, b, dy, out, dx, dw = gu.gconv_case(case)
    conv = ps_conv.PsConv2d(C, C, R, stride=stride, padding=pad, groups=G)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    net = prep_model(torch.nn.Sequential(conv), torch.device('cuda', 0), BF)
    flat = FlatSpace(net)
    flat.attach_grads(steal=True)
    flat.zero_grads()
    net(_dev(x).contiguous(memory_format=_CL)).backward(_dev(dy))
    torch.cuda.synchronize()
    for pid, (p, off) in enumerate(zip(flat.params, flat.offsets)):
        assert p.grad.data_ptr() == flat._gptrs[pid]
        got = flat.flat_g[off:off + p.numel()].double().cpu()
        ref = dw.permute(0, 2, 3, 1) if p.dim() == 4 else dy.sum((0, 2, 3))
        _same(got.view(ref.shape), ref.contiguous(), f"flat slice {pid}")


def test_resnext29_trainer_steps():
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='resnext29_32x4d', dataset='Cifar10',
                    batch_size=32, lr=0.02, momentum=0.9, enable_gpu=True)
    tr = NNTrainer(cfg, device=torch.device('cuda', 0))
    tr.build_model()
    torch.manual_seed(13)
    x = torch.randn(32, 3, 32, 32, device='cuda', dtype=tr.compute_dtype)
    y = torch.randint(0, 10, (32,), device='cuda')
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        losses = [tr.train_step(x, y) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(l == l and abs(l) != float('inf') for l in losses), losses
    assert not [r for r in rec if 'outside flat_g' in str(r.message)]
    for pid, p in enumerate(tr.flat.params):
        assert p.grad is not None and p.grad.data_ptr() == tr.flat._gptrs[pid]
    grouped = [m for m in tr.network.modules()
               if isinstance(m, ps_conv.PsConv2d) and m.groups > 1]
    assert len(grouped) == 9
    assert all(bool(m.weight.grad.any()) for m in grouped)
