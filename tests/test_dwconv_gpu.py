"""GPU tests of the depthwise convolution kernels (ops/kernels/conv_dw.hip)
against float64 CPU references: exact (torch.equal) on the integer lattice
of tests/dwconv_utils.py in bf16 and f32; on random data 3 % of the
reference's maximum in bf16 (the bound of tests/test_conv_gpu.py) and the
elementwise gamma(n + 2) bound of tests/f32_ref.py in f32."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import conv_lattice as cl
import dwconv_utils as du
import f32_ref
from ps_pytorch_amd.ops import conv as ps_conv
from ps_pytorch_amd.ops import current_stream_ptr, dtype_tag, require_lib

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])


def _dev(t, dtype):
    """float64 CPU integers -> the storage type on the GPU (exact)."""
    d = t.to('cuda', dtype)
    assert torch.equal(d.double().cpu(), t)
    return d


def _fn(case, x, w, b, dy):
    """(out, dx, dw, db) through _DwConvFn, as float64 on the CPU."""
    stride, pad = case[5], case[6]
    xd = x.contiguous(memory_format=_CL).requires_grad_(True)
    wd = w.clone().requires_grad_(True)
    bd = b.clone().requires_grad_(True) if b is not None else None
    out = ps_conv._DwConvFn.apply(xd, wd, bd, stride, pad)
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


@DTYPES
@pytest.mark.parametrize("case", du.CASES)
def test_lattice_exact_through_function(case, dtype):
    x, w, b, dy, out, dx, dw = du.dwconv_case(case)
    bias = b if case == du.BIAS_CASE else None
    got = _fn(case, _dev(x, dtype), _dev(w, dtype),
              _dev(bias, dtype) if bias is not None else None, _dev(dy, dtype))
    _same(got[0], out + b.view(1, -1, 1, 1) if bias is not None else out,
          f"fwd {case}")
    _same(got[1], dx, f"dgrad {case}")
    _same(got[2], dw, f"wgrad {case}")
    if bias is not None:
        _same(got[3], dy.sum((0, 2, 3)), f"bias grad {case}")


def _guarded(n, dtype):
    whole = torch.full((n + 2 * cl.GUARD,), float('nan'), dtype=dtype,
                       device='cuda')
    return whole, whole[cl.GUARD:cl.GUARD + n]


def _check_guarded(whole, view, ref, what):
    torch.cuda.synchronize()
    got = view.double().cpu().view(ref.shape)
    assert not torch.isnan(got).any(), f"{what}: elements never written"
    _same(got, ref, what)
    n = view.numel()
    for band in (whole[:cl.GUARD], whole[cl.GUARD + n:]):
        assert bool(torch.isnan(band).all()), f"{what}: guard band written"


@DTYPES
@pytest.mark.parametrize("case", du.RAW_CASES)
def test_lattice_exact_raw_entry_points(case, dtype):
    """Outputs are slices of NaN-filled buffers with guard bands, the
    partial buffer is NaN-filled: unwritten elements and stray stores fail."""
    Nb, C, H, W, R, stride, pad = case
    P, Q = cl.out_hw(H, W, R, stride, pad)
    x, w, b, dy, out, dx, dw = du.dwconv_case(case)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    xd, wd, dyd = (_dev(nhwc(t), dtype) for t in (x, w, dy))
    lib, tag, strm = require_lib(), dtype_tag(dtype), current_stream_ptr()
    dims = (Nb, H, W, C, P, Q, R, stride, pad)
    whole, o = _guarded(out.numel(), dtype)
    assert lib.ps_dwconv_fwd(xd.data_ptr(), wd.data_ptr(), 0, o.data_ptr(),
                             *dims, tag, strm) == 0
    _check_guarded(whole, o, nhwc(out), f"fwd {case}")
    whole, o = _guarded(dx.numel(), dtype)
    assert lib.ps_dwconv_dgrad(dyd.data_ptr(), wd.data_ptr(), o.data_ptr(),
                               *dims, tag, strm) == 0
    _check_guarded(whole, o, nhwc(dx), f"dgrad {case}")
    split = 2
    partial = torch.full((split * R * R * C,), float('nan'), dtype=F32,
                         device='cuda')
    whole, o = _guarded(dw.numel(), dtype)
    assert lib.ps_dwconv_wgrad(dyd.data_ptr(), xd.data_ptr(),
                               partial.data_ptr(), o.data_ptr(), *dims, split,
                               tag, strm) == 0
    _check_guarded(whole, o, nhwc(dw), f"wgrad {case}")
    # outside the envelope: nonzero, nothing launched
    assert lib.ps_dwconv_fwd(xd.data_ptr(), wd.data_ptr(), 0, o.data_ptr(),
                             Nb, H, W, 12, P, Q, R, stride, pad, tag,
                             strm) != 0
    assert lib.ps_dwconv_fwd(xd.data_ptr(), wd.data_ptr(), 0, o.data_ptr(),
                             Nb, H, W, C, P, Q, 9, stride, pad, tag,
                             strm) != 0


@DTYPES
@pytest.mark.parametrize("case", du.RANDOM_CASES)
def test_random_data_within_bound(case, dtype):
    Nb, C, H, W, R, stride, pad = case
    P, Q = cl.out_hw(H, W, R, stride, pad)
    g = cl.gen('dwconv_random', case)
    x, w, b, dy = (torch.randn(s, generator=g).to(dtype) for s in (
        (Nb, C, H, W), (C, 1, R, R), (C,), (Nb, C, P, Q)))

    def ref64(x, w, b, dy):
        xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
        ref = F.conv2d(xr, wr, br, stride=stride, padding=pad, groups=C)
        ref.backward(dy.double())
        return ref.detach(), xr.grad, wr.grad, br.grad

    refs = ref64(x, w, b, dy)
    got = _fn(case, x.cuda(), w.cuda(), b.cuda(), dy.cuda())
    names = ("fwd", "dgrad", "wgrad", "bias grad")
    if dtype == BF:
        for name, a, r in zip(names, got, refs):
            err = float((a - r.detach()).abs().max()
                        / r.detach().abs().max().clamp_min(1e-6))
            print(f"{name} {case}: rel err {err:.4g}")
            assert err < 0.03, f"{name} {err}"
    else:
        M = Nb * P * Q
        mags = ref64(x.abs(), w.abs(), b.abs(), dy.abs())
        for name, a, r, m, n in zip(names, got, refs, mags,
                                    (R * R, R * R, M, M)):
            f32_ref.assert_within(a, r, f32_ref.gamma(n + 2) * m,
                                  f"{name} {case}")


@DTYPES
def test_backward_bit_identical_across_runs(dtype):
    x, w, b, dy, *_ = du.dwconv_case(du.SPLIT_CASE)
    Nb, C, H, W, R, stride, pad = du.SPLIT_CASE
    assert ps_conv._dwconv_wgrad_split(Nb * H * W, C, R,
                                       64 if dtype == BF else 32) > 1
    g = cl.gen('dwconv_det', du.SPLIT_CASE)
    xs, ws, dys = (torch.randn(t.shape, generator=g).to(dtype).cuda()
                   for t in (x, w, dy))
    a = _fn(du.SPLIT_CASE, xs, ws, None, dys)
    c = _fn(du.SPLIT_CASE, xs, ws, None, dys)
    assert torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])


@DTYPES
def test_psconv2d_routes_depthwise_to_the_hand_path(monkeypatch, dtype):
    torch.manual_seed(5)
    conv = ps_conv.PsConv2d(72, 72, 3, padding=1, groups=72).to('cuda', dtype)
    x = torch.randn(2, 72, 9, 9, device='cuda', dtype=dtype) \
        .contiguous(memory_format=_CL)
    calls = []
    real = ps_conv._DwConvFn.apply
    monkeypatch.setattr(ps_conv._DwConvFn, 'apply',
                        lambda *a: calls.append(1) or real(*a))
    out = conv(x)
    assert calls == [1]
    ref = F.conv2d(x.double().cpu(), conv.weight.double().cpu(),
                   conv.bias.double().cpu(), padding=1, groups=72)
    assert float((out.double().cpu() - ref).abs().max() / ref.abs().max()) \
        < (0.03 if dtype == BF else 1e-5)
    monkeypatch.setattr(ps_conv, '_DWCONV', False)
    off = conv(x)
    assert calls == [1]
    assert torch.equal(off, F.conv2d(x, conv.weight, conv.bias, padding=1,
                                     groups=72))


@DTYPES
def test_dw_and_db_land_in_the_flat_slices_exactly(dtype):
    """Steal mode: the kernels write dw (as [C][R*R]) and db straight into
    flat_g; the values there are the lattice reference."""
    from ps_pytorch_amd.parallel.flat import FlatSpace, prep_model
    case = du.BIAS_CASE
    Nb, C, H, W, R, stride, pad = case
    x, w, b, dy, out, dx, dw = du.dwconv_case(case)
    conv = ps_conv.PsConv2d(C, C, R, stride=stride, padding=pad, groups=C)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    net = prep_model(torch.nn.Sequential(conv), torch.device('cuda', 0), dtype)
    flat = FlatSpace(net)
    flat.attach_grads(steal=True)
    flat.zero_grads()
    net(_dev(x, dtype).contiguous(memory_format=_CL)).backward(_dev(dy, dtype))
    torch.cuda.synchronize()
    for pid, (p, off) in enumerate(zip(flat.params, flat.offsets)):
        assert p.grad.data_ptr() == flat._gptrs[pid]
        got = flat.flat_g[off:off + p.numel()].double().cpu()
        ref = dw if p.dim() == 4 else dy.sum((0, 2, 3))
        _same(got.view(ref.shape), ref.contiguous(), f"flat slice {pid}")


def _trainer():
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='mobilenet', dataset='Cifar10', batch_size=32,
                    lr=0.02, momentum=0.9, enable_gpu=True)
    tr = NNTrainer(cfg, device=torch.device('cuda', 0))
    tr.build_model()
    g = torch.Generator().manual_seed(13)
    x = torch.randn(32, 3, 32, 32, generator=g).to('cuda', tr.compute_dtype)
    y = torch.randint(0, 10, (32,), generator=g).cuda()
    return tr, x, y


def test_mobilenet_trainer_steps():
    tr, x, y = _trainer()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        losses = [tr.train_step(x, y) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(l == l and abs(l) != float('inf') for l in losses), losses
    assert not [r for r in rec if 'outside flat_g' in str(r.message)]
    for pid, p in enumerate(tr.flat.params):
        assert p.grad is not None and p.grad.data_ptr() == tr.flat._gptrs[pid]
    dws = [m for m in tr.network.modules()
           if isinstance(m, ps_conv.PsConv2d) and m.groups > 1]
    assert len(dws) == 13
    assert all(bool(m.weight.grad.any()) for m in dws)


def test_mobilenet_graph_steps_equal_eager():
    """enable_graph runs 3 eager warmup steps, so replays 1 and 2 are steps
    4 and 5 of an eager run from the same seed: the same loss, bit for bit
    (every kernel in the step has a fixed reduction order)."""
    torch.manual_seed(7)
    tr_e, x, y = _trainer()
    eager = [float(tr_e.train_step(x, y)) for _ in range(5)][3:]
    torch.manual_seed(7)
    tr_g, x2, y2 = _trainer()
    assert tr_g.enable_graph(x2, y2), "hipGraph capture failed"
    graph = [float(tr_g.graph_step(x2, y2)) for _ in range(2)]
    print("eager", eager, "graph", graph)
    assert graph == eager
