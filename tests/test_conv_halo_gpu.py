"""Halo-resident 3x3 kernel (conv3x3_halo_kernel) against the generic
implicit-GEMM kernel it replaces on the 64 -> 64, stride-1 fwd / dgrad
shapes: outputs must be BIT-IDENTICAL (same MFMA, same tap and kk order per
accumulator, same f32 bias / carry add, one rounding), and must match a
torch fp32 convolution within the bound test_conv_gpu.py holds the bf16
kernels to. ps_conv_halo_variant launches one kernel alone (variant 0 =
conv_gemm_kernel, 1 = halo), so one process can compare them."""
import functools

import pytest
import torch
import torch.nn.functional as F

from ps_pytorch_amd.ops import current_stream_ptr, require_lib

gpu = pytest.mark.gpu

C = K = 64
NAN_BITS = 0x7FC1       # a bf16 NaN: an unwritten element fails torch.equal

# (Nb, H, W)
CASES = [
    (1, 4, 32),     # one tile, both image edges
    (5, 4, 32),     # consecutive tiles are different images
    (2, 8, 32),     # every tile touches exactly one edge
    (1, 32, 32),    # interior tiles
    (1, 64, 32),    # H != W
    (1, 8, 16),     # one tile at W = 16, both image edges
    (1, 16, 16),    # two tiles at W = 16
    (3, 16, 16),    # image boundaries at W = 16
    (1, 24, 16),    # H not a power of two
]
# (dgrad, extra): extra = bias (fwd) or carry (dgrad) present
MODES = [(0, False), (0, True), (1, False), (1, True)]


@functools.lru_cache(maxsize=None)
def _inputs(nb, H, W):
    g = torch.Generator().manual_seed(10000 * nb + 100 * H + W)
    src = torch.randn(nb, H, W, C, generator=g).to('cuda', torch.bfloat16)
    w = torch.randn(K, 3, 3, C, generator=g).mul(0.05) \
        .to('cuda', torch.bfloat16)                 # [K, R, S, C]
    wt = w.permute(1, 2, 3, 0).contiguous()         # [R, S, C, K]
    bias = torch.randn(K, generator=g).to('cuda', torch.bfloat16)
    carry = torch.randn(nb, H, W, C, generator=g).to('cuda', torch.bfloat16)
    return src.contiguous(), w.contiguous(), wt, bias, carry.contiguous()


def _sentinel(nb, H, W):
    return torch.full((nb, H, W, K), NAN_BITS, dtype=torch.int16,
                      device='cuda').view(torch.bfloat16)


def _run(nb, H, W, dgrad, extra, variant):
    lib = require_lib()
    src, w, wt, bias, carry = _inputs(nb, H, W)
    dst = _sentinel(nb, H, W)
    rc = lib.ps_conv_halo_variant(
        dgrad, src.data_ptr(), (wt if dgrad else w).data_ptr(),
        bias.data_ptr() if (extra and not dgrad) else 0, dst.data_ptr(),
        carry.data_ptr() if (extra and dgrad) else 0,
        nb, H, W, C, K, H, W, variant, current_stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return dst


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_halo_bit_identical_to_generic_kernel(case, mode):
    nb, H, W = case
    dgrad, extra = mode
    ref = _run(nb, H, W, dgrad, extra, 0)
    got = _run(nb, H, W, dgrad, extra, 1)
    assert not torch.isnan(ref).any()
    assert not torch.isnan(got).any()       # every element written
    assert torch.equal(got, ref)


def _rel_err(a, b):
    d = (a.float() - b.float()).abs().max()
    return float(d / b.float().abs().max().clamp_min(1e-6))


@gpu
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case", [(2, 8, 32), (3, 16, 16)])
def test_halo_matches_torch_fp32(case, variant):
    """Error measure and bound of tests/test_conv_gpu.py; variant 0 (the
    existing kernel) goes through the same assertion."""
    nb, H, W = case
    src, w, wt, bias, carry = _inputs(nb, H, W)
    wr = w.float().permute(0, 3, 1, 2).requires_grad_(False)    # [K,C,R,S]
    xr = src.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    outr = F.conv2d(xr, wr, bias.float(), padding=1)
    out = _run(nb, H, W, 0, True, variant)
    err = _rel_err(out, outr.detach().permute(0, 2, 3, 1))
    print(f"fwd variant {variant} {case}: {err}")
    assert err < 0.03, f"fwd {err}"
    # dgrad: `src` plays dout
    outr.backward(src.float().permute(0, 3, 1, 2))
    dxr = xr.grad.permute(0, 2, 3, 1)
    dx = _run(nb, H, W, 1, False, variant)
    err = _rel_err(dx, dxr)
    print(f"dgrad variant {variant} {case}: {err}")
    assert err < 0.03, f"dgrad {err}"
    dxc = _run(nb, H, W, 1, True, variant)
    err = _rel_err(dxc, dxr + carry.float())
    print(f"dgrad+carry variant {variant} {case}: {err}")
    assert err < 0.03, f"dgrad+carry {err}"


@gpu
@pytest.mark.parametrize("dgrad", [0, 1])
def test_halo_resident_blocks_repeatable(dgrad):
    """512 tiles: many blocks share a CU at 3 blocks/CU. Twenty runs, each
    bitwise equal to the one generic-kernel result (a screen of the counted
    waits and raw barriers, not a stress loop)."""
    nb, H, W = 64, 32, 32
    ref = _run(nb, H, W, dgrad, True, 0)
    for _ in range(20):
        assert torch.equal(_run(nb, H, W, dgrad, True, 1), ref)


INELIGIBLE = [
    # H, W, C, K, P, Q
    (32, 32, 128, 64, 32, 32),      # C = 128
    (32, 32, 64, 128, 32, 32),      # K = 128
    (16, 8, 64, 64, 16, 8),         # W = 8
    (4, 64, 64, 64, 4, 64),         # W = 64
    (6, 32, 64, 64, 6, 32),         # H = 6 at W = 32: ragged tile
    (32, 32, 64, 64, 16, 16),       # stride 2 shows as P != H
]


@gpu
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dgrad", [0, 1])
@pytest.mark.parametrize("shape", INELIGIBLE)
def test_ineligible_shape_launches_nothing(shape, dgrad, variant):
    H, W, Cc, Kk, P, Q = shape
    lib = require_lib()
    nb = 2
    # fwd reads [nb,H,W,C] and writes [nb,P,Q,K]; dgrad the reverse
    big = nb * H * W * max(Cc, Kk)
    src = torch.zeros(big, dtype=torch.bfloat16, device='cuda')
    w = torch.zeros(Kk * 9 * Cc, dtype=torch.bfloat16, device='cuda')
    dst = torch.full((big,), -7.0, dtype=torch.bfloat16, device='cuda')
    rc = lib.ps_conv_halo_variant(
        dgrad, src.data_ptr(), w.data_ptr(), 0, dst.data_ptr(), 0,
        nb, H, W, Cc, Kk, P, Q, variant, current_stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((dst == -7.0).all())


def test_psconv2d_eligible_shape_matches_torch(monkeypatch):
    """The Python-visible dispatch (PsConv2d fwd + bwd, default switches) on
    a halo-eligible shape against torch fp32. Runs on the CPU fallback when
    there is no GPU."""
    from ps_pytorch_amd.ops.conv import PsConv2d
    monkeypatch.delenv('PS_CONV_HALO', raising=False)
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    g = torch.Generator().manual_seed(11)
    conv = PsConv2d(64, 64, 3, stride=1, padding=1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(64, 64, 3, 3, generator=g) * 0.05)
    conv = conv.to(dev, torch.bfloat16).to(memory_format=torch.channels_last)
    x = torch.randn(2, 64, 8, 32, generator=g).to(dev, torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dout = torch.randn(2, 64, 8, 32, generator=g).to(dev, torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    out = conv(x)
    out.backward(dout)
    xr = x.detach().float().requires_grad_(True)
    wr = conv.weight.detach().float().requires_grad_(True)
    outr = F.conv2d(xr, wr, padding=1)
    outr.backward(dout.float())
    assert _rel_err(out.detach(), outr.detach()) < 0.03
    assert _rel_err(x.grad, xr.grad) < 0.03
    assert _rel_err(conv.weight.grad, wr.grad) < 0.03
