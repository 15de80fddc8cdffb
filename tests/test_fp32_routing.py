"""CPU-side checks for the fp32 hand path: CPU tensors keep the torch route,
the support predicates only open for CUDA f32 / bf16, the gamma bound the
GPU tests rely on holds for torch's own f32 conv, and the new entry points
resolve in the built library."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from f32_ref import (CONV_SHAPES, assert_within, conv_bounds, conv_case,
                     conv_ref64, gamma)
from ps_pytorch_amd.ops import F32_SYMBOLS
from ps_pytorch_amd.ops import conv as ps_conv
from ps_pytorch_amd.ops import linear as ps_linear
from ps_pytorch_amd.ops import pool as ps_pool
from ps_pytorch_amd.ops.conv import PsConv2d, conv_with_passthrough
from ps_pytorch_amd.ops.linear import PsLinear
from ps_pytorch_amd.ops.loss import cross_entropy


def test_cpu_f32_keeps_torch_route(monkeypatch):
    """A CPU process never needs the native library: every Ps op must take
    its torch route (require_lib would be the only way onto the kernels)."""
    def boom():
        raise AssertionError("CPU f32 tensor was routed to the HIP kernels")
    for mod in (ps_conv, ps_linear, ps_pool):
        monkeypatch.setattr(mod, 'require_lib', boom)
    from ps_pytorch_amd.ops import loss as ps_loss
    monkeypatch.setattr(ps_loss, 'require_lib', boom)

    torch.manual_seed(0)
    x = torch.randn(2, 8, 6, 5, requires_grad=True)
    conv = PsConv2d(8, 16, 3, padding=1)
    y = conv(x)
    assert torch.equal(y, F.conv2d(x, conv.weight, conv.bias, padding=1))
    y2, xp = conv_with_passthrough(conv, x)
    assert torch.equal(y2, y) and xp is x
    pooled = ps_pool.max_pool2d(y, 2)
    assert torch.equal(pooled, F.max_pool2d(y, 2))
    g = ps_pool.global_avg_pool(pooled)
    assert torch.equal(g, F.adaptive_avg_pool2d(pooled, 1).flatten(1))
    lin = PsLinear(16, 10)
    logits = lin(g)
    assert torch.equal(logits, F.linear(g, lin.weight, lin.bias))
    t = torch.tensor([1, 7])
    loss = cross_entropy(logits, t)
    assert torch.equal(loss, F.cross_entropy(logits, t))
    loss.backward()
    assert x.grad is not None and conv.weight.grad is not None


class _FakeCuda:
    """Just enough tensor surface for the support predicates."""

    def __init__(self, dtype, shape=(2, 8, 6, 5), is_cuda=True):
        self.dtype, self.shape, self.is_cuda = dtype, shape, is_cuda

    def dim(self):
        return len(self.shape)


def _conv_ok(x, w):
    return ps_conv._supported(x, w, (1, 1), (1, 1), (1, 1), 1)


def test_support_predicates(monkeypatch):
    w32 = torch.zeros(16, 8, 3, 3)
    wbf = w32.bfloat16()
    # real CPU tensors: never
    assert not _conv_ok(torch.zeros(2, 8, 6, 5), w32)
    assert not ps_linear._supported(torch.zeros(2, 8), torch.zeros(4, 8))
    assert not ps_pool._supported(torch.zeros(2, 8, 6, 5))
    # CUDA-like tensors: f32 and bf16 yes, f16 / f64 no
    assert _conv_ok(_FakeCuda(torch.float32), w32)
    assert _conv_ok(_FakeCuda(torch.bfloat16), wbf)
    assert not _conv_ok(_FakeCuda(torch.float32, is_cuda=False), w32)
    for dt in (torch.float16, torch.float64):
        assert not _conv_ok(_FakeCuda(dt), w32.to(dt))
        assert not ps_pool._supported(_FakeCuda(dt))
        assert not ps_linear._supported(_FakeCuda(dt, (2, 8)),
                                        torch.zeros(4, 8, dtype=dt))
    assert not _conv_ok(_FakeCuda(torch.float32), wbf)   # mixed dtypes
    assert ps_pool._supported(_FakeCuda(torch.float32))
    assert ps_linear._supported(_FakeCuda(torch.float32, (2, 8)),
                                torch.zeros(4, 8))
    # envelope is unchanged for f32: stride 3, dilation, groups stay out
    x = _FakeCuda(torch.float32)
    assert not ps_conv._supported(x, w32, (3, 3), (1, 1), (1, 1), 1)
    assert not ps_conv._supported(x, w32, (1, 1), (1, 1), (2, 2), 1)
    assert not ps_conv._supported(x, w32, (1, 1), (1, 1), (1, 1), 2)
    # PS_F32 kill-switch closes f32 only; the per-op switches close both
    monkeypatch.setattr(ps_conv, '_F32', False)
    assert not _conv_ok(_FakeCuda(torch.float32), w32)
    assert not ps_pool._supported(_FakeCuda(torch.float32))
    assert not ps_linear._supported(_FakeCuda(torch.float32, (2, 8)),
                                    torch.zeros(4, 8))
    assert _conv_ok(_FakeCuda(torch.bfloat16), wbf)
    monkeypatch.setattr(ps_conv, '_F32', True)
    monkeypatch.setattr(ps_conv, '_ENABLED', False)
    assert not _conv_ok(_FakeCuda(torch.float32), w32)
    assert not _conv_ok(_FakeCuda(torch.bfloat16), wbf)


def test_wgrad_split_rule():
    f = ps_conv._wgrad_split_f32
    assert f(60, 16, 72) == 1                  # too short to split
    assert f(1024, 64, 576) == 16              # capped by M // 64
    assert f(1 << 20, 64, 576) == 512 // 9     # ~2 blocks/CU
    assert f(1 << 20, 8, 8) == 256             # hard cap
    assert f(1 << 20, 2048, 2048) == 1         # tiles alone fill the GPU


@pytest.mark.parametrize("shape", [CONV_SHAPES[2], CONV_SHAPES[6]])
def test_gamma_bound_holds_for_torch_f32_conv(shape):
    """Guards the GPU tests against a bound the reference implementation
    itself would break: torch's CPU f32 conv must sit inside it."""
    stride, pad = shape[6], shape[7]
    x, w, b, dout, _ = conv_case(shape, 'random')
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if b is not None else None
    out = F.conv2d(xr, wr, br, stride=stride, padding=pad)
    out.backward(dout)
    r_out, r_dx, r_dw, r_db = conv_ref64(x, w, b, dout, stride, pad)
    b_out, b_dx, b_dw, b_db = conv_bounds(shape, x, w, b, dout)
    assert_within(out, r_out, b_out, 'fwd')
    assert_within(xr.grad, r_dx, b_dx, 'dgrad')
    assert_within(wr.grad, r_dw, b_dw, 'wgrad')
    if b is not None:
        assert_within(br.grad, r_db, b_db, 'bias grad')
    # and a bf16-rounded input must break it, or the bound checks nothing
    out_bf = F.conv2d(x.bfloat16().float(), w, b, stride=stride, padding=pad)
    assert ((out_bf.double() - r_out).abs() > b_out).any()
    assert gamma(648 + 2) < 1e-4


def test_f32_symbols_resolve():
    import __graft_entry__
    from ps_pytorch_amd.ops import build as ops_build
    __graft_entry__.build()
    try:
        lib = ctypes.CDLL(str(ops_build.SO_PATH))
    except OSError as e:
        pytest.skip(f"native library cannot be loaded on this host: {e}")
    for sym in F32_SYMBOLS:
        assert hasattr(lib, sym), sym
