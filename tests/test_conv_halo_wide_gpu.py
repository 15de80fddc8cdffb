"""conv3x3_halo_wide_kernel (3x3 s1 p1 fwd / dgrad, a 128- or 256-channel
contraction, W in 16 / 8) through ps_conv_halo_wide_variant: variant 0 = the
generic conv_gemm_kernel<128,128>, variant 1 = the halo-resident wide kernel.

The wide kernel runs the generic kernel's step order (taps outside, chunks
inside, kk = 0, 1), so the two are BIT-IDENTICAL. The claims:
  * integer-lattice inputs (tests/conv_lattice.py generators): both variants
    equal the float64 reference under torch.equal, given |ref| <= RANGE,
    which the unmarked test below asserts on the reference alone;
  * random bf16 data: each variant within test_conv_gpu.py's 0.03 of a torch
    fp32 convolution, and variant 1 torch.equal to variant 0.
W = 4 and 512-channel contractions are not taken by the kernel (their
patches do not fit LDS in that order) and are checked as ineligible.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_lattice as cl
from ps_pytorch_amd.ops import current_stream_ptr, require_lib

gpu = pytest.mark.gpu
BF = torch.bfloat16

# (Nb, C, H, W, K)
SHAPES = [
    (1, 128, 8, 16, 128),       # W = 16: one tile, both image edges
    (1, 128, 16, 16, 128),      # two tiles
    (3, 128, 16, 16, 128),      # image boundaries between tiles
    (1, 128, 24, 16, 128),      # H not a power of two
    (1, 256, 16, 16, 128),      # more chunks than column tiles
    (2, 128, 8, 8, 128),        # W = 8: one tile holding two images
    (6, 128, 8, 8, 128),
    (2, 256, 8, 8, 256),
    (2, 128, 8, 8, 256),        # two column tiles (dgrad: four chunks)
]
# (dgrad, extra): extra = bias (fwd) or carry (dgrad) present
MODES = [(0, False), (0, True), (1, False), (1, True)]


def _fwd_row(shape):
    Nb, C, H, W, K = shape
    return (Nb, C, H, W, K, 3, 1, 1)


@functools.lru_cache(maxsize=None)
def _lattice(shape, dgrad, extra):
    """(src, weight, extra tensor or None, ref) as float64 NCHW on the CPU.
    fwd without bias: the biased case's operands, reference recomputed."""
    if dgrad:
        dy, w, cy, ref = cl.dgrad_case(_fwd_row(shape) + (int(extra),))
        return dy, w, cy, ref
    x, w, b, ref = cl.fwd_case(_fwd_row(shape))
    if not extra:
        b, ref = None, F.conv2d(x, w, None, padding=1)
    return x, w, b, ref


def test_lattice_references_within_range():
    """No GPU: the one condition of the exact tests, on the reference."""
    for shape in SHAPES:
        for dgrad, extra in MODES:
            ref = _lattice(shape, dgrad, extra)[3]
            assert float(ref.abs().max()) <= cl.RANGE, (shape, dgrad, extra)
            assert torch.equal(ref, ref.round())


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to('cuda', BF)


def _sentinel(*shape):
    return torch.full(shape, cl.NAN_BITS, dtype=torch.int16,
                      device='cuda').view(BF)


def _launch(shape, dgrad, src, w_kcrs, extra_t, variant):
    """src / extra_t NHWC bf16 on the device, w_kcrs [K, C, 3, 3] bf16."""
    Nb, C, H, W, K = shape
    wk = (w_kcrs.permute(2, 3, 1, 0) if dgrad          # wT [R, S, C, K]
          else w_kcrs.permute(0, 2, 3, 1)).contiguous()  # w  [K, R, S, C]
    dst = _sentinel(Nb, H, W, C if dgrad else K)
    ex = extra_t.data_ptr() if extra_t is not None else 0
    rc = require_lib().ps_conv_halo_wide_variant(
        dgrad, src.data_ptr(), wk.data_ptr(), 0 if dgrad else ex,
        dst.data_ptr(), ex if dgrad else 0,
        Nb, H, W, C, K, H, W, variant, current_stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return dst


@gpu
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_lattice_exact(shape, mode, variant):
    dgrad, extra = mode
    src, w, ex, ref = _lattice(shape, dgrad, extra)
    assert float(ref.abs().max()) <= cl.RANGE
    if ex is None:
        ext = None
    elif dgrad:
        ext = _nhwc(ex)
    else:
        ext = ex.to('cuda', BF)
    got = _launch(shape, dgrad, _nhwc(src), w.to('cuda', BF), ext, variant)
    assert not torch.isnan(got).any()           # every element written
    assert torch.equal(got.double().cpu(), ref.permute(0, 2, 3, 1))


def _rel_err(a, b):
    d = (a.float() - b.float()).abs().max()
    return float(d / b.float().abs().max().clamp_min(1e-6))


@functools.lru_cache(maxsize=None)
def _random(shape):
    """Random bf16 operands and the torch fp32 results, computed once."""
    Nb, C, H, W, K = shape
    g = torch.Generator().manual_seed(7 + 1000 * Nb + 10 * W + C + K)
    x = torch.randn(Nb, C, H, W, generator=g).to(BF)
    dy = torch.randn(Nb, K, H, W, generator=g).to(BF)
    w = torch.randn(K, C, 3, 3, generator=g).mul(0.05).to(BF)
    bias = torch.randn(K, generator=g).to(BF)
    carry = torch.randn(Nb, C, H, W, generator=g).to(BF)
    out = F.conv2d(x.float(), w.float(), bias.float(), padding=1)
    dx = torch.nn.grad.conv2d_input(x.shape, w.float(), dy.float(), padding=1)
    return x, dy, w, bias, carry, out, dx, dx + carry.float()


RANDOM_SHAPES = [(3, 128, 16, 16, 128), (1, 256, 16, 16, 128),
                 (6, 128, 8, 8, 128), (2, 256, 8, 8, 256)]


@gpu
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_random_data_against_torch_fp32_and_generic(shape):
    """Error measure and bound of tests/test_conv_gpu.py. Variant 0 (the
    existing kernel) goes through the same assertion; variant 1 must be
    bitwise equal to variant 0."""
    x, dy, w, bias, carry, out, dx, dxc = _random(shape)
    wd = w.to('cuda')
    runs = [('fwd+bias', 0, _nhwc(x), bias.to('cuda'), out),
            ('dgrad', 1, _nhwc(dy), None, dx),
            ('dgrad+carry', 1, _nhwc(dy), _nhwc(carry), dxc)]
    for what, dgrad, src, ex, ref in runs:
        ref = ref.permute(0, 2, 3, 1).to('cuda')
        got = [_launch(shape, dgrad, src, wd, ex, v) for v in (0, 1)]
        for v in (0, 1):
            err = _rel_err(got[v], ref)
            print(f"{what} variant {v} {shape}: {err}")
            assert err < 0.03, f"{what} variant {v}: {err}"
        assert not torch.isnan(got[1]).any()
        assert torch.equal(got[1], got[0]), f"{what} variant 1 against 0"


INELIGIBLE = [
    # Nb, H, W, C, K, P, Q
    (1, 8, 8, 128, 128, 8, 8),          # Nb 1 at W = 8: half a tile
    (2, 16, 16, 64, 128, 16, 16),       # C = 64
    (2, 16, 16, 128, 64, 16, 16),       # K = 64
    (2, 16, 16, 128, 128, 8, 8),        # stride 2 shows as P != H
    (2, 8, 32, 128, 128, 8, 32),        # W = 32
    (8, 4, 4, 128, 128, 4, 4),          # W = 4
    (2, 8, 8, 512, 512, 8, 8),          # eight chunks
    (2, 8, 8, 192, 192, 8, 8),          # three chunks, ragged column tile
]


@gpu
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dgrad", [0, 1])
@pytest.mark.parametrize("shape", INELIGIBLE)
def test_ineligible_shape_launches_nothing(shape, dgrad, variant):
    Nb, H, W, Cc, Kk, P, Q = shape
    big = Nb * H * W * max(Cc, Kk)
    src = torch.zeros(big, dtype=BF, device='cuda')
    w = torch.zeros(Kk * 9 * Cc, dtype=BF, device='cuda')
    dst = _sentinel(big)
    rc = require_lib().ps_conv_halo_wide_variant(
        dgrad, src.data_ptr(), w.data_ptr(), 0, dst.data_ptr(), 0,
        Nb, H, W, Cc, Kk, P, Q, variant, current_stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((dst.view(torch.int16) == cl.NAN_BITS).all())
