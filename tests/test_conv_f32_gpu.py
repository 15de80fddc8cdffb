"""Exact-f32 MFMA convolution family (ops/kernels/conv_f32.hip) against
float64 CPU references: exact equality on exactly-representable inputs, the
derivable gamma(n) rounding bound on random inputs, the fused residual carry,
run-to-run determinism and stream ordering."""
import pytest
import torch

from f32_ref import (CONV_SHAPES, assert_exact, assert_within, conv_bounds,
                     conv_case, conv_ref64, gen, grid, ints, out_hw)
from ps_pytorch_amd.ops.conv import _ConvCarryFn, _ConvFn

pytestmark = pytest.mark.gpu

_CL = torch.channels_last


def _dev(t, grad=False):
    if t is None:
        return None
    t = t.to('cuda')
    if t.dim() == 4:
        t = t.contiguous(memory_format=_CL)
    return t.requires_grad_(grad)


def _fwd_bwd(x, w, b, douts, stride, pad):
    """One forward, then one backward per upstream gradient.
    Returns out and a list of (dx, dw, db)."""
    xd, wd, bd = _dev(x, True), _dev(w, True), _dev(b, True)
    out = _ConvFn.apply(xd, wd, bd, stride, pad)
    assert out.dtype == torch.float32
    res = []
    for d in douts:
        for t in (xd, wd, bd):
            if t is not None:
                t.grad = None
        out.backward(_dev(d), retain_graph=True)
        res.append((xd.grad.clone(), wd.grad.clone(),
                    bd.grad.clone() if bd is not None else None))
    return out.detach(), res


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv_f32_exact(shape):
    """Every product and partial sum is representable in f32 (contraction
    lengths < 4096, magnitudes < 2**24 ulps), so an f32-fma kernel must
    reproduce float64 bit for bit; a bf16 round-trip, a dropped or doubled
    term or a transposed operand cannot."""
    stride, pad = shape[6], shape[7]
    x, w, b, d_int, d_grid = conv_case(shape, 'exact')
    out, (g_int, g_grid) = _fwd_bwd(x, w, b, [d_int, d_grid], stride, pad)

    r_out, _, r_dw, r_db = conv_ref64(x, w, b, d_int, stride, pad)
    assert_exact(out, r_out, 'fwd')
    assert_exact(g_int[1], r_dw, 'wgrad')
    if b is not None:
        assert_exact(g_int[2], r_db, 'bias grad')
    _, r_dx, _, _ = conv_ref64(x, w, b, d_grid, stride, pad)
    assert_exact(g_grid[0], r_dx, 'dgrad')


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv_f32_random_within_gamma_bound(shape):
    stride, pad = shape[6], shape[7]
    x, w, b, dout, _ = conv_case(shape, 'random')
    out, ((dx, dw, db),) = _fwd_bwd(x, w, b, [dout], stride, pad)
    r_out, r_dx, r_dw, r_db = conv_ref64(x, w, b, dout, stride, pad)
    b_out, b_dx, b_dw, b_db = conv_bounds(shape, x, w, b, dout)
    assert_within(out, r_out, b_out, 'fwd')
    assert_within(dx, r_dx, b_dx, 'dgrad')
    assert_within(dw, r_dw, b_dw, 'wgrad')
    if b is not None:
        assert_within(db, r_db, b_db, 'bias grad')


CARRY_SHAPES = [
    (2, 8, 6, 5, 16, 3, 1, 1, False),      # stride-1 3x3
    (3, 72, 7, 7, 24, 3, 2, 1, False),     # stride-2 3x3
    (4, 64, 8, 8, 128, 1, 2, 0, False),    # 1x1 s2: 3/4 of dx is carry alone
]


@pytest.mark.parametrize("shape", CARRY_SHAPES)
def test_conv_f32_carry_exact(shape):
    Nb, C, H, W, K, R, stride, pad, _ = shape
    P, Q = out_hw(H, W, R, stride, pad)
    g = gen(77 + C)
    x = grid((Nb, C, H, W), g)
    w = ints((K, C, R, R), g)
    dout = grid((Nb, K, P, Q), g)
    dcarry = grid((Nb, C, H, W), g)
    xd, wd = _dev(x, True), _dev(w, True)
    out, xp = _ConvCarryFn.apply(xd, wd, None, stride, pad)
    torch.autograd.backward([out, xp], [_dev(dout), _dev(dcarry)])
    _, r_dx, _, _ = conv_ref64(x, w, None, dout, stride, pad)
    assert_exact(xd.grad, r_dx + dcarry.double(), 'dgrad + carry')
    if R == 1 and stride == 2:
        # positions no output tap reaches carry dcarry alone
        assert torch.equal(xd.grad[:, :, 1::2, :].cpu(), dcarry[:, :, 1::2, :])


@pytest.mark.parametrize("shape", [CONV_SHAPES[1], CONV_SHAPES[6]])
def test_conv_f32_backward_deterministic(shape):
    stride, pad = shape[6], shape[7]
    x, w, b, dout, _ = conv_case(shape, 'random')
    _, (g1, g2) = _fwd_bwd(x, w, b, [dout, dout], stride, pad)
    _, (g3,) = _fwd_bwd(x, w, b, [dout], stride, pad)
    for a, c, d, name in zip(g1, g2, g3, ('dx', 'dw', 'db')):
        if a is None:
            continue
        assert torch.equal(a, c), name
        assert torch.equal(a, d), name


def test_conv_f32_honours_current_stream():
    shape = CONV_SHAPES[1]
    stride, pad = shape[6], shape[7]
    x, w, b, dout, _ = conv_case(shape, 'random')
    out0, ((dx0, dw0, _),) = _fwd_bwd(x, w, b, [dout], stride, pad)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out1, ((dx1, dw1, _),) = _fwd_bwd(x, w, b, [dout], stride, pad)
    side.synchronize()
    assert torch.equal(out0, out1)
    assert torch.equal(dx0, dx1)
    assert torch.equal(dw0, dw1)
