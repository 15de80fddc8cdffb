"""fp32 PsLinear (a 1x1 conv on the exact-f32 MFMA entry points), the f32
pooling kernels and the f32 fused softmax cross-entropy, against float64 /
plain-torch references."""
import pytest
import torch
import torch.nn.functional as F

from f32_ref import (assert_exact, assert_within, gamma, gen, grid, ints,
                     linear_ref64)
from ps_pytorch_amd.ops.linear import _LinearFn
from ps_pytorch_amd.ops.loss import cross_entropy
from ps_pytorch_amd.ops.pool import global_avg_pool, max_pool2d

pytestmark = pytest.mark.gpu

_CL = torch.channels_last

LINEAR_SHAPES = [(5, 800, 500), (64, 512, 10), (33, 20, 7)]   # M, K, N


def _lin(x, w, b, douts):
    xd = x.to('cuda').requires_grad_(True)
    wd = w.to('cuda').requires_grad_(True)
    bd = b.to('cuda').requires_grad_(True) if b is not None else None
    out = _LinearFn.apply(xd, wd, bd)
    res = []
    for d in douts:
        for t in (xd, wd, bd):
            if t is not None:
                t.grad = None
        out.backward(d.to('cuda'), retain_graph=True)
        res.append((xd.grad.clone(), wd.grad.clone(),
                    bd.grad.clone() if bd is not None else None))
    return out.detach(), res


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", LINEAR_SHAPES)
def test_linear_f32_exact(shape, bias):
    M, K, N = shape
    g = gen(M * 7 + N)
    x = grid((M, K), g)
    w = ints((N, K), g)
    b = ints((N,), g) if bias else None
    d_int, d_grid = ints((M, N), g), grid((M, N), g)
    out, (g_int, g_grid) = _lin(x, w, b, [d_int, d_grid])
    r_out, _, r_dw, r_db = linear_ref64(x, w, b, d_int)
    assert_exact(out, r_out, 'fwd')
    assert_exact(g_int[1], r_dw, 'wgrad')
    if bias:
        assert_exact(g_int[2], r_db, 'bias grad')
    _, r_dx, _, _ = linear_ref64(x, w, b, d_grid)
    assert_exact(g_grid[0], r_dx, 'dgrad')


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", LINEAR_SHAPES)
def test_linear_f32_random_within_gamma_bound(shape, bias):
    M, K, N = shape
    g = gen(M * 11 + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    dout = torch.randn(M, N, generator=g)
    out, ((dx, dw, db),) = _lin(x, w, b, [dout])
    r_out, r_dx, r_dw, r_db = linear_ref64(x, w, b, dout)
    a_out, a_dx, a_dw, a_db = linear_ref64(
        x.abs(), w.abs(), b.abs() if bias else None, dout.abs())
    assert_within(out, r_out, gamma(K + 2) * a_out, 'fwd')
    assert_within(dx, r_dx, gamma(N + 2) * a_dx, 'dgrad')
    assert_within(dw, r_dw, gamma(M + 2) * a_dw, 'wgrad')
    if bias:
        assert_within(db, r_db, gamma(M + 2) * a_db, 'bias grad')


# ---- max pool ----
MAXPOOL = [((2, 50, 8, 8), 2, 2, 0), ((2, 24, 9, 7), 3, 2, 1),
           ((3, 7, 5, 5), 2, 1, 0)]


@pytest.mark.parametrize("shape,k,s,p", MAXPOOL)
def test_maxpool_f32_matches_torch(shape, k, s, p):
    g = gen(sum(shape) + k)
    x = torch.randn(shape, generator=g)           # no ties
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, k, s, p)
    # upstream gradient on the 2**-8 grid: a pixel that wins several
    # overlapping windows sums their gradients, and grid values make that sum
    # exact in any order, so equality does not depend on torch's sum order
    dy = grid(yr.shape, g)
    yr.backward(dy)
    xd = x.to('cuda').contiguous(memory_format=_CL).requires_grad_(True)
    y = max_pool2d(xd, k, s, p)
    assert y.dtype == torch.float32
    y.backward(dy.to('cuda').contiguous(memory_format=_CL))
    assert torch.equal(y.detach().cpu(), yr.detach())
    assert torch.equal(xd.grad.cpu(), xr.grad)


# ---- global average pool ----
@pytest.mark.parametrize("shape", [(3, 512, 1, 1), (2, 50, 4, 4),
                                   (5, 64, 7, 3)])
def test_gavgpool_f32_within_gamma_bound(shape):
    Nb, C, H, W = shape
    HW = H * W
    g = gen(sum(shape))
    x = torch.randn(shape, generator=g)
    dy = torch.randn(Nb, C, generator=g)
    xd = x.to('cuda').contiguous(memory_format=_CL).requires_grad_(True)
    y = global_avg_pool(xd)
    assert y.dtype == torch.float32 and y.shape == (Nb, C)
    y.backward(dy.to('cuda'))
    x64 = x.double()
    r_y = x64.mean(dim=(2, 3))
    r_dx = (dy.double() / HW)[:, :, None, None].expand(shape)
    gm = gamma(HW + 1)
    assert_within(y, r_y, gm * x64.abs().mean(dim=(2, 3)), 'gavg fwd')
    assert_within(xd.grad, r_dx, gm * r_dx.abs(), 'gavg bwd')


# ---- softmax cross-entropy ----
def _ce_inputs(M, C, big):
    g = gen(M * 3 + C)
    x = torch.randn(M, C, generator=g)
    if big:   # logits near +-80: exp overflows f32 without max-subtraction
        x[:, 0::2] += 80.0
        x[:, 1::2] -= 80.0
    t = torch.randint(0, C, (M,), generator=g)
    return x, t


@pytest.mark.parametrize("M,C,big", [(7, 10, False), (1024, 10, False),
                                     (33, 1000, False), (4, 3, False),
                                     (33, 1000, True), (7, 10, True)])
def test_softmax_ce_f32_vs_float64(M, C, big):
    """exp/log are not correctly rounded, so the yardstick is measured: the
    kernel's max-abs error against float64 may be at most 4x that of torch's
    own fp32 CUDA F.cross_entropy on the same input (different exp/log and
    reduction order, each a few ulp)."""
    x, t = _ce_inputs(M, C, big)
    x64 = x.double().requires_grad_(True)
    l64 = F.cross_entropy(x64, t)
    l64.backward()

    xt = x.to('cuda').requires_grad_(True)
    lt = F.cross_entropy(xt, t.to('cuda'))
    lt.backward()

    xk = x.to('cuda').requires_grad_(True)
    lk = cross_entropy(xk, t.to('cuda'))
    assert lk.dtype == torch.float32
    lk.backward()

    assert torch.isfinite(lk) and torch.isfinite(xk.grad).all()
    e_loss_k = abs(float(lk.detach().double().cpu() - l64.detach()))
    e_loss_t = abs(float(lt.detach().double().cpu() - l64.detach()))
    e_grad_k = float((xk.grad.cpu().double() - x64.grad).abs().max())
    e_grad_t = float((xt.grad.cpu().double() - x64.grad).abs().max())
    msg = (f"M={M} C={C} big={big}: loss err kernel {e_loss_k:.3e} torch "
           f"{e_loss_t:.3e}; dlogits err kernel {e_grad_k:.3e} torch "
           f"{e_grad_t:.3e}")
    print(msg)
    assert e_loss_k <= 4 * e_loss_t, msg
    assert e_grad_k <= 4 * e_grad_t, msg
