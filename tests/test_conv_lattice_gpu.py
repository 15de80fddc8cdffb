"""GPU half of the exact-integer oracle: every row of the tables in
tests/conv_lattice.py through the raw entry points of the library, compared
with torch.equal against the float64 reference. Integer operands make fp32
accumulation exact in any order, so a missing, duplicated or misplaced term
anywhere in a kernel changes at least one output element. Every output is a
slice of a NaN-filled buffer with guard bands: an unwritten element and a
store outside the tensor both fail."""
import pytest
import torch

import conv_lattice as cl
from ps_pytorch_amd.ops import current_stream_ptr, require_lib

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
BF = torch.bfloat16


def _dev(t):
    """float64 CPU integers -> bf16 on the GPU (exact)."""
    d = t.to('cuda', BF).contiguous()
    assert torch.equal(d.double().cpu(), t.contiguous())
    return d


def _nhwc(t):
    return _dev(t.permute(0, 2, 3, 1))


def _guarded(n, dtype=BF):
    """(whole, view): n elements with cl.GUARD sentinel elements on either
    side, all prefilled with NaN (bf16 0x7FC1, or f32 NaN)."""
    if dtype == BF:
        whole = torch.full((n + 2 * cl.GUARD,), cl.NAN_BITS,
                           dtype=torch.int16, device='cuda').view(BF)
    else:
        whole = torch.full((n + 2 * cl.GUARD,), float('nan'), dtype=dtype,
                           device='cuda')
    return whole, whole[cl.GUARD:cl.GUARD + n]


def _check(whole, view, ref_flat_order, what, index_names):
    """No NaN left, value-equal to the reference (so +0 and -0 agree),
    guard bands bit-for-bit untouched."""
    torch.cuda.synchronize()
    got = view.double().cpu().view(ref_flat_order.shape)
    assert not torch.isnan(got).any(), \
        f"{what}: {int(torch.isnan(got).sum())} elements never written"
    if not torch.equal(got, ref_flat_order):
        bad = (got != ref_flat_order).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(
            f"{what}: {len(bad)} of {got.numel()} elements differ; first at "
            f"{index_names} = {first}: got {got[first].item():g}, "
            f"want {ref_flat_order[first].item():g}")
    bits = whole.view(torch.int16)
    n = view.numel()
    for band in (bits[:cl.GUARD], bits[cl.GUARD + n:]):
        assert bool((band == cl.NAN_BITS).all()), f"{what}: guard band written"


def _run_fwd(case):
    Nb, C, H, W, K, R, stride, pad = case
    P, Q = cl.out_hw(H, W, R, stride, pad)
    x, w, b, ref = cl.fwd_case(case)
    xd, wd, bd = _nhwc(x), _nhwc(w), _dev(b)        # w[K, R, S, C]
    whole, out = _guarded(Nb * P * Q * K)
    require_lib().ps_conv_fwd(
        xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), 0,
        Nb, H, W, C, K, P, Q, R, R, stride, pad, current_stream_ptr())
    _check(whole, out, ref.permute(0, 2, 3, 1).contiguous(),
           f"fwd {case} [{cl.fwd_branch(*case)}]", "(n, p, q, k)")


def _run_dgrad(case):
    Nb, C, H, W, K, R, stride, pad, carry = case
    P, Q = cl.out_hw(H, W, R, stride, pad)
    dy, w, cy, ref = cl.dgrad_case(case)
    dyd = _nhwc(dy)
    wt = _dev(w.permute(2, 3, 1, 0))                # wT[R, S, C, K]
    cyd = _nhwc(cy) if carry else None
    whole, dx = _guarded(Nb * H * W * C)
    require_lib().ps_conv_dgrad(
        dyd.data_ptr(), wt.data_ptr(), dx.data_ptr(),
        cyd.data_ptr() if carry else 0,
        Nb, H, W, C, K, P, Q, R, R, stride, pad, current_stream_ptr())
    _check(whole, dx, ref.permute(0, 2, 3, 1).contiguous(),
           f"dgrad {case} [{cl.dgrad_branch(*case)}]", "(n, h, w, c)")


def _run_wgrad(case):
    Nb, C, H, W, K, R, stride, pad, split = case
    P, Q = cl.out_hw(H, W, R, stride, pad)
    x, dy, ref = cl.wgrad_case(case)
    xd, dyd = _nhwc(x), _nhwc(dy)
    n = K * R * R * C
    partial = torch.full((split * n,), float('nan'), dtype=torch.float32,
                         device='cuda')
    whole, dw = _guarded(n)
    require_lib().ps_conv_wgrad(
        dyd.data_ptr(), xd.data_ptr(), partial.data_ptr(), dw.data_ptr(),
        Nb, H, W, C, K, P, Q, R, R, stride, pad, split, current_stream_ptr())
    _check(whole, dw, ref.permute(0, 2, 3, 1).contiguous(),
           f"wgrad {case} [{cl.wgrad_branch(*case)}]", "(k, r, s, c)")


@pytest.mark.parametrize("case", cl.FWD_CASES)
def test_fwd_exact(case):
    _run_fwd(case)


@pytest.mark.parametrize("case", cl.FWD_RAW_ONLY)
def test_fwd_exact_raw_only(case):
    _run_fwd(case)


@pytest.mark.parametrize("case", cl.DGRAD_CASES)
def test_dgrad_exact(case):
    _run_dgrad(case)


@pytest.mark.parametrize("case", cl.DGRAD_RAW_ONLY)
def test_dgrad_exact_raw_only(case):
    _run_dgrad(case)


@pytest.mark.parametrize("case", cl.WGRAD_CASES)
def test_wgrad_exact(case):
    _run_wgrad(case)


@pytest.mark.parametrize("case", cl.WGRAD_RAW_ONLY)
def test_wgrad_exact_raw_only(case):
    _run_wgrad(case)


@pytest.mark.parametrize("case", cl.BIAS_CASES)
def test_bias_grad_exact(case):
    M, K = case
    dy, ref = cl.bias_case(case)
    dyd = _dev(dy)
    bpart = torch.full((512 * K,), float('nan'), dtype=torch.float32,
                       device='cuda')
    whole, db = _guarded(K)
    require_lib().ps_conv_bias_grad(db.data_ptr(), dyd.data_ptr(),
                                    bpart.data_ptr(), M, K,
                                    current_stream_ptr())
    _check(whole, db, ref, f"bias grad {case}", "(k,)")


def _bit_patterns(n, seed):
    """Random bf16 bit patterns (NaNs, infinities, denormals included):
    these kernels move bits, so they are compared as int16."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, (n,), generator=g,
                         dtype=torch.int32).to(torch.int16)


def _check_bits(whole, view, want, what):
    torch.cuda.synchronize()
    assert torch.equal(view.cpu(), want.reshape(-1)), what
    n = view.numel()
    for band in (whole[:cl.GUARD], whole[cl.GUARD + n:]):
        assert bool((band == cl.NAN_BITS).all()), f"{what}: guard band written"


def _guarded_bits(n):
    whole = torch.full((n + 2 * cl.GUARD,), cl.NAN_BITS, dtype=torch.int16,
                       device='cuda')
    return whole, whole[cl.GUARD:cl.GUARD + n]


@pytest.mark.parametrize("shape", [(50, 500), (64, 576), (10, 33), (33, 1)])
def test_wt_transpose_bitwise(shape):
    K, RSC = shape
    w = _bit_patterns(K * RSC, 100 * K + RSC).view(K, RSC)
    wd = w.cuda()
    whole, wt = _guarded_bits(K * RSC)
    require_lib().ps_wt_transpose(wt.data_ptr(), wd.data_ptr(), K, RSC,
                                  current_stream_ptr())
    _check_bits(whole, wt, w.t().contiguous(), f"wt_transpose {shape}")


@pytest.mark.parametrize("rows", [1, 1000])
@pytest.mark.parametrize("pad", [(20, 24), (3, 4), (1, 4), (50, 64),
                                 (500, 512), (10, 64)])
def test_padc_bitwise(pad, rows):
    C, CP = pad
    src = _bit_patterns(rows * C, 1000 * C + rows).view(rows, C)
    sd = src.cuda()
    whole, dst = _guarded_bits(rows * CP)
    require_lib().ps_padc(dst.data_ptr(), sd.data_ptr(), rows, C, CP,
                          current_stream_ptr())
    want = torch.zeros(rows, CP, dtype=torch.int16)
    want[:, :C] = src
    _check_bits(whole, dst, want, f"padc {pad} x {rows}")


def _exact(got, ref, what):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(
            f"{what}: {len(bad)} of {got.numel()} elements differ; first at "
            f"{first}: got {got[first].item():g}, want {ref[first].item():g}")


# conv1's input has no gradient, so only conv2 can take a carry
E2E_CONV_RUNS = [(cl.E2E_CONV[0], False), (cl.E2E_CONV[1], False),
                 (cl.E2E_CONV[1], True)]


@pytest.mark.parametrize(
    "case,carry", E2E_CONV_RUNS,
    ids=[c[0] + ('_carry' if cy else '') for c, cy in E2E_CONV_RUNS])
def test_conv_function_exact(case, carry):
    """_ConvFn / _ConvCarryFn on LeNet's two convolutions: channel padding
    (C = 1 -> 4, 20 -> 24), ragged-K padding of the backward (K = 20, 50 ->
    64) and the slices back, on the same integer inputs."""
    from ps_pytorch_amd.ops.conv import _ConvCarryFn, _ConvFn
    name, Nb, C, H, W, K, R, stride, pad, xgrad = case
    x, w, b, dy, out_r, dx_r, dw_r, db_r = cl.e2e_conv_case(case)
    xd = x.to('cuda', BF).contiguous(memory_format=_CL).requires_grad_(xgrad)
    wd = w.to('cuda', BF).contiguous(memory_format=_CL).requires_grad_(True)
    bd = b.to('cuda', BF).requires_grad_(True)
    dyd = dy.to('cuda', BF).contiguous(memory_format=_CL)
    if carry:
        cy = cl.ints(x.shape, 8, cl.gen('e2e_carry', case))
        out, xp = _ConvCarryFn.apply(xd, wd, bd, stride, pad)
        torch.autograd.backward([out, xp], [dyd, cy.to('cuda', BF)
                                            .contiguous(memory_format=_CL)])
        dx_r = dx_r + cy
    else:
        out = _ConvFn.apply(xd, wd, bd, stride, pad)
        out.backward(dyd)
    _exact(out, out_r, f"{name} out")
    _exact(wd.grad, dw_r, f"{name} dw")
    _exact(bd.grad, db_r, f"{name} db")
    if xgrad:
        _exact(xd.grad, dx_r, f"{name} dx")
    else:
        assert xd.grad is None


@pytest.mark.parametrize("case", cl.E2E_LINEAR)
def test_linear_function_exact(case):
    """_LinearFn on LeNet's fc layers (800 -> 500, 500 -> 10) at M = 70:
    ragged N padded to 64 for the backward and sliced back."""
    from ps_pytorch_amd.ops.linear import _LinearFn
    x, w, b, dy, out_r, dx_r, dw_r, db_r = cl.e2e_linear_case(case)
    xd = x.to('cuda', BF).requires_grad_(True)
    wd = w.to('cuda', BF).requires_grad_(True)
    bd = b.to('cuda', BF).requires_grad_(True)
    out = _LinearFn.apply(xd, wd, bd)
    out.backward(dy.to('cuda', BF))
    _exact(out, out_r, f"linear {case} out")
    _exact(xd.grad, dx_r, f"linear {case} dx")
    _exact(wd.grad, dw_r, f"linear {case} dw")
    _exact(bd.grad, db_r, f"linear {case} db")
