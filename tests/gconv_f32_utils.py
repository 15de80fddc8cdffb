"""Inputs and float64 references for the f32 grouped convolution kernels
(ops/kernels/conv_group_f32.hip)."""
import functools

import torch
import torch.nn.functional as F

import f32_ref
import gconv_utils as gu


# gconv_utils.CASES plus the two paths only the f32 kernels have
CASES = gu.CASES + [
    (2, 64, 9, 9, 16, 3, 2, 1),      # Cg 4, stride 2, odd H and W: direct
                                     # gather, parity-predicated dgrad
    (1, 128, 6, 7, 16, 2, 1, 0),     # Cg 8, 2x2: halo patch at R < 3, tap
                                     # rows in the wgrad grid
]


def ref64(case, x, w, b, dy):
    """(out, dx, dw, db) of the groups=G convolution in float64."""
    G, stride, pad = case[4], case[6], case[7]
    x, w, b = (t.double().requires_grad_(True) for t in (x, w, b))
    out = F.conv2d(x, w, b, stride=stride, padding=pad, groups=G)
    dx, dw, db = torch.autograd.grad(out, (x, w, b), dy.double())
    return out.detach(), dx, dw, db


@functools.lru_cache(maxsize=None)
def exact_case(case):
    """x on the 2**-8 grid, integer w and b, an integer dy (wgrad, bias
    gradient) and a grid dy (dgrad); then the references (out, dx, dw, db).
    Built once and never modified."""
    Nb, C, H, W, G, R, stride, pad = case
    P, Q = f32_ref.out_hw(H, W, R, stride, pad)
    g = f32_ref.gen(1600 + CASES.index(case))
    x = f32_ref.grid((Nb, C, H, W), g)
    w = f32_ref.ints((C, C // G, R, R), g)
    b = f32_ref.ints((C,), g)
    d_int = f32_ref.ints((Nb, C, P, Q), g)
    d_grid = f32_ref.grid((Nb, C, P, Q), g)
    out, _, dw, db = ref64(case, x, w, b, d_int)
    dx = ref64(case, x, w, b, d_grid)[1]
    return x, w, b, d_int, d_grid, out, dx, dw, db


def assert_in_range(refs):
    """Every reference value is under 2**24 units of 2**-8, so f32 sums of
    grid multiples are exact in any order."""
    for r in refs:
        assert float(r.abs().max()) * 256 < 2 ** 24
