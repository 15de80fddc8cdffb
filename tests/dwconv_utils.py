"""Exact-integer cases for the depthwise convolution kernels
(ops/kernels/conv_dw.hip), on the lattice of tests/conv_lattice.py:
small-integer operands (exact in bf16 and in f32), float64 CPU references
with groups=C, torch.equal. One x, w, dy serve fwd, dgrad and wgrad, so each
operand takes the smallest amplitude its contractions allow (R*R for fwd
and dgrad, Nb*P*Q for wgrad)."""
import functools

import torch
import torch.nn.functional as F

import conv_lattice as cl

# (Nb, C, H, W, R, stride, pad): the smallest shapes at which each
# mechanism of the kernels can go wrong
CASES = [
    (3, 8, 7, 5, 3, 1, 1),       # one granule, tile smaller than a block
    (2, 72, 9, 9, 3, 1, 1),      # full slab + 1-octet tail slab, tile tails
    (2, 32, 8, 8, 3, 2, 1),      # stride 2, the MobileNet first-block width
    (2, 136, 9, 7, 3, 2, 1),     # stride 2, odd H/W, three slabs with tail
    (1, 64, 12, 12, 5, 1, 2),    # R = 5, TR = 1 wgrad
    (2, 16, 11, 9, 5, 2, 2),     # R = 5 stride 2
    (1, 8, 10, 10, 7, 1, 3),     # R = 7
    (1, 24, 13, 13, 7, 2, 3),    # R = 7 stride 2, odd
    (2, 64, 6, 6, 3, 1, 0),      # pad 0 (P != H)
    (1, 8, 3, 40, 3, 1, 1),      # H below the tile height, W over 3 tiles
    (1, 8, 37, 3, 3, 2, 1),      # the transpose of that, stride 2
    (5, 128, 16, 16, 3, 1, 1),   # M = 1280: wgrad split > 1
    (2, 64, 33, 33, 3, 1, 1),    # tile count not dividing H or W, split > 1
]
RAW_CASES = [CASES[1], CASES[3]]
SPLIT_CASE = CASES[11]
BIAS_CASE = CASES[1]
RANDOM_CASES = [CASES[i] for i in (1, 3, 4, 5, 6, 7)]   # one per R x stride


@functools.lru_cache(maxsize=None)
def dwconv_case(case):
    """(x, w, b, dy, out, dx, dw), NCHW float64 on the CPU, built once and
    never modified; out is without the bias. Draw order x, w, b, dy."""
    Nb, C, H, W, R, stride, pad = case
    P, Q = cl.out_hw(H, W, R, stride, pad)
    fa = cl.amps(R * R)                         # fwd and dgrad
    wa = cl.amps(Nb * P * Q)                    # wgrad
    g = cl.gen('dwconv', case)
    x = cl.ints((Nb, C, H, W), min(fa[0], wa[0]), g)
    w = cl.ints((C, 1, R, R), fa[1], g)
    b = cl.ints((C,), 8, g)
    dy = cl.ints((Nb, C, P, Q), min(fa[0], wa[1]), g)
    out = F.conv2d(x, w, None, stride=stride, padding=pad, groups=C)
    dx = torch.nn.grad.conv2d_input(x.shape, w, dy, stride=stride,
                                    padding=pad, groups=C)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=stride,
                                     padding=pad, groups=C)
    return x, w, b, dy, out, dx, dw
