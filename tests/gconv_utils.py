"""Exact-integer cases for the grouped convolution kernels
(ops/kernels/conv_group.hip), on the lattice of tests/conv_lattice.py:
small-integer operands, float64 CPU references with groups=G, torch.equal.
One x, w, dy serve fwd, dgrad and wgrad, so each operand takes the
smallest amplitude its contractions allow (R*R*Cg for fwd and dgrad,
Nb*P*Q for wgrad)."""
import functools

import torch
import torch.nn.functional as F

import conv_lattice as cl

# (Nb, C, H, W, G, R, stride, pad): the smallest shapes at which each
# mechanism of the kernels can go wrong
CASES = [
    (3, 64, 7, 5, 16, 3, 1, 1),      # Cg 4, one slab, one partial row tile
    (2, 128, 9, 9, 16, 3, 1, 1),     # Cg 8, two slabs, tile tail
    (2, 192, 8, 8, 12, 3, 2, 1),     # Cg 16, three slabs, stride 2
    (2, 128, 9, 9, 8, 3, 2, 1),      # Cg 16, stride 2, odd H and W
    (2, 64, 9, 7, 2, 3, 1, 1),       # Cg 32
    (1, 128, 12, 12, 2, 3, 2, 1),    # Cg 64, stride 2
    (2, 64, 6, 6, 4, 1, 1, 0),       # 1x1: phantom half-step at SG 16
    (1, 64, 8, 8, 8, 5, 1, 2),       # 25 taps: odd pairing, pad 2
    (5, 128, 16, 16, 32, 3, 1, 1),   # M 1280: row tiles, wgrad split > 1
]
RAW_CASES = [CASES[1], CASES[2]]
SPLIT_CASE = CASES[8]
BIAS_CASE = CASES[1]


@functools.lru_cache(maxsize=None)
def gconv_case(case):
    """(x, w, b, dy, out, dx, dw), NCHW float64 on the CPU, built once and
    never modified; out is without the bias. Draw order x, w, b, dy."""
    Nb, C, H, W, G, R, stride, pad = case
    P, Q = cl.out_hw(H, W, R, stride, pad)
    fa = cl.amps(R * R * (C // G))              # fwd and dgrad
    wa = cl.amps(Nb * P * Q)                    # wgrad
    g = cl.gen('gconv', case)
    x = cl.ints((Nb, C, H, W), min(fa[0], wa[0]), g)
    w = cl.ints((C, C // G, R, R), fa[1], g)
    b = cl.ints((C,), 8, g)
    dy = cl.ints((Nb, C, P, Q), min(fa[0], wa[1]), g)
    out = F.conv2d(x, w, None, stride=stride, padding=pad, groups=G)
    dx = torch.nn.grad.conv2d_input(x.shape, w, dy, stride=stride,
                                    padding=pad, groups=G)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=stride,
                                     padding=pad, groups=G)
    return x, w, b, dy, out, dx, dw
