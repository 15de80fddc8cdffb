"""Exact-integer ("lattice") oracle for the bf16 conv / linear kernels of
ops/kernels/conv.hip: case tables, inputs, float64 references and Python
mirrors of the kernel dispatch.

All operands are small integers, which bf16 holds exactly. Every product and
every partial sum is then an integer far below 2**24, so fp32 accumulation
is exact IN ANY ORDER (per tap, per chunk, per split-K slab, through the
slab reduce), and so are the bias / carry adds. If the final value also
satisfies |v| <= 256 (integers up to 256 are bf16 values) its one rounding
to bf16 is exact too, and a kernel must reproduce the mathematically exact
convolution element for element: torch.equal, no tolerance. The only
condition is that range, and the reference alone decides it (RANGE below,
asserted for every case in test_conv_lattice.py, never clamped).

fwd_branch / dgrad_branch / wgrad_branch MUST mirror the dispatch in
conv.hip (the same convention as ops/conv.py's _wgrad_split):
  fwd_branch   - ps_conv_fwd -> conv_halo_eligible / conv_fwd_generic
                 (FWD_BODY)
  dgrad_branch - ps_conv_dgrad -> conv_halo_eligible / conv_dgrad_generic
                 (DG_BODY, the parity-class loop and DG2)
  wgrad_branch - ps_conv_wgrad (WGS, wgrad_row_eligible, WG_AL / WG_TK)
at the default switches (PS_GLDS, PS_SWZ, PS_CONV_HALO, PS_WG_RING unset).
A new dispatch branch in conv.hip comes with a name here and a row in the
tables; test_conv_lattice.py fails when a name has no row.
"""
import functools
import itertools
import math
import zlib

import torch
import torch.nn.functional as F

RANGE = 256             # |ref| <= RANGE: the final bf16 rounding is exact
GUARD = 256             # sentinel elements before and after every output
NAN_BITS = 0x7FC1       # a bf16 NaN, as in test_conv_halo_gpu.py

# ----------------------------------------------------------- case tables
# fwd: (Nb, C, H, W, K, R=S, stride, pad)
FWD_CASES = [
    (2, 4, 9, 7, 20, 3, 1, 1), (2, 4, 9, 7, 40, 3, 2, 1),
    (1, 4, 8, 8, 64, 3, 1, 1), (2, 4, 9, 7, 24, 3, 2, 1),
    (2, 4, 12, 12, 20, 5, 1, 0), (1, 4, 16, 16, 64, 7, 2, 3),
    (1, 4, 13, 11, 16, 5, 2, 2), (1, 4, 12, 12, 72, 5, 1, 2),
    (2, 24, 12, 12, 50, 5, 1, 0), (1, 8, 9, 7, 24, 3, 2, 1),
    (1, 16, 8, 8, 32, 3, 1, 1), (1, 40, 9, 9, 72, 3, 2, 1),
    (1, 80, 8, 8, 64, 3, 1, 1),
    (1, 64, 8, 8, 64, 1, 1, 0), (2, 64, 9, 7, 128, 1, 2, 0),
    (130, 20, 1, 1, 10, 1, 1, 0),
    (1, 128, 8, 8, 128, 3, 1, 1), (2, 64, 9, 9, 192, 3, 2, 1),
    (1, 128, 8, 8, 256, 1, 2, 0), (1, 88, 8, 8, 128, 3, 1, 1),
    (70, 200, 1, 1, 136, 1, 1, 0), (70, 100, 1, 1, 130, 1, 1, 0),
    (1, 88, 9, 9, 128, 3, 2, 1),
    (1, 64, 8, 8, 32, 3, 2, 1), (66, 128, 1, 1, 10, 1, 1, 0),
    (1, 100, 5, 5, 10, 1, 1, 0), (1, 64, 8, 8, 24, 3, 1, 1),
    (1, 100, 9, 9, 10, 1, 2, 0),
    (1, 128, 8, 8, 64, 3, 1, 1), (2, 64, 8, 8, 64, 3, 1, 1),
    (1, 88, 7, 9, 72, 3, 2, 1), (1, 64, 8, 8, 64, 5, 1, 2),
    (1, 128, 9, 7, 64, 3, 2, 1), (1, 100, 7, 7, 40, 1, 1, 0),
    (1, 64, 4, 32, 64, 3, 1, 1), (3, 64, 16, 16, 64, 3, 1, 1),   # halo
    # 1x1 one-step at stride 2 with C < 64: the one name of the mirror the
    # rows above leave out
    (1, 40, 9, 7, 24, 1, 2, 0),
]
# Reached only through the raw entry points (or PS_PADK=0): PsConv2d pads
# C <= 3 and ragged C < 64 to 4 or 8, _ConvFn.backward pads K % 8 != 0.
FWD_RAW_ONLY = [
    (2, 3, 8, 8, 64, 3, 1, 1), (2, 1, 12, 12, 20, 5, 1, 0),
    (1, 7, 9, 7, 33, 3, 2, 1), (1, 3, 16, 16, 64, 7, 2, 3),
    (1, 20, 9, 9, 50, 3, 1, 1), (1, 9, 7, 9, 24, 3, 2, 1),
]

# dgrad: (Nb, C, H, W, K, R=S, stride, pad, carry)
DGRAD_CASES = [
    (1, 128, 8, 8, 64, 3, 1, 1, 0), (1, 128, 8, 8, 64, 3, 1, 1, 1),
    (1, 24, 8, 8, 64, 3, 1, 1, 0), (1, 24, 8, 8, 64, 3, 1, 1, 1),
    (2, 20, 12, 12, 64, 5, 1, 0, 0), (70, 500, 1, 1, 64, 1, 1, 0, 0),
    (70, 100, 1, 1, 64, 1, 1, 0, 1),
    (1, 64, 8, 8, 64, 3, 1, 1, 0), (1, 64, 7, 9, 128, 1, 1, 0, 1),
    (2, 24, 12, 12, 56, 5, 1, 0, 0), (1, 8, 8, 8, 24, 3, 1, 1, 1),
    (1, 136, 8, 8, 24, 3, 1, 1, 0), (1, 130, 7, 7, 40, 1, 1, 0, 1),
    (1, 64, 8, 8, 24, 3, 1, 1, 1), (1, 40, 9, 7, 88, 3, 1, 1, 0),
    (1, 64, 4, 32, 64, 3, 1, 1, 0), (1, 64, 4, 32, 64, 3, 1, 1, 1),
    (3, 64, 16, 16, 64, 3, 1, 1, 0), (3, 64, 16, 16, 64, 3, 1, 1, 1),
    (1, 64, 8, 8, 128, 3, 2, 1, 0), (1, 64, 8, 8, 128, 3, 2, 1, 1),
    (1, 128, 9, 7, 128, 3, 2, 1, 0), (1, 128, 9, 7, 128, 3, 2, 1, 1),
    (2, 64, 8, 8, 128, 1, 2, 0, 0), (2, 64, 8, 8, 128, 1, 2, 0, 1),
    (1, 64, 7, 7, 128, 1, 2, 0, 1), (1, 128, 8, 8, 64, 1, 2, 0, 0),
    (1, 128, 7, 9, 64, 1, 2, 0, 1),
    (1, 24, 9, 9, 40, 3, 2, 1, 0), (1, 24, 9, 9, 40, 3, 2, 1, 1),
    (1, 64, 8, 8, 64, 5, 2, 2, 0),
    (1, 136, 9, 9, 40, 3, 2, 1, 0), (1, 136, 9, 9, 40, 3, 2, 1, 1),
    (1, 40, 7, 7, 24, 1, 2, 0, 0), (1, 40, 8, 8, 24, 1, 2, 0, 1),
    (1, 136, 8, 8, 24, 1, 2, 0, 0), (1, 136, 7, 7, 24, 1, 2, 0, 1),
    (2, 64, 1, 8, 64, 3, 2, 1, 0),      # H = 1: only hp = 0 classes exist
]
DGRAD_RAW_ONLY = [
    (2, 20, 12, 12, 50, 5, 1, 0, 0), (1, 3, 16, 16, 64, 7, 2, 3, 0),
]

# wgrad: (Nb, C, H, W, K, R=S, stride, pad, split)
WGRAD_CASES = [
    (2, 4, 8, 8, 64, 3, 1, 1, 2), (2, 4, 9, 7, 64, 3, 1, 1, 1),
    (2, 4, 16, 16, 64, 7, 2, 3, 2), (2, 4, 13, 11, 24, 5, 2, 2, 1),
    (2, 4, 12, 12, 24, 5, 1, 0, 2),
    (2, 24, 12, 12, 64, 5, 1, 0, 2), (2, 8, 9, 7, 24, 3, 2, 1, 1),
    (1, 40, 16, 16, 64, 3, 1, 1, 3), (2, 16, 16, 16, 64, 3, 2, 1, 2),
    (2, 24, 9, 9, 56, 3, 1, 1, 1),
    (1, 96, 8, 8, 64, 3, 1, 1, 1), (2, 64, 16, 16, 88, 3, 1, 1, 3),
    (1, 96, 32, 32, 64, 3, 1, 1, 5),
    (2, 64, 8, 8, 64, 3, 1, 1, 1), (4, 64, 8, 8, 64, 3, 1, 1, 3),
    (1, 128, 16, 16, 128, 3, 1, 1, 2),
    (2, 64, 4, 8, 64, 3, 1, 1, 1), (4, 64, 8, 4, 64, 3, 1, 1, 2),  # P != Q
    (16, 64, 2, 2, 64, 3, 1, 1, 1), (64, 64, 1, 1, 64, 3, 1, 1, 1),
    (8, 64, 6, 6, 64, 3, 1, 1, 3),
    (4, 128, 8, 8, 128, 1, 1, 0, 2), (130, 128, 1, 1, 128, 1, 1, 0, 2),
    (130, 200, 1, 1, 64, 1, 1, 0, 1), (130, 64, 1, 1, 200, 1, 1, 0, 2),
    (2, 64, 8, 8, 128, 3, 2, 1, 1), (2, 64, 9, 7, 64, 3, 2, 1, 1),
    (2, 64, 8, 8, 128, 1, 2, 0, 1), (1, 88, 9, 9, 72, 3, 2, 1, 1),
    (1, 64, 8, 8, 64, 5, 1, 2, 1),
    (2, 128, 7, 7, 128, 3, 1, 1, 1), (2, 88, 8, 8, 136, 1, 1, 0, 2),
    (2, 64, 9, 9, 128, 1, 2, 0, 1), (2, 88, 16, 16, 136, 3, 2, 1, 2),
    (2, 100, 6, 6, 24, 3, 1, 1, 1), (2, 64, 16, 16, 64, 1, 2, 0, 2),
    (2, 88, 6, 6, 136, 3, 1, 1, 1), (2, 88, 9, 9, 136, 3, 2, 1, 1),
    (2, 88, 8, 8, 72, 3, 2, 1, 1),
]
WGRAD_RAW_ONLY = [
    (2, 3, 8, 8, 64, 3, 1, 1, 2), (2, 1, 12, 12, 20, 5, 1, 0, 1),
    (1, 20, 9, 9, 64, 3, 1, 1, 1), (2, 3, 16, 16, 64, 7, 2, 3, 2),
    (2, 5, 9, 7, 64, 3, 2, 1, 1), (70, 100, 1, 1, 10, 1, 1, 0, 1),
]

# ps_conv_bias_grad: (M, K). 2100 and 2049 rows reach the 512-block cap of
# the launch; K = 10 and 50 take the ragged element loads. A block covers
# 4 * (256 // ceil(K / 8)) rows per pass, so in those rows only the first
# few blocks hold data: (2100, 2048) is the smallest shape at which every
# one of the 512 partial rows is non-trivial and the grid-stride loop takes
# a second pass (one row per pass-quarter at K = 2048).
BIAS_CASES = [(130, 64), (70, 10), (3, 24), (2100, 8), (2049, 50),
              (2100, 2048)]

# Seed salts for cases whose draw would leave RANGE (none needed so far):
# {(tag,) + case: salt}. The bound never moves; the draw does.
SALT = {}


def out_hw(H, W, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


# ------------------------------------------------------ dispatch mirrors
def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def _al(flag):
    return 'al' if flag else 'ragged'


def halo_eligible(C, H, W, K, R, stride, pad):
    """conv_halo_eligible (P == H and Q == W follow from 3x3 s1 p1)."""
    return (R == 3 and stride == 1 and pad == 1 and C == 64 and K == 64
            and W in (16, 32) and H > 0 and H % (128 // W) == 0)


def fwd_branch(Nb, C, H, W, K, R, stride, pad):
    if halo_eligible(C, H, W, K, R, stride, pad):
        return f'halo_w{W}'
    rs, rsc = R * R, R * R * C
    tn = 64
    if rs > 1 and C == 4 and rs * 4 <= 64:
        fam, tn = 'c4_nb1', (32 if K <= 32 else 64)
    elif rs > 1 and C == 4 and rs * 4 <= 256:
        fam, tn = 'c4_nb2', (32 if K <= 32 else 64)
    elif rs > 1 and C % 8 == 0 and C % 64 and rsc <= 768:
        fam, tn = 'c8', (32 if K <= 32 else 64)
    elif rs > 1 and rsc <= 64:
        fam = 'small_nb1'
    elif rs > 1 and rsc <= 192:
        fam = 'small_nb2'
    elif rs == 1 and C <= 64:
        fam = '1x1_onestep'
    else:
        fam, tn = 'gen', (128 if K >= 128 else 32 if K <= 32 else 64)
    return f'{fam}_tn{tn}_s{stride}_{_al(C % 64 == 0)}'


def dgrad_branch(Nb, C, H, W, K, R, stride, pad, carry):
    cy = 'carry' if carry else 'plain'
    if halo_eligible(C, H, W, K, R, stride, pad):
        return f'halo_w{W}_{cy}'
    al = _al(K % 64 == 0)           # the contraction runs over K
    if stride == 1:
        tn = 128 if C >= 128 else 32 if C <= 32 else 64
        return f's1_tn{tn}_{al}_{cy}'
    any_empty = False               # a parity class with no (r, s) tap
    for hp in range(min(2, H)):
        for wp in range(min(2, W)):
            r0, s0 = (hp + pad) & 1, (wp + pad) & 1
            if R <= r0 or R <= s0:
                any_empty = True
    tn = 128 if C >= 128 else 64
    return f"s2_tn{tn}_{al}_{cy}_{'seed' if any_empty else 'full'}"


def wgrad_branch(Nb, C, H, W, K, R, stride, pad, split):
    P, Q = out_hw(H, W, R, stride, pad)
    rs, rsc = R * R, R * R * C
    pw = 'pw' if _pow2(P * Q) and _pow2(Q) else 'magic'
    c8 = C % 8 == 0 and C % 64 != 0
    if rs > 1 and ((C == 4 and rs * 4 <= 256) or (c8 and rsc <= 768)
                   or rsc <= 192):
        cv = 4 if C == 4 else 8 if c8 else 0
        return f'small_cv{cv}_s{stride}_{pw}'
    if (stride == 1 and R == 3 and pad == 1 and _pow2(P) and _pow2(Q)
            and 4 <= Q <= 32):
        ring = C % 64 == 0 and K % 64 == 0
        return 'row_ring' if ring else 'row_reg_ragged'
    tk = 128 if K >= 128 else 64
    return f'gen_tk{tk}_s{stride}_{pw}_{_al(C % 64 == 0 and K % tk == 0)}'


def supported(Nb, C, H, W, K, R, stride, pad):
    """A shape the ops layer would send to the kernels (ops/conv.py
    _supported) with a non-empty output."""
    P, Q = out_hw(H, W, R, stride, pad)
    return R <= 7 and stride in (1, 2) and pad < R and P >= 1 and Q >= 1


@functools.lru_cache(maxsize=None)
def branch_universe():
    """Every name the three mirrors produce over a sweep of supported
    shapes wide enough to cross each threshold of the dispatch."""
    fwd, dg, wg = set(), set(), set()
    chans = sorted(set(range(1, 12)) | {16, 20, 21, 22, 24, 32, 33, 40, 48,
                                        56, 63, 64, 65, 72, 80, 88, 96, 100,
                                        128, 130, 136, 192, 200})
    ks = (8, 10, 24, 32, 33, 64, 72, 128, 136)
    hws = ((8, 8), (9, 7), (4, 32), (16, 16), (1, 8), (1, 1), (7, 7))
    for C, K, (H, W), (R, pad), stride in itertools.product(
            chans, ks, hws, ((1, 0), (3, 1), (5, 0), (5, 2), (7, 3)), (1, 2)):
        s = (1, C, H, W, K, R, stride, pad)
        if not supported(*s):
            continue
        fwd.add(fwd_branch(*s))
        for carry in (0, 1):
            dg.add(dgrad_branch(*s, carry))
        wg.add(wgrad_branch(*s, 1))
    return frozenset(fwd), frozenset(dg), frozenset(wg)


# -------------------------------------------------------------- inputs
def _var(a):
    return a * (a + 1) / 3.0        # variance of a uniform integer in [-a, a]


def amps(L):
    """Operand amplitudes for a contraction of length L: the largest pair
    whose 6-sigma sum stays under 224."""
    for a1, a2 in ((3, 3), (2, 2), (2, 1), (1, 1)):
        if 6.0 * math.sqrt(_var(a1) * _var(a2) * L) <= 224:
            return a1, a2
    return 1, 1


def fwd_len(case):
    return case[5] * case[5] * case[1]


def dgrad_len(case):
    K, R, stride = case[4], case[5], case[6]
    return R * R * K if stride == 1 else max(R * R * K // 4, K)


def wgrad_len(case):
    Nb, C, H, W, K, R, stride, pad = case[:8]
    P, Q = out_hw(H, W, R, stride, pad)
    return Nb * P * Q


def gen(tag, case):
    key = (tag,) + tuple(case)
    if key in SALT:
        key = key + (SALT[key],)
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(shape, a, g):
    return torch.randint(-a, a + 1, tuple(shape), generator=g).double()


@functools.lru_cache(maxsize=None)
def fwd_case(case):
    """(x, w, bias, ref): NCHW float64 on the CPU, built once, never
    modified. Draw order x, w, bias."""
    Nb, C, H, W, K, R, stride, pad = case
    a1, a2 = amps(fwd_len(case))
    g = gen('fwd', case)
    x = ints((Nb, C, H, W), a1, g)
    w = ints((K, C, R, R), a2, g)
    b = ints((K,), 8, g)
    return x, w, b, F.conv2d(x, w, b, stride=stride, padding=pad)


@functools.lru_cache(maxsize=None)
def dgrad_case(case):
    """(dy, w, carry | None, ref). Draw order dy, w, carry."""
    Nb, C, H, W, K, R, stride, pad, carry = case
    P, Q = out_hw(H, W, R, stride, pad)
    a1, a2 = amps(dgrad_len(case))
    g = gen('dgrad', case)
    dy = ints((Nb, K, P, Q), a1, g)
    w = ints((K, C, R, R), a2, g)
    cy = ints((Nb, C, H, W), 8, g) if carry else None
    ref = torch.nn.grad.conv2d_input((Nb, C, H, W), w, dy, stride=stride,
                                     padding=pad)
    return dy, w, cy, (ref + cy if carry else ref)


@functools.lru_cache(maxsize=None)
def wgrad_case(case):
    """(x, dy, ref). Draw order x, dy."""
    Nb, C, H, W, K, R, stride, pad, _ = case
    P, Q = out_hw(H, W, R, stride, pad)
    a1, a2 = amps(wgrad_len(case))
    g = gen('wgrad', case)
    x = ints((Nb, C, H, W), a1, g)
    dy = ints((Nb, K, P, Q), a2, g)
    ref = torch.nn.grad.conv2d_weight(x, (K, C, R, R), dy, stride=stride,
                                      padding=pad)
    return x, dy, ref


@functools.lru_cache(maxsize=None)
def bias_case(case):
    """(dy[M, K], ref[K])."""
    M, K = case
    dy = ints((M, K), 1 if M > 600 else 2, gen('bias', case))
    return dy, dy.sum(0)


# End-to-end cases through the autograd Functions (padding and slicing in
# ops/conv.py, ops/linear.py). One x, w, dy serve fwd, dgrad and wgrad, so
# each operand takes the smallest amplitude its contractions allow.
# (name, Nb, C, H, W, K, R, stride, pad, input needs grad)
E2E_CONV = [
    ('lenet_conv1', 4, 1, 28, 28, 20, 5, 1, 0, False),
    ('lenet_conv2', 4, 20, 12, 12, 50, 5, 1, 0, True),
]
# PsLinear 800 -> 500 -> 10 at M = 70, layer by layer: fc1's exact outputs
# (sigma about 33) as fc2's inputs would carry fc2's sums far out of RANGE,
# so each layer gets lattice inputs of its own. (M, in, out)
E2E_LINEAR = [(70, 800, 500), (70, 500, 10)]


@functools.lru_cache(maxsize=None)
def e2e_conv_case(case):
    """(x, w, b, dy, out, dx, dw, db), NCHW float64."""
    name, Nb, C, H, W, K, R, stride, pad, _ = case
    shp = (Nb, C, H, W, K, R, stride, pad)
    fa, da, wa = amps(fwd_len(shp)), amps(dgrad_len(shp)), amps(wgrad_len(shp))
    P, Q = out_hw(H, W, R, stride, pad)
    g = gen('e2e', case)
    x = ints((Nb, C, H, W), min(fa[0], wa[0]), g)
    w = ints((K, C, R, R), min(fa[1], da[1]), g)
    b = ints((K,), 8, g)
    dy = ints((Nb, K, P, Q), min(da[0], wa[1], 1 if Nb * P * Q > 600 else 2),
              g)
    out = F.conv2d(x, w, b, stride=stride, padding=pad)
    dx = torch.nn.grad.conv2d_input(x.shape, w, dy, stride=stride, padding=pad)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=stride,
                                     padding=pad)
    return x, w, b, dy, out, dx, dw, dy.sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def e2e_linear_case(case):
    """(x, w, b, dy, out, dx, dw, db), float64."""
    M, Kin, N = case
    fa, da, wa = amps(Kin), amps(N), amps(M)
    g = gen('e2e_linear', case)
    x = ints((M, Kin), min(fa[0], wa[0]), g)
    w = ints((N, Kin), min(fa[1], da[1]), g)
    b = ints((N,), 8, g)
    dy = ints((M, N), min(da[0], wa[1], 2), g)
    return x, w, b, dy, x @ w.t() + b, dy @ w, dy.t() @ x, dy.sum(0)


# ------------------------------------------------ independent reference
def naive_conv_int64(x, w, b, dy, stride, pad):
    """(out, dx, dw) by plain nested loops over int64, no torch conv
    routine: the oracle's own check."""
    x, w, b, dy = (t.to(torch.int64) for t in (x, w, b, dy))
    Nb, C, H, W = x.shape
    K, _, R, S = w.shape
    P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    out = b.view(1, K, 1, 1).repeat(Nb, 1, P, Q)
    dx = torch.zeros_like(x)
    dw = torch.zeros_like(w)
    for n in range(Nb):
        for k in range(K):
            for p in range(P):
                for q in range(Q):
                    for r in range(R):
                        for s in range(S):
                            h, v = p * stride - pad + r, q * stride - pad + s
                            if not (0 <= h < H and 0 <= v < W):
                                continue
                            for c in range(C):
                                out[n, k, p, q] += x[n, c, h, v] * w[k, c, r, s]
                                dx[n, c, h, v] += dy[n, k, p, q] * w[k, c, r, s]
                                dw[k, c, r, s] += dy[n, k, p, q] * x[n, c, h, v]
    return out, dx, dw
