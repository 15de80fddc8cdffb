"""Case table and float64 reference for the fused GroupNorm kernels
(ops/kernels/groupnorm.hip), shared by tests/test_gn.py (CPU) and
tests/test_gn_gpu.py. Inputs come from the lattice of tests/bn_utils.py; the
forward reference of one sample is a BN-shaped dict over [HW, C] (the group's
mean / var / E[x^2] broadcast to its channels, M = HW * Cg), so that
bn_utils.fwd_bounds / io_bound / undecided apply as they stand: the kernel's
scalar chain is batchnorm.hip's, taken per (sample, group).
"""
import functools

import torch

import bn_utils as bu
from ps_pytorch_amd.ops.modules import _gn_plan

F64 = torch.float64

# (name, N, HW, C, G, relu, res). Row lanes RL = 256 / (SC / VEC); at C = 64,
# Cg <= 16 the slab is 64 (32) channels in bf16 and 32 (16) in f32: 8 granule
# lanes, RL = 32 in both types, 64 at the 64-B segment.
CASES = [
    ('cg2_rl_plus1', 3, 33, 64, 32, 1, 1),      # one slab, in-granule fold
    ('cg4_rl_minus1', 1, 31, 64, 16, 0, 1),
    ('cg8_c8_hw1', 3, 1, 8, 1, 1, 0),           # C below one slab, HW = 1
    ('cg16_c16_ragged', 1, 77, 16, 1, 0, 0),    # HW < row lanes (128 / 64)
    ('cg32_gl12', 3, 50, 96, 3, 1, 1),          # bf16: 12 lanes, RL = 21
    ('cg64_3slabs', 1, 45, 192, 3, 1, 0),       # cross-lane fold, three slabs
    ('cg4_3slabs', 3, 130, 192, 48, 0, 1),      # ragged HW, several row steps
    # plan boundaries (test_gn.py::test_plan): 128-B / 64-B / streamed
    ('bwd_128B_last', 1, 256, 64, 32, 1, 1),
    ('bwd_64B_first', 1, 257, 64, 4, 0, 0),
    ('fwd_128B_last', 1, 512, 64, 32, 0, 1),
    ('fwd_64B_first', 3, 513, 64, 4, 1, 0),     # bwd streamed: 2 chunks + 1
    ('fwd_64B_last', 1, 1024, 64, 32, 1, 1),
    ('fwd_streamed_first', 1, 1025, 64, 4, 1, 0),
    # streamed both ways, two full chunks of 512 rows plus one row
    ('streamed_2chunks_1', 3, 1025, 32, 2, 1, 1),
    # streamed past 64 chunks of 8 rows: 33 blocks of two 8-row passes
    ('streamed_capped', 1, 520, 2048, 32, 0, 1),
]
CASE_IDS = [c[0] for c in CASES]


def plans(case, elt):
    _, N, HW, C, G, _, _ = case
    return _gn_plan(HW, C, C // G, elt, 1), _gn_plan(HW, C, C // G, elt, 2)


@functools.lru_cache(maxsize=2)
def gn_case(case):
    """float64 CPU inputs of one row, [N, HW, C]: x, res (or None), dy,
    gamma, beta. Built once, never modified. Asserts the lattice condition
    HW * Cg * max(x^2) / step^2 < 2^24 (bn_utils.assert_lattice_exact with
    M = HW * Cg rows)."""
    _, N, HW, C, G, relu, res = case
    gen = bu._gen('gn', case)
    x = bu.lattice((N, HW, C), gen)
    r = bu.lattice((N, HW, C), gen) if res else None
    dy = bu.lattice((N, HW, C), gen)
    gam, beta = bu.params(C, gen)
    for t, name in ((x, 'x'), (dy, 'dy')):
        bu.assert_lattice_exact(t.reshape(HW * (C // G), N * G), 0.25,
                                f"{case} {name}")
    return x, r, dy, gam, beta


def _per_group(t, G):
    """[C] per-channel sums -> each group's total broadcast to its channels."""
    C = t.shape[0]
    return t.view(G, C // G).sum(1).repeat_interleave(C // G)


def ref_fwd_sample(x, gam, beta, res, relu, G):
    """bn_utils.ref_fwd's dict for one sample x [HW, C] with group statistics."""
    HW, C = x.shape
    m = HW * (C // G)
    s1, s2 = _per_group(x.sum(0), G), _per_group((x * x).sum(0), G)
    mean, e2 = s1 / m, s2 / m
    var = _per_group(((x - mean) ** 2).sum(0), G) / m
    invstd = 1 / torch.sqrt(var + bu.EPS)
    scale = gam * invstd
    v1 = (x - mean) * scale + beta
    pre = v1 + res if res is not None else v1
    return {'M': m, 'C': C, 'relu': relu, 's1': s1, 's2': s2, 'e2': e2,
            'mean': mean, 'var': var, 'invstd': invstd, 'scale': scale,
            'shift': beta - mean * scale, 'v1': v1, 'pre': pre,
            'mask': pre > 0, 'y': pre.clamp_min(0) if relu else pre}


@functools.lru_cache(maxsize=2)
def fwd_ref(case):
    """Per sample: (reference dict, bn_utils.fwd_bounds) of one table row."""
    _, N, HW, C, G, relu, _ = case
    x, res, _, gam, beta = gn_case(case)
    out = []
    for n in range(N):
        r = res[n] if res is not None else None
        o = ref_fwd_sample(x[n], gam, beta, r, bool(relu), G)
        out.append((o, bu.fwd_bounds(x[n], gam, beta, r, o)))
    return out


def ref_bwd_sample(x, dy, gam, mean, invstd, mask, G):
    """float64 backward of one sample from GIVEN per-channel mean / invstd
    (the kernel's saved f32 values) and mask; 'dx_abs' and 't_abs' are the
    same formulas evaluated with absolute values."""
    HW, C = x.shape
    m = HW * (C // G)
    d = dy if mask is None else dy * mask
    xc = x - mean
    s, t = d.sum(0), (d * (xc * invstd)).sum(0)
    t_abs = (d * xc * invstd).abs().sum(0)
    A, B = _per_group(gam * s, G), _per_group(gam * t, G)
    A_abs = _per_group(gam.abs() * d.abs().sum(0), G)
    B_abs = _per_group(gam.abs() * t_abs, G)
    a = gam * invstd
    dx = a * d - invstd ** 2 * B / m * xc - invstd * A / m
    dx_abs = (a.abs() * d.abs() + invstd ** 2 * B_abs / m * xc.abs()
              + invstd * A_abs / m)
    return {'d': d, 's': s, 't': t, 't_abs': t_abs, 'dx': dx, 'dx_abs': dx_abs}
