"""Float64 oracle, lattice inputs and derived error bounds for the fused
BatchNorm kernels (ops/kernels/batchnorm.hip). Everything here runs on the
CPU; tests/test_bn_oracle.py checks the oracle itself, the GPU tests in
tests/test_bn_oracle_gpu.py compare the kernels with it.

Lattice. x, res and dy are multiples of `step` with |k| <= K (default 1/4
and 16: [-4, 4]); gamma is a multiple of 1/8 in +-[0.5, 1.5] and beta an odd
multiple of 1/16 (bf16 holds both; beta + res is never 0, so a channel with
x == mean does not sit on the relu boundary). Every partial sum of x, x^2 or
dy_eff is then an integer multiple of step^2 below 2^24 * step^2 as long as
M * max(x^2) / step^2 < 2^24, i.e. exact in f32 in ANY order. `bn_case`
asserts that. So the kernel's s1, s2 and sum(dy_eff) carry no error at all
and one skipped or doubled row shows at full size in save_mean and dbeta.

Arithmetic contract read from the kernel (docs/KERNELS.md, batchnorm.hip),
u = 2^-24, g(n) = f32_ref.gamma(n), "D" = bound on |kernel - float64|:

  mean   = fl(s1 / M)                      IEEE division of exact operands:
           the correctly rounded quotient, D_mean = u |mean|; the tests ask
           for equality with the float64 quotient rounded to f32 (rounding
           twice is harmless for a quotient: 53 >= 2 * 24 + 2).
  var    = max(fl(fl(s2 / M) - fl(mean * mean)), 0), or one fma
           D_var = b + u (var + b),  b = u E[x^2] + g(3) mean^2
           u E[x^2] is the rounding of s2 / M; g(3) mean^2 the two roundings
           inside mean_k^2 and the one of the product. b is the cancellation
           cost of the one-pass formula, about 4u E[x^2] when |mean| >> std.
           The clamp moves var_k towards var >= 0, never away.
  invstd = rsqrtf(fl(var + eps))           one add rounding, rsqrtf allowed
           2 ulp = 4u relative (HIP documents 1). Taken as an interval:
           invstd_k lies between ((var + D_var + eps)(1 + u))^-1/2 (1 - 4u)
           and ((max(var - D_var, 0) + eps)(1 - u))^-1/2 (1 + 4u);
           D_invstd is the larger distance to the float64 value. This
           stays valid where D_var > var + eps (a constant channel at a
           large offset), where a first-order bound would not.
  scale  = fl(gamma * invstd)              D_scale = |gamma| D_invstd
                                                     + u (|scale| + ...)
  shift  = fl(beta - fl(mean * scale)), or one fma
  v      = fl(fl(x * scale) + shift), or one fma; then fl(v + res)
           v_k - v = (x - mean)(scale_k - scale) - (mean_k - mean) scale_k
                     + roundings of x scale, mean scale, shift, v (, v+res)
           D_v = |x - mean| D_scale + D_mean S + u |x| S + u |mean| S
                 + u (|shift| + D_shift') + u (|v1| + ...) (+ u |v|)
           with S = |scale| + D_scale. The terms u |mean| S (twice: D_mean
           and the product rounding) are the cost of the x * scale + shift
           form when |mean| >> std.
  y      = relu?(v) rounded ONCE to the io type: D_y = D_v in f32,
           D_v + 2^-8 (|y| + D_v) in bf16 (relu is 1-Lipschitz).
  mask   = v > 0 on the f32 v in both types: must equal pre > 0 wherever
           |pre| > D_v; elements inside the band are undecided.
  running_mean = fl(fl(fl(1 - m) rm) + fl(m mean)):
           D = g(3) |(1 - m) rm| + m D_mean + g(2) m |mean|; exact where
           rm = 0 and m is a power of two (the case table).
  running_var  = the same with unbiased = fl(fl(var M) / max(M - 1, 1)):
           D_unb = D_var M / (M - 1) + g(2) (unb + ...).

  backward, with dy_eff = mask ? dy : 0 taken from the kernel's own mask:
  dbeta  = sum dy_eff                      exact on the lattice; bf16
           parameters: the exact sum rounded once to bf16.
  dgamma = sum fl(fl(dy_eff fl(x - mean_k)) invstd_k), f32, any order:
           D = g(M + 5) sum |dy_eff xhat|        (3 roundings per term,
               + sum |dy_eff| D_mean I            M - 1 adds, 2 spare)
               + sum |dy_eff (x - mean)| D_invstd,  I = invstd + D_invstd
           then rounded once to the parameter type (2^-8 in bf16).
  dx     = fl(a dy_eff + b fl(x - mean_k) + c), contraction allowed, with
           a = scale, b = fl(fl(fl(-a invstd) S) / M), c = fl(fl(-a s) / M),
           S the f32 dgamma sum and s = dbeta:
           D_b = (D_a I |S| + |a| D_invstd |S| + A I D_S) / M + g(3) |b|...
           D_c = D_a |s| / M + g(2) |c|...
           D_dx = D_a |dy_eff| + D_b |x - mean| + B (D_mean + u |x - mean|)
                  + D_c + g(3) (|a dy_eff| + |b (x - mean)| + |c|)
           and one rounding to the io type.
  dres   = dy_eff, exact.

Each "..." above is the same expression evaluated with the reference value
enlarged by its own bound, which covers the second-order terms; the code
below spells them out.
"""
import functools
import zlib

import numpy as np
import torch

import f32_ref
from f32_ref import U, gamma as g

UB = 2.0 ** -8                      # unit roundoff of bf16
EPS = float(np.float32(1e-5))       # the f32 value the kernel receives
F64 = torch.float64

# ------------------------------------------------------------ case table
# (group, C, M, relu, res). Every group meets all four (relu, res)
# combinations; every case runs in bf16 and in f32. R = 2048 / C rows per
# block pass, chunk = 8 R rows per reduce block, at most 1024 blocks.
RR = [(0, 0), (1, 0), (0, 1), (1, 1)]
ENVELOPE_C = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]


def _ragged_m(C):
    return 3 * (16384 // C) + 2048 // C + 1


CASES = (
    # tail only, M < R
    [('tail_lt_R', 8, 5, 1, 1), ('tail_lt_R', 64, 1, 1, 0),
     ('tail_lt_R', 64, 31, 0, 1), ('tail_lt_R', 64, 31, 0, 0),
     ('tail_lt_R', 64, 1, 0, 1)]
    # one full chunk + a tail of one row / a tail of chunk - 1 rows
    + [('tail_edge', 64, 257, 1, 1), ('tail_edge', 64, 255, 0, 0),
       ('tail_edge', 2048, 9, 1, 0), ('tail_edge', 2048, 7, 0, 1)]
    # M no multiple of R, several blocks
    + [('ragged', 32, 3 * 512 + 77, 1, 0), ('ragged', 128, 1000, 0, 1),
       ('ragged', 512, 7 * 7 * 3, 1, 1), ('ragged', 128, 1000, 0, 0)]
    # every C of the envelope at one ragged M
    + [('envelope', C, _ragged_m(C), *RR[(i + 1) % 4])
       for i, C in enumerate(ENVELOPE_C)]
    # fold loop b += 256: nb = 256 (last block a 3-row tail), 256, 258 (two
    # threads take a second step), and 255 (one fold thread idle)
    + [('fold', 2048, 8 * 255 + 3, 1, 1), ('fold', 2048, 8 * 256, 0, 0),
       ('fold', 2048, 8 * 257 + 1, 1, 0), ('fold', 2048, 8 * 254 + 3, 0, 1)]
    # past the 1024-block cap: second grid pass + one partial position
    + [('capped', 2048, 8192 + 8 + 3, 1, 1),
       ('capped', 512, 32768 + 32 + 3, 1, 1)]
)
CASE_IDS = [f"{c[0]}-C{c[1]}-M{c[2]}-relu{c[3]}-res{c[4]}" for c in CASES]

TAIL_CASE = ('tail_lt_R', 64, 31, 0, 1)
RAGGED_CASE = ('ragged', 128, 1000, 0, 1)
CAPPED_CASE = ('capped', 2048, 8192 + 8 + 3, 1, 1)
MOMENTUM = 0.25          # power of two: m * mean is exact (see running_mean)


def rows_per_pass(C):
    return 256 // (C // 8)


def stats_blocks(M, C):
    """Blocks (= partial rows written) of the two reduce kernels."""
    chunk = 8 * rows_per_pass(C)
    return min(-(-M // chunk), 1024)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def lattice(shape, gen, step=0.25, K=16):
    return torch.randint(-K, K + 1, tuple(shape), generator=gen).to(F64) * step


def assert_lattice_exact(x, step, what):
    """Every partial sum of x^2 (hence of x) is exact in f32."""
    M = x.shape[0]
    n = M * float((x * x).max()) / (step * step)
    assert n < 2 ** 24, f"{what}: M max(x^2) / step^2 = {n:.4g} >= 2^24"
    k = x / step
    assert torch.equal(k, k.round()), f"{what}: not on the lattice"


def params(C, gen):
    k = torch.randint(4, 13, (C,), generator=gen).to(F64)
    sign = torch.where(torch.rand(C, generator=gen) < 0.25, -1.0, 1.0).to(F64)
    gam = sign * k / 8
    j = torch.randint(-8, 8, (C,), generator=gen).to(F64)
    beta = (2 * j + 1) / 16
    return gam, beta


@functools.lru_cache(maxsize=3)
def bn_case(case, step=0.25, K=16):
    """float64 CPU inputs of one table row: x, res (or None), dy, gamma,
    beta. Built once and shared; never modified."""
    _, C, M, relu, res = case
    gen = _gen('bn', case)
    x = lattice((M, C), gen, step, K)
    r = lattice((M, C), gen, step, K) if res else None
    dy = lattice((M, C), gen, step, K)
    gam, beta = params(C, gen)
    for t, name in ((x, 'x'), (dy, 'dy')):
        assert_lattice_exact(t, step, f"{case} {name}")
    return x, r, dy, gam, beta


# ----------------------------------------------------------------- oracle
def ref_fwd(x, gam, beta, res=None, relu=False, rm=None, rv=None,
            momentum=MOMENTUM, eps=EPS, training=True, stats_x=None):
    """float64 forward in [M, C] form. stats_x: take the batch statistics
    from another [M, C] tensor (the ext_stats input). Returns a dict."""
    M, C = x.shape
    o = {'M': M, 'C': C, 'relu': relu}
    if training:
        sx = x if stats_x is None else stats_x
        assert sx.shape[0] == M
        mean = sx.sum(0) / M
        var = ((sx - mean) ** 2).sum(0) / M
        o['s1'], o['s2'] = sx.sum(0), (sx * sx).sum(0)
        o['e2'] = o['s2'] / M
        if rm is not None:
            unb = var * M / (M - 1 if M > 1 else 1)
            o['unbiased'] = unb
            o['running_mean'] = (1 - momentum) * rm + momentum * mean
            o['running_var'] = (1 - momentum) * rv + momentum * unb
    else:
        mean, var = rm, rv
    invstd = 1 / torch.sqrt(var + eps)
    scale = gam * invstd
    pre = (x - mean) * scale + beta
    o['v1'] = pre
    if res is not None:
        pre = pre + res
    o.update(mean=mean, var=var, invstd=invstd, scale=scale,
             shift=beta - mean * scale, pre=pre, mask=pre > 0,
             y=pre.clamp_min(0) if relu else pre)
    return o


def ref_bwd(x, dy, gam, mean, invstd, mask=None):
    """float64 backward for a GIVEN mask ([M, C] bool, or None)."""
    M = x.shape[0]
    d = dy if mask is None else dy * mask
    xc = x - mean
    xhat = xc * invstd
    dbeta = d.sum(0)
    dgamma = (d * xhat).sum(0)
    dx = gam * invstd * (d - dbeta / M - xhat * dgamma / M)
    return {'dy_eff': d, 'xc': xc, 'xhat': xhat, 'dbeta': dbeta,
            'dgamma': dgamma, 'dx': dx, 'dres': d}


def unpack_mask(mask_bytes, M, C):
    """[M * C / 8] uint8 -> [M, C] bool: bit k of byte [r * G + cg] is
    channel cg * 8 + k."""
    b = mask_bytes.view(M, C // 8, 1).to(torch.int32)
    return ((b >> torch.arange(8, dtype=torch.int32)) & 1).bool().view(M, C)


# ----------------------------------------------------------------- bounds
def io_bound(bound, ref, bf16):
    """One rounding to the io / parameter type on top of an f32 bound."""
    return bound + UB * (ref.abs() + bound) if bf16 else bound


def fwd_bounds(x, gam, beta, res, o, rm=None, rv=None, momentum=MOMENTUM,
               eps=EPS, training=True):
    """Elementwise bounds for the forward outputs; see the module docstring
    for each term. `o` is ref_fwd's result for the same arguments. The bound
    on y is io_bound(b['v'], o['y'], bf16)."""
    M = o['M']
    mean, var, invstd, scale = o['mean'], o['var'], o['invstd'], o['scale']
    b = {}
    if training:
        d_mean = U * mean.abs()
        bb = U * o['e2'] + g(3) * mean ** 2
        d_var = bb + U * (var + bb)
    else:                       # running statistics are read, not computed
        d_mean = torch.zeros_like(mean)
        d_var = torch.zeros_like(var)
    # t = (var_k + eps)(1 + d), |d| <= u; rsqrtf(t) within 2 ulp = 4u
    hi = (((var - d_var).clamp_min(0) + eps) * (1 - U)) ** -0.5 * (1 + 4 * U)
    lo = ((var + d_var + eps) * (1 + U)) ** -0.5 * (1 - 4 * U)
    d_invstd = torch.maximum(hi - invstd, invstd - lo)
    d_scale = gam.abs() * d_invstd
    d_scale = d_scale + U * (scale.abs() + d_scale)
    S = scale.abs() + d_scale
    shift = o['shift']
    # shift_k itself (the ws check): mean_k scale_k rounded, then the sum
    d_shift = (d_mean * S + mean.abs() * d_scale + U * (mean.abs() + d_mean) * S)
    d_shift = d_shift + U * (shift.abs() + d_shift)
    v1 = o['v1']
    d_v = ((x - mean).abs() * d_scale + d_mean * S + U * x.abs() * S
           + U * (mean.abs() + d_mean) * S + U * (shift.abs() + d_shift))
    d_v = d_v + U * (v1.abs() + d_v)
    if res is not None:
        d_v = d_v + U * (o['pre'].abs() + d_v)
    b.update(mean=d_mean, var=d_var, invstd=d_invstd, scale=d_scale,
             shift=d_shift, v=d_v)
    if training and rm is not None:
        m = momentum
        b['running_mean'] = (g(3) * ((1 - m) * rm).abs() + m * d_mean
                             + g(2) * m * (mean.abs() + d_mean))
        Md = M - 1 if M > 1 else 1
        d_unb = d_var * M / Md
        d_unb = d_unb + g(2) * (o['unbiased'] + d_unb)
        b['running_var'] = (g(3) * ((1 - m) * rv).abs() + m * d_unb
                            + g(2) * m * (o['unbiased'] + d_unb))
    return b


def bwd_bounds(gam, o, fb, r, bf16=False):
    """Bounds for dgamma and dx; o, fb: forward reference and bounds, r:
    ref_bwd's result. dbeta and dres are exact."""
    M = o['M']
    invstd, scale = o['invstd'], o['scale']
    d, xc = r['dy_eff'], r['xc']
    I = invstd + fb['invstd']
    d_S = (g(M + 5) * (d * r['xhat']).abs().sum(0)
           + d.abs().sum(0) * fb['mean'] * I
           + (d * xc).abs().sum(0) * fb['invstd'])
    S = r['dgamma'].abs()
    s = r['dbeta'].abs()
    d_a = fb['scale']
    A = scale.abs() + d_a
    bref = (scale * invstd * r['dgamma'] / M).abs()
    d_b = (d_a * I * S + scale.abs() * fb['invstd'] * S + A * I * d_S) / M
    d_b = d_b + g(3) * (bref + d_b)
    B = bref + d_b
    cref = (scale * r['dbeta'] / M).abs()
    d_c = d_a * s / M
    d_c = d_c + g(2) * (cref + d_c)
    d_dx = (d_a * d.abs() + d_b * xc.abs() + B * (fb['mean'] + U * xc.abs())
            + d_c + g(3) * (A * d.abs() + B * (xc.abs() + fb['mean'])
                            + cref + d_c))
    return {'dgamma_f32': d_S, 'dgamma': io_bound(d_S, r['dgamma'], bf16),
            'dx': io_bound(d_dx, r['dx'], bf16), 'b': d_b, 'c': d_c}


def undecided(o, fb):
    """Elements whose relu decision the bound on v leaves open."""
    return o['pre'].abs() <= fb['v']


# ------------------------------------------------- checks with a record
RATIOS = {}      # (quantity, type) -> largest err / bound seen in this run


def check_within(got, ref, bound, what, key=None):
    """f32_ref.assert_within, NaN-proof, recording the largest err/bound."""
    got = got.detach().cpu().to(F64).view(ref.shape)
    assert not torch.isnan(got).any(), f"{what}: elements never written"
    f32_ref.assert_within(got, ref, bound, what)
    if key is not None:
        pos = bound > 0
        if pos.any():
            ratio = float(((got - ref).abs()[pos] / bound[pos]).max())
            RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def check_exact(got, ref, what):
    got = got.detach().cpu().to(F64).view(ref.shape)
    assert not torch.isnan(got).any(), f"{what}: elements never written"
    f32_ref.assert_exact(got, ref, what)


def once(ref, dtype):
    """The float64 value rounded once to `dtype`, back in float64."""
    return ref.to(dtype).to(F64)


# ---------------------------------------------------- offset-mean inputs
OFFSET_M, OFFSET_C = 128, 8


def offset_case(bf16):
    """x with |mean| >> std. Channels 0-3: 64 + lattice in [-1, 1];
    channel 4: constant; channel 5: mean 2, std 1 (64 rows at 1, 64 at 3);
    channels 6, 7: the plain lattice. bf16 holds 64.25 only as 64 (its
    spacing is 1/2 above 64), so the bf16 inputs use the step 1/2 and the
    constant 64.5; f32 uses 1/4 and 64.25. The sums stay exact:
    128 * 65^2 * 16 < 2^24."""
    step = 0.5 if bf16 else 0.25
    gen = _gen('bn_offset', bf16)
    M, C = OFFSET_M, OFFSET_C
    x = lattice((M, C), gen)
    K = int(1 / step)
    x[:, :4] = 64 + lattice((M, 4), gen, step, K)
    x[:, 4] = 64 + step
    x[:, 5] = 2 + torch.where(torch.randperm(M, generator=gen) < M // 2, -1.0, 1.0).to(F64)
    assert_lattice_exact(x, 0.25, 'offset x')
    res = lattice((M, C), gen)
    dy = lattice((M, C), gen)
    gam, beta = params(C, gen)
    return x, res, dy, gam, beta
