"""Shared helpers for the fp32-path tests: float64 CPU references, the
exact-representability input generators and the gamma(n) rounding bound.

The bound is the standard one for an inner product of length n evaluated in
f32 in ANY order (Higham, Accuracy and Stability of Numerical Algorithms,
section 3.1):  |fl(sum a_i b_i) - sum a_i b_i| <= gamma(n) * sum |a_i b_i|,
gamma(n) = n u / (1 - n u), u = 2**-24. The tests use gamma(n + 2) to cover
the bias / carry add of the epilogue and the slab fold's extra level.
"""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24

# Nb, C, H, W, K, R, stride, pad, bias
CONV_SHAPES = [
    (2, 8, 6, 5, 16, 3, 1, 1, False),      # H != W, M = 60: ragged M tile
    (4, 64, 16, 16, 64, 3, 1, 1, False),   # M = 1024: several tiles + slabs
    (3, 72, 7, 7, 24, 3, 2, 1, False),     # odd H, stride 2; RSC = 648
    (4, 64, 8, 8, 128, 1, 2, 0, False),    # 1x1 s2: empty parity classes
    (2, 3, 33, 33, 16, 7, 2, 3, False),    # C = 3 stem, 7x7
    (4, 1, 28, 28, 20, 5, 1, 0, True),     # LeNet conv1, bias
    (4, 20, 12, 12, 50, 5, 1, 0, True),    # C and K both ragged
    (2, 130, 4, 4, 70, 3, 1, 1, False),    # C and K just past a tile edge
]


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def grid(shape, g) -> torch.Tensor:
    """Multiples of 2**-8 in [-4, 4]: needs 10 mantissa bits, so any bf16
    round-trip in the path under test changes the value."""
    return torch.randint(-1024, 1025, tuple(shape), generator=g).float() / 256.0


def ints(shape, g) -> torch.Tensor:
    return torch.randint(-4, 5, tuple(shape), generator=g).float()


def out_hw(H, W, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def conv_ref64(x, w, b, dout, stride, pad):
    """float64 CPU conv: (out, dx, dw, db) for the given upstream gradient."""
    x = x.detach().cpu().double().contiguous().requires_grad_(True)
    w = w.detach().cpu().double().contiguous().requires_grad_(True)
    b = (b.detach().cpu().double().requires_grad_(True)
         if b is not None else None)
    out = F.conv2d(x, w, b, stride=stride, padding=pad)
    ins = [x, w] + ([b] if b is not None else [])
    gr = torch.autograd.grad(out, ins, dout.detach().cpu().double())
    return out.detach(), gr[0], gr[1], (gr[2] if b is not None else None)


def conv_bounds(shape, x, w, b, dout):
    """Elementwise gamma-bounds (out, dx, dw, db) for one conv shape."""
    Nb, C, H, W, K, R, stride, pad, _ = shape
    P, Q = out_hw(H, W, R, stride, pad)
    a_out, a_dx, a_dw, a_db = conv_ref64(
        x.abs(), w.abs(), b.abs() if b is not None else None, dout.abs(),
        stride, pad)
    M = Nb * P * Q
    return (gamma(R * R * C + 2) * a_out, gamma(R * R * K + 2) * a_dx,
            gamma(M + 2) * a_dw,
            gamma(M + 2) * a_db if a_db is not None else None)


def linear_ref64(x, w, b, dout):
    x = x.detach().cpu().double().requires_grad_(True)
    w = w.detach().cpu().double().requires_grad_(True)
    b = (b.detach().cpu().double().requires_grad_(True)
         if b is not None else None)
    out = F.linear(x, w, b)
    ins = [x, w] + ([b] if b is not None else [])
    gr = torch.autograd.grad(out, ins, dout.detach().cpu().double())
    return out.detach(), gr[0], gr[1], (gr[2] if b is not None else None)


@functools.lru_cache(maxsize=None)
def conv_case(shape, kind: str):
    """CPU inputs for one shape, built once and shared (never modified).

    kind 'exact': x on the grid, w / bias integer, two upstream gradients —
    dout_i integer (for wgrad / bias grad against the grid x) and dout_g on
    the grid (for dgrad against the integer w). 'random': normal data, w
    scaled by 1/sqrt(RSC).
    """
    Nb, C, H, W, K, R, stride, pad, bias = shape
    P, Q = out_hw(H, W, R, stride, pad)
    g = gen(1000 + CONV_SHAPES.index(shape))
    if kind == 'exact':
        x = grid((Nb, C, H, W), g)
        w = ints((K, C, R, R), g)
        b = ints((K,), g) if bias else None
        d1 = ints((Nb, K, P, Q), g)
        d2 = grid((Nb, K, P, Q), g)
        return x, w, b, d1, d2
    x = torch.randn(Nb, C, H, W, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (R * R * C) ** 0.5
    b = torch.randn(K, generator=g) if bias else None
    d1 = torch.randn(Nb, K, P, Q, generator=g)
    return x, w, b, d1, None


def assert_within(got, ref64, bound, what):
    """|got - ref64| <= bound elementwise (all float64 on the CPU)."""
    got = got.detach().cpu().double()
    err = (got - ref64).abs()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    over = err > bound
    if over.any():
        ratio = (err / bound.clamp_min(1e-300))[over].max().item()
        raise AssertionError(
            f"{what}: {int(over.sum())} of {over.numel()} elements exceed the "
            f"gamma bound, worst err/bound = {ratio:.3g}")
    # how much of the bound is used (informational, shown with pytest -s)
    used = (err / bound.clamp_min(1e-300))[bound > 0]
    if used.numel():
        print(f"{what}: max err/bound = {used.max().item():.3g}")


def assert_exact(got, ref64, what):
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    if not torch.equal(got, ref64):
        bad = got != ref64
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from "
            f"float64, max |diff| = {(got - ref64).abs().max().item():.6g}")
