"""LDS-ring row-halo wgrad (conv_wgrad_row_ring_kernel) against the register
kernel it replaces on aligned shapes: the two must produce BIT-IDENTICAL
split-K slabs (same split, same row chunking, same step order per
accumulator), and dw through ps_conv_wgrad must match a torch fp32 weight
gradient. ps_conv_wgrad_row_variant launches one kernel alone (variant 0 =
register, 1 = ring), so one process can compare them."""
import functools

import pytest
import torch
import torch.nn.functional as F

from ps_pytorch_amd.ops import current_stream_ptr, require_lib

pytestmark = pytest.mark.gpu

NST = 4     # ring depth the library is built with (WG_RING_NST)

# (H = W, Nb, C, K, split)
TABLE = [
    (4, 1, 64, 64, 1),      # 4 of a step's 8 rows exist; shorter than prologue
    (4, 3, 128, 128, 1),    # 2x2 tiles; a step spans two images; 2nd partial
    (8, 2, 64, 64, 1),
    (8, 2, 64, 64, 2),
    (8, 2, 64, 64, 3),      # ipr rounds to 8: the last chunk is EMPTY
    (16, 1, 64, 64, 1),     # 8 steps
    (16, 1, 128, 64, 1),    # 8 steps, two c-tiles
    (16, 1, 64, 128, 1),    # 8 steps, two k-tiles
    (32, 1, 64, 64, 1),
    (32, 1, 64, 64, 5),     # chunks 7, 7, 7, 7, 4
]
# H = W = 16 (2 rows per step): (Nb, split) -> steps per block
STEP_SWEEP = [
    (1, 8),     # 1
    (1, 4),     # 2
    (1, 3),     # 3, 3, 2
    (1, 2),     # 4
    (3, 5),     # 5, 5, 5, 5, 4
    (2, 3),     # 6, 6, 4
    (4, 5),     # 7, 7, 7, 7, 4
    (9, 8),     # 9
    (5, 4),     # 10: one full ring group, then the longest tail
    (2, 1),     # 16: three ring groups
]
CASES = TABLE + [(16, nb, 64, 64, sp) for nb, sp in STEP_SWEEP]


def _steps_per_block(hw, nb, split):
    rows_per_step = 32 // hw
    rows = nb * hw
    ipr = -(-rows // split)
    ipr = -(-ipr // rows_per_step) * rows_per_step
    out = []
    for sid in range(split):
        r0 = sid * ipr
        r1 = min(r0 + ipr, rows)
        out.append(max(0, -(-(r1 - r0) // rows_per_step)))
    return out


def test_step_sweep_covers_every_ring_phase():
    """Steps per block take every value 1 .. 2*NST+1 (every tail length,
    nsteps below / equal to / above the ring depth), and an empty block."""
    seen = set()
    for hw, nb, _, _, sp in CASES:
        seen.update(_steps_per_block(hw, nb, sp))
    assert set(range(0, 2 * NST + 2)) <= seen, sorted(seen)


@functools.lru_cache(maxsize=None)
def _inputs(hw, nb, C, K):
    g = torch.Generator().manual_seed(1000 * hw + 100 * nb + C + 3 * K)
    x = torch.randn(nb, hw, hw, C, generator=g).to('cuda', torch.bfloat16)
    dy = torch.randn(nb, hw, hw, K, generator=g).to('cuda', torch.bfloat16)
    return x.contiguous(), dy.contiguous()          # NHWC


def _slabs(hw, nb, C, K, split, variant):
    lib = require_lib()
    x, dy = _inputs(hw, nb, C, K)
    part = torch.full((split, K, 9 * C), float('nan'), dtype=torch.float32,
                      device='cuda')
    rc = lib.ps_conv_wgrad_row_variant(
        dy.data_ptr(), x.data_ptr(), part.data_ptr(), nb, hw, hw, C, K,
        hw, hw, split, variant, current_stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return part


@pytest.mark.parametrize("case", CASES)
def test_ring_slabs_bit_identical_to_register_kernel(case):
    hw, nb, C, K, split = case
    ref = _slabs(hw, nb, C, K, split, 0)
    ring = _slabs(hw, nb, C, K, split, 1)
    # NaN-prefilled: an element either kernel leaves unwritten fails too
    assert not torch.isnan(ref).any()
    assert torch.equal(ring, ref)
    for sid, n in enumerate(_steps_per_block(hw, nb, split)):
        if n == 0:          # an empty block must still write its zeros
            assert torch.count_nonzero(ring[sid]) == 0


@pytest.mark.parametrize("case", CASES)
def test_dw_matches_torch_fp32(case):
    hw, nb, C, K, split = case
    lib = require_lib()
    x, dy = _inputs(hw, nb, C, K)
    part = torch.empty(split * K * 9 * C, dtype=torch.float32, device='cuda')
    dw = torch.empty(K, 3, 3, C, dtype=torch.bfloat16, device='cuda')
    lib.ps_conv_wgrad(dy.data_ptr(), x.data_ptr(), part.data_ptr(),
                      dw.data_ptr(), nb, hw, hw, C, K, hw, hw, 3, 3, 1, 1,
                      split, current_stream_ptr())
    wr = torch.zeros(K, C, 3, 3, device='cuda', requires_grad=True)
    out = F.conv2d(x.float().permute(0, 3, 1, 2), wr, padding=1)
    out.backward(dy.float().permute(0, 3, 1, 2))
    ref = wr.grad.permute(0, 2, 3, 1)               # [K, R, S, C]
    err = float((dw.float() - ref).abs().max()
                / ref.abs().max().clamp_min(1e-6))
    assert err < 0.03, f"wgrad {err}"


def test_ring_repeatable():
    a = _slabs(16, 4, 64, 64, 5, 1)
    b = _slabs(16, 4, 64, 64, 5, 1)
    assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [
    # H, W, P, Q, C, K
    (2, 2, 2, 2, 64, 64),       # Q = 2: halo image would overflow
    (64, 64, 64, 64, 64, 64),   # Q = 64: more than one step per row
    (16, 16, 8, 8, 64, 64),     # stride 2 shows as P != H
])
@pytest.mark.parametrize("variant", [0, 1])
def test_ineligible_shape_launches_nothing(shape, variant):
    H, W, P, Q, C, K = shape
    lib = require_lib()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, H, W, C, generator=g).to('cuda', torch.bfloat16)
    dy = torch.randn(1, P, Q, K, generator=g).to('cuda', torch.bfloat16)
    part = torch.full((1, K, 9 * C), -7.0, dtype=torch.float32, device='cuda')
    rc = lib.ps_conv_wgrad_row_variant(
        dy.data_ptr(), x.data_ptr(), part.data_ptr(), 1, H, W, C, K, P, Q,
        1, variant, current_stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((part == -7.0).all())


def test_ring_rejects_ragged_channels():
    lib = require_lib()
    x = torch.zeros(1, 8, 8, 32, dtype=torch.bfloat16, device='cuda')
    dy = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device='cuda')
    part = torch.full((1, 64, 9 * 32), -7.0, dtype=torch.float32,
                      device='cuda')
    rc = lib.ps_conv_wgrad_row_variant(
        dy.data_ptr(), x.data_ptr(), part.data_ptr(), 1, 8, 8, 32, 64, 8, 8,
        1, 1, current_stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((part == -7.0).all())
