"""The kk-split B ring of conv3x3_halo_wide_kernel (8-KiB stages, two blocks
per CU at a 128-channel contraction) through ps_conv_halo_wide_variant:
variant 2 against variant 0, the generic conv_gemm_kernel<128,128>, and
against variant 1, the same kernel on 16-KiB stages.

Only where the B fragments come from changes, so the raw bf16 outputs must be
torch.equal. The data is random normal: lattice data sums exactly in any
order and would hide a slice staged for the wrong step. The shapes are the
smallest that reach each path: one and several tiles (odd block counts, the
first and last image rows of a tile), two column tiles (B row base n0 = 128)
and W = 8 (the 160-KiB two-block budget). A 256-channel contraction keeps the
16-KiB ring: there variant 2 launches nothing and returns nonzero.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import conv_lattice as cl
from ps_pytorch_amd.ops import current_stream_ptr, require_lib

gpu = pytest.mark.gpu
BF = torch.bfloat16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# contractions (channels) variant 2 is instantiated for: at 256 the 16-KiB
# ring stayed faster, so the hook refuses variant 2 there
KK_CONTRACTIONS = (128,)


@functools.lru_cache(maxsize=None)
def _operands(Nb, C, H, W, K):
    """Random bf16 NHWC operands on the CPU, made once per shape."""
    g = torch.Generator().manual_seed(20 + 1000 * Nb + 10 * W + C + 3 * K)
    x = torch.randn(Nb, H, W, C, generator=g).to(BF)
    dy = torch.randn(Nb, H, W, K, generator=g).to(BF)
    w = torch.randn(K, C, 3, 3, generator=g).mul(0.05).to(BF)
    bias = torch.randn(K, generator=g).to(BF)
    carry = torch.randn(Nb, H, W, C, generator=g).to(BF)
    return x, dy, w, bias, carry


def _launch(shape, op, variant):
    """(return code, raw output); op in fwd, fwd+bias, dgrad, dgrad+carry."""
    Nb, C, H, W, K = shape
    x, dy, w, bias, carry = (t.to('cuda') for t in _operands(*shape))
    dgrad = op.startswith('dgrad')
    wk = (w.permute(2, 3, 1, 0) if dgrad            # wT [R, S, C, K]
          else w.permute(0, 2, 3, 1)).contiguous()  # w  [K, R, S, C]
    dst = torch.full((Nb, H, W, C if dgrad else K), cl.NAN_BITS,
                     dtype=torch.int16, device='cuda')
    rc = require_lib().ps_conv_halo_wide_variant(
        int(dgrad), (dy if dgrad else x).data_ptr(), wk.data_ptr(),
        bias.data_ptr() if op == 'fwd+bias' else 0, dst.data_ptr(),
        carry.data_ptr() if op == 'dgrad+carry' else 0,
        Nb, H, W, C, K, H, W, variant, current_stream_ptr())
    torch.cuda.synchronize()
    return rc, dst


def _eligible_batch(shape, op):
    """The shape itself, or, where the hook refuses it, the same refusal from
    every variant and the next larger batch it takes."""
    Nb, C, H, W, K = shape
    for nb in range(Nb, Nb + 4):
        rcs = [_launch((nb, C, H, W, K), op, v)[0] for v in (0, 1, 2)]
        if rcs == [0, 0, 0]:
            return (nb, C, H, W, K)
        assert all(rcs), (nb, rcs)      # refused by all three alike
    raise AssertionError(f"no eligible batch from {shape}")


# (Nb, C, H, W, K), ops
CASES = [
    ((1, 128, 16, 16, 128), ('fwd', 'dgrad', 'dgrad+carry')),   # 2 tiles
    ((3, 128, 16, 16, 128), ('fwd', 'dgrad', 'dgrad+carry')),   # 6 tiles
    ((2, 128, 16, 16, 256), ('fwd+bias',)),     # two column tiles
    ((2, 256, 16, 16, 128), ('dgrad',)),        # dgrad of 256 -> 128: same
    ((2, 128, 8, 8, 128), ('fwd', 'dgrad+carry')),      # W = 8, one tile
    ((5, 128, 8, 8, 128), ('fwd', 'dgrad+carry')),      # odd piece count
    ((2, 256, 8, 8, 256), ('fwd', 'dgrad')),    # four chunks
]


@gpu
@pytest.mark.parametrize("shape,ops", CASES)
def test_kk_ring_bit_identical_to_generic(shape, ops):
    for op in ops:
        contraction = shape[4] if op.startswith('dgrad') else shape[1]
        if contraction not in KK_CONTRACTIONS:
            assert _launch(shape, op, 2)[0] != 0
            continue
        s = _eligible_batch(shape, op)
        got = {v: _launch(s, op, v)[1] for v in (0, 1, 2)}
        for v in (0, 1, 2):
            assert not torch.isnan(got[v].view(BF)).any(), (op, v)  # all written
        assert torch.equal(got[2], got[0]), f"{op} {s}: variant 2 against 0"
        assert torch.equal(got[1], got[0]), f"{op} {s}: variant 1 against 0"


@gpu
def test_unknown_variant_launches_nothing():
    rc, dst = _launch((1, 128, 16, 16, 128), 'fwd', 3)
    assert rc != 0
    assert bool((dst == cl.NAN_BITS).all())


_CHILD = r"""
import sys
import torch
from ps_pytorch_amd.ops.conv import PsConv2d
g = torch.Generator().manual_seed(5)
conv = PsConv2d(128, 128, 3, padding=1, bias=True)
with torch.no_grad():
    conv.weight.copy_(torch.randn(128, 128, 3, 3, generator=g) * 0.05)
    conv.bias.copy_(torch.randn(128, generator=g))
conv = conv.to('cuda', torch.bfloat16)
x = torch.randn(2, 128, 16, 16, generator=g).to('cuda', torch.bfloat16) \
    .contiguous(memory_format=torch.channels_last).requires_grad_(True)
dy = torch.randn(2, 128, 16, 16, generator=g).to('cuda', torch.bfloat16) \
    .contiguous(memory_format=torch.channels_last)
out = conv(x)
out.backward(dy)
torch.cuda.synchronize()
torch.save([t.detach().float().cpu().contiguous() for t in
            (out, x.grad, conv.weight.grad, conv.bias.grad)], sys.argv[1])
"""


@gpu
def test_module_equal_under_every_switch_value(tmp_path):
    """PsConv2d forward + backward at 128 -> 128, 16x16, Nb = 2, one fresh
    process per value of PS_CONV_HALO_WIDE (the library reads it once): the
    output and the three gradients are equal across all of them."""
    procs = {}
    for val in (None, '0', '1', '2'):
        env = {k: v for k, v in os.environ.items()
               if k != 'PS_CONV_HALO_WIDE'}
        if val is not None:
            env['PS_CONV_HALO_WIDE'] = val
        procs[val] = subprocess.Popen(
            [sys.executable, '-c', _CHILD, str(tmp_path / f"sw_{val}.pt")],
            cwd=REPO, env=env, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT, text=True)
    res = {}
    for val, p in procs.items():
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, f"PS_CONV_HALO_WIDE={val}:\n{log[-2000:]}"
        res[val] = torch.load(tmp_path / f"sw_{val}.pt")
    for val in (None, '1', '2'):
        for name, a, b in zip(('out', 'dx', 'dw', 'db'), res[val], res['0']):
            assert torch.isfinite(a).all()
            assert torch.equal(a, b), f"{name}: switch {val} against 0"
