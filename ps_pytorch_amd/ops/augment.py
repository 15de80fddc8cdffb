"""Fused batch loader op on the in-tree CDNA4 kernel (ops/kernels/augment.hip).

One call turns B dataset indices into a finished training batch: gather from
the device-resident uint8 dataset, random crop out of the padded image,
horizontal flip, normalize, cast, channels-last layout, labels. The batch is
a pure function of (seed, stream, step, batch slot, dataset index) —
Philox4x32-10, see ops/functional.py augment_draws — so a CPU run and a GPU
run with the same seed see the same batches bit for bit, and a
hipGraph-captured loader draws fresh offsets on every replay (the step lives
in device memory and is advanced by a kernel node).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch

from . import require_lib, dtype_tag, current_stream_ptr
from .functional import augment_draws, augment_ref

MAX_CHANNELS = 4
_PAD_MODES = (None, 'reflect', 'constant')


def uses_rng(pad: int, hflip: bool) -> bool:
    """Whether a call with these parameters draws (and advances the step)."""
    return pad > 0 or bool(hflip)


def check_augment_args(x_u8: torch.Tensor, y: torch.Tensor, idx: torch.Tensor,
                       mean255: Sequence[float], inv_std255: Sequence[float],
                       pad: int, pad_mode: Optional[str],
                       dtype: torch.dtype) -> None:
    """The kernel's preconditions; ValueError when one does not hold. Index
    VALUES are the caller's responsibility (the kernel does not check them)."""
    if x_u8.dim() != 4 or x_u8.dtype != torch.uint8:
        raise ValueError("x_u8 must be a uint8 [N,C,H,W] tensor, got "
                         f"{x_u8.dtype} {tuple(x_u8.shape)}")
    if not x_u8.is_contiguous():
        raise ValueError("x_u8 must be NCHW contiguous")
    N, C, H, W = x_u8.shape
    if C > MAX_CHANNELS:
        raise ValueError(f"at most {MAX_CHANNELS} channels, got {C}")
    if H >= 65536 or W >= 65536:
        raise ValueError(f"H and W must be below 65536, got {H}x{W}")
    if y.dtype != torch.int64 or y.dim() != 1 or y.numel() != N:
        raise ValueError(f"y must be int64 [{N}], got {y.dtype} "
                         f"{tuple(y.shape)}")
    if idx.dtype != torch.int64 or idx.dim() != 1:
        raise ValueError(f"idx must be int64 [B], got {idx.dtype} "
                         f"{tuple(idx.shape)}")
    if not (y.is_contiguous() and idx.is_contiguous()):
        raise ValueError("y and idx must be contiguous")
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"output dtype must be float32 or bfloat16, "
                         f"got {dtype}")
    if len(mean255) != C or len(inv_std255) != C:
        raise ValueError(f"mean255 / inv_std255 need {C} values each")
    if pad_mode not in _PAD_MODES:
        raise ValueError(f"pad_mode must be one of {_PAD_MODES}, "
                         f"got {pad_mode!r}")
    if pad < 0 or pad >= 65536:
        raise ValueError(f"pad must be in [0, 65536), got {pad}")
    if pad > 0 and pad_mode is None:
        raise ValueError("pad > 0 needs a pad_mode")
    if pad_mode == 'reflect' and pad > min(H, W) - 1:
        raise ValueError(f"reflect padding needs pad <= min(H, W) - 1 = "
                         f"{min(H, W) - 1}, got {pad}")


def _floats(v) -> list:
    if isinstance(v, torch.Tensor):
        v = v.detach().reshape(-1).tolist()
    return [float(f) for f in v]


def _check_out(out: torch.Tensor, out_y: torch.Tensor, shape, dtype,
               device) -> None:
    if (tuple(out.shape) != tuple(shape) or out.dtype != dtype
            or out.device != device
            or not out.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError(f"out must be a channels-last {dtype} tensor of "
                         f"shape {tuple(shape)} on {device}")
    if (out_y.dtype != torch.int64 or tuple(out_y.shape) != (shape[0],)
            or out_y.device != device or not out_y.is_contiguous()):
        raise ValueError(f"out_y must be a contiguous int64 [{shape[0]}] "
                         f"tensor on {device}")


def augment_batch(x_u8: torch.Tensor, y: torch.Tensor, idx: torch.Tensor,
                  mean255: Sequence[float], inv_std255: Sequence[float],
                  pad: int = 0, pad_mode: Optional[str] = None,
                  hflip: bool = False, augment: bool = True, seed: int = 0,
                  stream: int = 0, step=None,
                  dtype: torch.dtype = torch.float32,
                  out: Optional[torch.Tensor] = None,
                  out_y: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(batch [B,C,H,W] channels-last in `dtype`, labels int64 [B]) for the
    dataset indices `idx`.

    mean255 / inv_std255: per-channel f32 values as Python floats. With
    augment=False, or pad == 0 and no hflip, the call is a plain gather +
    normalize: no RNG, `step` is ignored and not advanced. Otherwise `step`
    is the draw counter: on the GPU an int64 device scalar, advanced by the
    call (a kernel behind the loader kernel); on the CPU an int, which the
    caller advances."""
    pad = int(pad)
    mean255, inv_std255 = _floats(mean255), _floats(inv_std255)
    check_augment_args(x_u8, y, idx, mean255, inv_std255, pad, pad_mode,
                       dtype)
    if not augment:
        pad, pad_mode, hflip = 0, None, False
    rng = uses_rng(pad, hflip)
    B = idx.numel()
    _, C, H, W = x_u8.shape

    if not x_u8.is_cuda:
        draws = (augment_draws(B, pad, hflip, seed, stream, int(step or 0))
                 if rng else None)
        xb, yb = augment_ref(x_u8, y, idx, mean255, inv_std255, pad,
                             pad_mode, hflip, draws, dtype)
        if out is not None:
            _check_out(out, out_y, (B, C, H, W), dtype, x_u8.device)
            out.copy_(xb)
            out_y.copy_(yb)
            return out, out_y
        return xb, yb

    lib = require_lib()
    dev = x_u8.device
    if y.device != dev or idx.device != dev:
        raise ValueError("x_u8, y and idx must live on one device")
    if rng:
        if (not isinstance(step, torch.Tensor) or step.dtype != torch.int64
                or step.numel() != 1 or step.device != dev):
            raise ValueError("step must be an int64 scalar tensor on "
                             f"{dev} when the call draws")
    if out is None:
        out = torch.empty((B, C, H, W), dtype=dtype, device=dev,
                          memory_format=torch.channels_last)
        out_y = torch.empty(B, dtype=torch.int64, device=dev)
    else:
        _check_out(out, out_y, (B, C, H, W), dtype, dev)
    f4 = ctypes.c_float * MAX_CHANNELS
    pad4 = [0.0] * (MAX_CHANNELS - C)
    lib.ps_augment_batch(
        out.data_ptr(), out_y.data_ptr(), x_u8.data_ptr(), y.data_ptr(),
        idx.data_ptr(), B, C, H, W, dtype_tag(dtype), pad,
        int(pad_mode == 'reflect'), int(bool(hflip)),
        f4(*mean255, *pad4), f4(*inv_std255, *pad4),
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFF,
        step.data_ptr() if rng else 0, current_stream_ptr())
    return out, out_y
