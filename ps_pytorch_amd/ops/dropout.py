"""Counter-based dropout and ReLU on the in-tree CDNA4 kernels
(ops/kernels/dropout.hip).

Replaces the at::native dropout / relu the reference reaches through
nn.Dropout / nn.ReLU (ref: src/model_ops/vgg.py:22-30). The mask is a pure
function of (seed, salt, stream, step, element index) — Philox4x32-10, see
ops/functional.py — so the CPU oracle reproduces it bit for bit, a CPU run
and a GPU run with the same seed drop the same units, and a hipGraph-captured
step draws a fresh mask on every replay (the step counter lives in device
memory and is advanced by a kernel node).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import require_lib, dtype_tag, current_stream_ptr
from .functional import (act_drop_bwd_ref, act_drop_ref, dropout_keep_mask,
                         dropout_salt_stream, dropout_scale,
                         dropout_threshold)

# A/B kill-switch: PS_DROPOUT=0 routes through F.relu / F.dropout.
_ENABLED = os.environ.get('PS_DROPOUT', '1') != '0'


def _dense(x: torch.Tensor) -> torch.Tensor:
    """The kernels treat the tensor as flat storage: any dense layout works
    as it is (a channels_last 4-D input keeps its format)."""
    if x.is_contiguous() or (
            x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last)):
        return x
    return x.contiguous()


class _ActDropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, relu, thr, scale, seed, salt_stream, step):
        lib = require_lib()
        x = _dense(x)
        n = x.numel()
        y = torch.empty_like(x)          # preserve_format: same strides
        mask = torch.empty((n + 7) // 8, dtype=torch.uint8, device=x.device)
        lib.ps_act_drop_fwd(y.data_ptr(), mask.data_ptr(), x.data_ptr(), n,
                            dtype_tag(x.dtype), int(relu), thr, scale, seed,
                            salt_stream,
                            step.data_ptr() if step is not None else 0,
                            current_stream_ptr())
        ctx.save_for_backward(mask)
        ctx.scale = scale
        ctx.layout = y.stride()
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = require_lib()
        (mask,) = ctx.saved_tensors
        # dy must be laid out like y for the flat mask to line up
        if dy.stride() != ctx.layout:
            dy = torch.empty_strided(dy.shape, ctx.layout, dtype=dy.dtype,
                                     device=dy.device).copy_(dy)
        dx = torch.empty_like(dy)
        lib.ps_act_drop_bwd(dx.data_ptr(), dy.data_ptr(), mask.data_ptr(),
                            dy.numel(), dtype_tag(dy.dtype), ctx.scale,
                            current_stream_ptr())
        return dx, None, None, None, None, None, None


def _act_drop(x, relu, thr, scale, seed, salt_stream, step):
    return _ActDropFn.apply(x, relu, thr, scale, seed, salt_stream, step)


def relu(x: torch.Tensor) -> torch.Tensor:
    """ReLU: the thr = 0, relu = 1 case of the act-drop kernel (no RNG)."""
    if _ENABLED and x.is_cuda:
        return _act_drop(x, True, 0, 1.0, 0, 0, None)
    return F.relu(x)


class PsReLU(nn.Module):
    """nn.ReLU on the in-tree kernel (F.relu on CPU)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return relu(x)


class _CpuActDropFn(torch.autograd.Function):
    """CPU training path: the oracle's Philox mask, the kernel's rounding."""

    @staticmethod
    def forward(ctx, x, keep, scale, relu):
        y, bits = act_drop_ref(x, keep, scale, relu)
        ctx.save_for_backward(bits)
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, dy):
        (bits,) = ctx.saved_tensors
        return act_drop_bwd_ref(dy, bits, ctx.scale), None, None, None


class PsDropout(nn.Module):
    """Dropout (optionally with a ReLU fused in front: relu=True computes
    dropout(relu(x))) with counter-based masks.

    `salt` tells the dropout layers of one model apart, `stream` the
    data-parallel replicas (parallel/worker.py sets it to the rank). The
    seed is torch.initial_seed() at the first training forward. The step
    counter is a plain attribute — `step`, an int64 device tensor created on
    the input's device at the first GPU training forward (`host_step`, an
    int, on CPU) — NOT a buffer: it stays out of state_dict() and
    named_buffers().
    """

    def __init__(self, p: float = 0.5, relu: bool = False, salt: int = 0):
        super().__init__()
        if p < 0.0 or p > 1.0:
            raise ValueError(f"dropout probability must be in [0, 1], got {p}")
        self.p = float(p)
        self.relu = bool(relu)
        self.salt = int(salt)
        self.stream = 0
        self.seed = None
        self.step = None
        self.host_step = 0

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.training:
            return relu(x) if self.relu else x
        if x.is_cuda and not _ENABLED:
            return F.dropout(F.relu(x) if self.relu else x, self.p, True)
        thr = dropout_threshold(self.p)
        scale = dropout_scale(self.p)
        rng = thr > 0 and self.p < 1.0
        if rng and self.seed is None:
            self.seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
        if x.is_cuda:
            step = None
            if rng:
                if self.step is None or self.step.device != x.device:
                    # first forward (must be outside graph capture: the
                    # trainer's warmup steps see to that)
                    self.step = torch.zeros((), dtype=torch.int64,
                                            device=x.device)
                step = self.step
            return _act_drop(x, self.relu, thr if rng else 0, scale,
                             self.seed if rng else 0,
                             dropout_salt_stream(self.salt, self.stream),
                             step)
        keep = dropout_keep_mask(x.numel(), self.p, self.seed or 0, self.salt,
                                 self.stream, self.host_step)
        if rng:
            self.host_step += 1
        return _CpuActDropFn.apply(x, keep, scale, self.relu)

    def extra_repr(self) -> str:
        return f"p={self.p}, relu={self.relu}, salt={self.salt}"
