"""Fused NHWC BatchNorm(+residual)(+ReLU) module on the hand-written CDNA4
kernels (ops/kernels/batchnorm.hip), with a torch fallback that doubles as
the numerics reference (tests/test_bn.py; the kernels are held to the float64
oracle of tests/bn_utils.py by tests/test_bn_oracle_gpu.py).

State-dict surface matches nn.BatchNorm2d (weight, bias, running_mean,
running_var, num_batches_tracked) so checkpoints stay evaluator-compatible.

PsGroupNorm2d (below) is the GroupNorm counterpart on
ops/kernels/groupnorm.hip, with nn.GroupNorm's state dict.

PsLayerNorm2d, PsGELU and PsLayerScaleAdd (last section) are the steps of a
ConvNeXt block between its convolutions, on ops/kernels/layernorm.hip.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import require_lib, dtype_tag, current_stream_ptr

_CL = torch.channels_last


def _kernel_ok(x: torch.Tensor) -> bool:
    if not x.is_cuda or x.dim() != 4:
        return False
    C = x.shape[1]
    # stats kernels need C/8 lane-groups dividing the 256-thread block
    return (C % 8 == 0 and C <= 2048 and (256 % (C // 8)) == 0 and
            x.dtype in (torch.bfloat16, torch.float32))


class _FusedBNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var,
                momentum, eps, relu):
        lib = require_lib()
        x = x.contiguous(memory_format=_CL)
        if residual is not None:
            residual = residual.contiguous(memory_format=_CL)
        N, C, H, W = x.shape
        M = N * H * W
        y = torch.empty_like(x)
        save_mean = torch.empty(C, dtype=torch.float32, device=x.device)
        save_invstd = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = torch.empty(5 * C, dtype=torch.float32, device=x.device)
        partial = torch.empty(1024 * 2 * C, dtype=torch.float32, device=x.device)
        # bit-packed relu mask (1 byte per 8 channels): the backward reads
        # this instead of re-reading the full y tensor for the mask
        mask = (torch.empty(M * (C // 8), dtype=torch.uint8, device=x.device)
                if relu else None)
        # stats handshake: the producing conv's epilogue may have already
        # written this activation's per-channel sum/sumsq partials
        ext = getattr(x, '_ps_bn_stats', None)
        lib.ps_bn_fwd(
            x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
            running_mean.data_ptr(), running_var.data_ptr(),
            save_mean.data_ptr(), save_invstd.data_ptr(), ws.data_ptr(),
            partial.data_ptr(),
            residual.data_ptr() if residual is not None else 0,
            mask.data_ptr() if mask is not None else 0,
            ext[0].data_ptr() if ext is not None else 0,
            ext[1] if ext is not None else 0,
            M, C, float(momentum), float(eps), 1, int(relu),
            dtype_tag(x.dtype), current_stream_ptr())
        ctx.save_for_backward(x, gamma, save_mean, save_invstd)
        ctx.mask = mask
        ctx.relu = relu
        ctx.has_res = residual is not None
        # steal-mode flat_g targets (see parallel/flat.py attach_grads)
        ctx.gtgt = (getattr(gamma, '_ps_flat_grad_fn', None),
                    getattr(beta, '_ps_flat_grad_fn', None))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = require_lib()
        x, gamma, save_mean, save_invstd = ctx.saved_tensors
        mask = ctx.mask
        dy = dy.contiguous(memory_format=_CL)
        N, C, H, W = x.shape
        M = N * H * W
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if ctx.has_res else None
        g_tgt = ctx.gtgt[0]() if ctx.gtgt[0] is not None else None
        b_tgt = ctx.gtgt[1]() if ctx.gtgt[1] is not None else None
        dgamma = (g_tgt if g_tgt is not None and g_tgt.dtype == gamma.dtype
                  and g_tgt.is_cuda else torch.empty_like(gamma))
        dbeta = (b_tgt if b_tgt is not None and b_tgt.dtype == gamma.dtype
                 and b_tgt.is_cuda else torch.empty_like(gamma))
        ws = torch.empty(5 * C, dtype=torch.float32, device=x.device)
        partial = torch.empty(1024 * 2 * C, dtype=torch.float32, device=x.device)
        lib.ps_bn_bwd(
            x.data_ptr(), mask.data_ptr() if mask is not None else 0,
            dy.data_ptr(), gamma.data_ptr(),
            save_mean.data_ptr(), save_invstd.data_ptr(), dx.data_ptr(),
            dgamma.data_ptr(), dbeta.data_ptr(),
            dres.data_ptr() if dres is not None else 0, ws.data_ptr(),
            partial.data_ptr(),
            M, C, int(ctx.relu), dtype_tag(x.dtype), current_stream_ptr())
        return (dx, dgamma, dbeta, dres, None, None, None, None, None)


def _bn_eval_fused(x, gamma, beta, residual, rmean, rvar, eps, relu):
    lib = require_lib()
    x = x.contiguous(memory_format=_CL)
    if residual is not None:
        residual = residual.contiguous(memory_format=_CL)
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    ws = torch.empty(5 * C, dtype=torch.float32, device=x.device)
    lib.ps_bn_fwd(x.data_ptr(), y.data_ptr(), gamma.data_ptr(),
                  beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(),
                  0, 0, ws.data_ptr(), 0,
                  residual.data_ptr() if residual is not None else 0, 0,
                  0, 0,
                  N * H * W, C, 0.0, float(eps), 0, int(relu),
                  dtype_tag(x.dtype), current_stream_ptr())
    return y


class PsBatchNorm2d(nn.Module):
    """BatchNorm2d with optional fused residual-add + ReLU epilogue.

    forward(x, residual=None) == relu?(bn(x) + residual).
    GPU training path: hand-written NHWC kernels; otherwise torch ops.
    """

    def __init__(self, num_features: int, eps: float = 1e-5,
                 momentum: float = 0.1, relu: bool = False):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.relu = relu
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer('running_mean', torch.zeros(num_features))
        self.register_buffer('running_var', torch.ones(num_features))
        self.register_buffer('num_batches_tracked',
                             torch.tensor(0, dtype=torch.long))

    def _ensure_f32_stats(self) -> None:
        # running stats stay f32 even when the module is cast to bf16
        if self.running_mean.dtype != torch.float32:
            self.running_mean.data = self.running_mean.data.float()
            self.running_var.data = self.running_var.data.float()

    # num_batches_tracked: the canonical buffer update is a device-side
    # long add — 20 kernel launches per ResNet-18 step for a counter nobody
    # reads during training. Count on the host and materialize into the
    # buffer only when a state_dict is taken (or synced in from a load).
    def _sync_nbt_out(self, *a):
        host = getattr(self, '_nbt_host', 0)
        if host:
            self.num_batches_tracked.fill_(int(self.num_batches_tracked)
                                           + host)
            self._nbt_host = 0

    def _load_from_state_dict(self, *args, **kw):
        self._nbt_host = 0
        super()._load_from_state_dict(*args, **kw)

    def _save_to_state_dict(self, *args, **kw):
        # (root state_dict() recurses here, not into child .state_dict())
        self._sync_nbt_out()
        super()._save_to_state_dict(*args, **kw)

    def forward(self, x: torch.Tensor,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.training:
            self._nbt_host = getattr(self, '_nbt_host', 0) + 1
        if self.training and _kernel_ok(x):
            self._ensure_f32_stats()
            return _FusedBNFn.apply(x, self.weight, self.bias, residual,
                                    self.running_mean, self.running_var,
                                    self.momentum, self.eps, self.relu)
        if (not self.training and _kernel_ok(x)
                and not torch.is_grad_enabled()):
            # eval-mode fused path (running-stats normalize + res + relu)
            self._ensure_f32_stats()
            return _bn_eval_fused(x, self.weight, self.bias, residual,
                                  self.running_mean, self.running_var,
                                  self.eps, self.relu)
        # torch fallback (CPU, eval mode, unsupported shapes)
        rm = self.running_mean
        rv = self.running_var
        if rm.dtype != x.dtype and not x.is_cuda:
            rm = rm.to(x.dtype)
            rv = rv.to(x.dtype)
            y = F.batch_norm(x, rm, rv, self.weight, self.bias,
                             self.training, self.momentum, self.eps)
            if self.training:   # write back updated stats
                self.running_mean.data.copy_(rm.float())
                self.running_var.data.copy_(rv.float())
        else:
            self._ensure_f32_stats()
            y = F.batch_norm(x, self.running_mean, self.running_var,
                             self.weight, self.bias, self.training,
                             self.momentum, self.eps)
        if residual is not None:
            y = y + residual
        if self.relu:
            y = F.relu(y)
        return y

    def extra_repr(self) -> str:
        return (f"{self.num_features}, eps={self.eps}, "
                f"momentum={self.momentum}, relu={self.relu}")


# ---------------------------------------------------------------- GroupNorm
# Fused NHWC GroupNorm(+residual)(+ReLU) on ops/kernels/groupnorm.hip. The
# statistics are per (sample, group): no running buffers, train() and eval()
# run the same kernels, and a worker's shard of the batch changes nothing.

_GN_CG = (2, 4, 8, 16, 32, 64)
_GN_LDS_TILE_BUDGET = 64 * 1024


def _gn_ok(x: torch.Tensor, num_groups: int) -> bool:
    if not x.is_cuda or x.dim() != 4:
        return False
    C = x.shape[1]
    return (C % 8 == 0 and C <= 2048 and C % num_groups == 0
            and C // num_groups in _GN_CG and x.numel() > 0
            and x.dtype in (torch.bfloat16, torch.float32))


def _gn_plan(HW: int, C: int, Cg: int, elt_bytes: int, tiles: int) -> int:
    """Channels per block (`slab`) of the sample-resident GroupNorm kernels,
    or 0 for the streamed form. The only place this rule lives; the launch
    functions take the result as given.

    A block owns one sample x SC consecutive channels: SC is the smallest
    count that holds whole groups, whole 16-B granules and whole mask octets,
    divides C and spans at least `seg` bytes of every pixel (SC = C where C
    itself is narrower). seg is tried at 128 B, then 64 B; a wider group
    raises it to Cg * elt_bytes. The form is resident iff `tiles` [HW][SC]
    tiles (1 forward, 2 backward: x and dy) fit the 64-KiB block budget and
    the SC / (16 / elt_bytes) granule lanes fit one 256-thread block."""
    vec = 16 // elt_bytes
    unit = Cg if Cg % 8 == 0 else 8
    for seg in (128, 64):
        seg = max(seg, Cg * elt_bytes)
        if C * elt_bytes <= seg:
            sc = C
        else:
            sc = next(s for s in range(unit, C + 1, unit)
                      if C % s == 0 and s * elt_bytes >= seg)
        if (sc // vec <= 256
                and tiles * HW * sc * elt_bytes <= _GN_LDS_TILE_BUDGET):
            return sc
    return 0


class _FusedGNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, num_groups, eps, relu, need_grad):
        lib = require_lib()
        x = x.contiguous(memory_format=_CL)
        if residual is not None:
            residual = residual.contiguous(memory_format=_CL)
        N, C, H, W = x.shape
        HW, G = H * W, num_groups
        dev = x.device
        slab = _gn_plan(HW, C, C // G, x.element_size(), 1)
        y = torch.empty_like(x)
        # resident form without a backward: no statistics, no mask written
        stats = need_grad or not slab
        save_mean = (torch.empty(N * G, dtype=torch.float32, device=dev)
                     if stats else None)
        save_invstd = torch.empty_like(save_mean) if stats else None
        mask = (torch.empty(N * HW * (C // 8), dtype=torch.uint8, device=dev)
                if relu and need_grad else None)
        ws = (None if slab else torch.empty(
            lib.ps_gn_ws_floats(N, HW, C, G), dtype=torch.float32, device=dev))
        rc = lib.ps_gn_fwd(
            x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
            residual.data_ptr() if residual is not None else 0,
            mask.data_ptr() if mask is not None else 0,
            save_mean.data_ptr() if stats else 0,
            save_invstd.data_ptr() if stats else 0,
            ws.data_ptr() if ws is not None else 0,
            N, HW, C, G, float(eps), int(relu), slab,
            dtype_tag(x.dtype), current_stream_ptr())
        if rc:
            raise RuntimeError(
                f"ps_gn_fwd rejected N={N} HW={HW} C={C} G={G} slab={slab} "
                f"{x.dtype} (rc={rc})")
        if need_grad:
            ctx.save_for_backward(x, gamma, save_mean, save_invstd)
        ctx.mask = mask
        ctx.relu = relu
        ctx.G = G
        ctx.has_res = residual is not None
        # steal-mode flat_g targets (see parallel/flat.py attach_grads)
        ctx.gtgt = (getattr(gamma, '_ps_flat_grad_fn', None),
                    getattr(beta, '_ps_flat_grad_fn', None))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = require_lib()
        x, gamma, save_mean, save_invstd = ctx.saved_tensors
        mask, G = ctx.mask, ctx.G
        dy = dy.contiguous(memory_format=_CL)
        N, C, H, W = x.shape
        HW = H * W
        dev = x.device
        slab = _gn_plan(HW, C, C // G, x.element_size(), 2)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if ctx.has_res else None
        g_tgt = ctx.gtgt[0]() if ctx.gtgt[0] is not None else None
        b_tgt = ctx.gtgt[1]() if ctx.gtgt[1] is not None else None
        dgamma = (g_tgt if g_tgt is not None and g_tgt.dtype == gamma.dtype
                  and g_tgt.is_cuda else torch.empty_like(gamma))
        dbeta = (b_tgt if b_tgt is not None and b_tgt.dtype == gamma.dtype
                 and b_tgt.is_cuda else torch.empty_like(gamma))
        partial = torch.empty(N * 2 * C, dtype=torch.float32, device=dev)
        ws = (None if slab else torch.empty(
            lib.ps_gn_ws_floats(N, HW, C, G), dtype=torch.float32, device=dev))
        rc = lib.ps_gn_bwd(
            x.data_ptr(), mask.data_ptr() if mask is not None else 0,
            dy.data_ptr(), gamma.data_ptr(), save_mean.data_ptr(),
            save_invstd.data_ptr(), dx.data_ptr(), dgamma.data_ptr(),
            dbeta.data_ptr(), dres.data_ptr() if dres is not None else 0,
            partial.data_ptr(), ws.data_ptr() if ws is not None else 0,
            N, HW, C, G, int(ctx.relu), slab, dtype_tag(x.dtype),
            current_stream_ptr())
        if rc:
            raise RuntimeError(
                f"ps_gn_bwd rejected N={N} HW={HW} C={C} G={G} slab={slab} "
                f"{x.dtype} (rc={rc})")
        return (dx, dgamma, dbeta, dres, None, None, None, None)


class PsGroupNorm2d(nn.Module):
    """GroupNorm over NCHW input with optional fused residual-add + ReLU.

    forward(x, residual=None) == relu?(group_norm(x) + residual), the same in
    train() and eval(). GPU path: the hand-written NHWC kernels of
    groupnorm.hip; PS_GN=0, CPU tensors and shapes outside their envelope
    (C % 8, C/G not in 2..64, C > 2048, non-4-D) take F.group_norm, which is
    also the numerics reference. State dict: nn.GroupNorm's (weight, bias).
    `kernel_calls` / `fallback_calls` count the forwards of either path.
    """

    def __init__(self, num_groups: int, num_channels: int, eps: float = 1e-5,
                 relu: bool = False):
        super().__init__()
        if num_channels % num_groups:
            raise ValueError("num_channels must be divisible by num_groups")
        self.num_groups = num_groups
        self.num_channels = num_channels
        self.eps = eps
        self.relu = relu
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))
        self.kernel_calls = 0
        self.fallback_calls = 0

    def forward(self, x: torch.Tensor,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        if (os.environ.get('PS_GN', '1') != '0' and _gn_ok(x, self.num_groups)
                and self.weight.dtype == x.dtype):
            self.kernel_calls += 1
            need_grad = torch.is_grad_enabled() and (
                x.requires_grad or self.weight.requires_grad
                or self.bias.requires_grad
                or (residual is not None and residual.requires_grad))
            return _FusedGNFn.apply(x, self.weight, self.bias, residual,
                                    self.num_groups, self.eps, self.relu,
                                    need_grad)
        self.fallback_calls += 1
        y = F.group_norm(x, self.num_groups, self.weight, self.bias, self.eps)
        if residual is not None:
            y = y + residual
        if self.relu:
            y = F.relu(y)
        return y

    def extra_repr(self) -> str:
        return (f"{self.num_groups}, {self.num_channels}, eps={self.eps}, "
                f"relu={self.relu}")


# ------------------------------------------- LayerNorm / GELU / layer scale
# The steps of a ConvNeXt block between its convolutions, on
# ops/kernels/layernorm.hip. PS_LN=0 sends all three back to torch.

_LN_MAX_BLOCKS = 512      # about two blocks per CU on 256 CUs; also the cap
_LN_MIN_PASSES = 8        # floor: passes of 256/LG rows a block walks


def _ln_on() -> bool:
    return os.environ.get('PS_LN', '1') != '0'


def _ln_ok(x: torch.Tensor, *params: torch.Tensor) -> bool:
    """The row kernels' envelope; params are the per-channel vectors, which
    must be on x's device in x's type."""
    if not (_ln_on() and x.is_cuda and x.dim() == 4 and x.numel() > 0):
        return False
    C = x.shape[1]
    return (C % 8 == 0 and 8 <= C <= 2048
            and x.dtype in (torch.bfloat16, torch.float32)
            and all(p.dtype == x.dtype and p.device == x.device
                    and p.numel() == C for p in params))


def _vec16(t: torch.Tensor) -> torch.Tensor:
    """t dense (4-D: channels_last, else row-major) and 16-B aligned, as the
    kernels' 16-B accesses need; a dense view at an odd storage offset is
    copied."""
    t = t.contiguous(memory_format=_CL) if t.dim() == 4 else t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(
        memory_format=torch.preserve_format)


def _ln_plan(M: int, C: int, elt_bytes: int):
    """(rows_per_block, blocks) of the row kernels of layernorm.hip. The only
    place this rule lives; the launch functions take the result as given.

    A lane group of LG lanes (the smallest of 8, 16, 32, 64 that holds the
    row's C / (16 / elt_bytes) granules, 64 above) owns a row, so a block
    handles unit = 256 / LG rows at once. A block takes one contiguous chunk:
    M spread over _LN_MAX_BLOCKS blocks (two per CU), but no fewer than
    _LN_MIN_PASSES * unit rows, so that small inputs leave few partial rows
    to fold; rounded up to a multiple of unit. blocks <= _LN_MAX_BLOCKS
    bounds `partial` at 512 * 2 * C floats."""
    gran = C // (16 // elt_bytes)
    lg = next((v for v in (8, 16, 32) if v >= gran), 64)
    unit = 256 // lg
    want = max(_LN_MIN_PASSES * unit, -(-M // _LN_MAX_BLOCKS))
    rpb = -(-want // unit) * unit
    return rpb, -(-M // rpb)


def _steal(fn, like: torch.Tensor) -> torch.Tensor:
    """The flat-gradient slice of a parameter (parallel/flat.py attach_grads)
    if it can take the kernel's output directly, else a fresh tensor."""
    tgt = fn() if fn is not None else None
    return (tgt if tgt is not None and tgt.dtype == like.dtype and tgt.is_cuda
            and tgt.data_ptr() % 16 == 0 else torch.empty_like(like))


class _FusedLNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, need_grad):
        lib = require_lib()
        ctx.gtgt = (getattr(gamma, '_ps_flat_grad_fn', None),
                    getattr(beta, '_ps_flat_grad_fn', None))
        x, gamma, beta = _vec16(x), _vec16(gamma), _vec16(beta)
        N, C, H, W = x.shape
        M = N * H * W
        y = torch.empty_like(x)
        mean = (torch.empty(M, dtype=torch.float32, device=x.device)
                if need_grad else None)
        invstd = torch.empty_like(mean) if need_grad else None
        rpb, blocks = _ln_plan(M, C, x.element_size())
        rc = lib.ps_ln_fwd(
            x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
            mean.data_ptr() if need_grad else 0,
            invstd.data_ptr() if need_grad else 0,
            M, C, float(eps), rpb, blocks, dtype_tag(x.dtype),
            current_stream_ptr())
        if rc:
            raise RuntimeError(f"ps_ln_fwd rejected M={M} C={C} plan="
                               f"{(rpb, blocks)} {x.dtype} (rc={rc})")
        if need_grad:
            ctx.save_for_backward(x, gamma, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = require_lib()
        x, gamma, mean, invstd = ctx.saved_tensors
        dy = _vec16(dy)
        N, C, H, W = x.shape
        M = N * H * W
        dx = torch.empty_like(x)
        dgamma = _steal(ctx.gtgt[0], gamma)
        dbeta = _steal(ctx.gtgt[1], gamma)
        rpb, blocks = _ln_plan(M, C, x.element_size())
        partial = torch.empty(blocks * 2 * C, dtype=torch.float32,
                              device=x.device)
        rc = lib.ps_ln_bwd(
            x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
            invstd.data_ptr(), dx.data_ptr(), dgamma.data_ptr(),
            dbeta.data_ptr(), partial.data_ptr(), M, C, rpb, blocks,
            dtype_tag(x.dtype), current_stream_ptr())
        if rc:
            raise RuntimeError(f"ps_ln_bwd rejected M={M} C={C} plan="
                               f"{(rpb, blocks)} {x.dtype} (rc={rc})")
        return dx, dgamma, dbeta, None, None


class PsLayerNorm2d(nn.Module):
    """LayerNorm over the channels of every pixel of an NCHW-logical 4-D
    input (channels_last in memory), ConvNeXt's norm.

    GPU path: layernorm.hip; PS_LN=0, CPU tensors and shapes outside the
    envelope (C % 8, C > 2048, non-4-D) take F.layer_norm on the permuted
    view, which is also the numerics reference. State dict: weight, bias.
    `kernel_calls` / `fallback_calls` count the forwards of either path."""

    def __init__(self, num_channels: int, eps: float = 1e-6):
        super().__init__()
        self.num_channels = num_channels
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))
        self.kernel_calls = 0
        self.fallback_calls = 0

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if _ln_ok(x, self.weight, self.bias):
            self.kernel_calls += 1
            need_grad = torch.is_grad_enabled() and (
                x.requires_grad or self.weight.requires_grad
                or self.bias.requires_grad)
            return _FusedLNFn.apply(x, self.weight, self.bias, self.eps,
                                    need_grad)
        self.fallback_calls += 1
        y = F.layer_norm(x.permute(0, 2, 3, 1), (self.num_channels,),
                         self.weight, self.bias, self.eps)
        return y.permute(0, 3, 1, 2)

    def extra_repr(self) -> str:
        return f"{self.num_channels}, eps={self.eps}"


class _GELUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = require_lib()
        x = _vec16(x)
        y = torch.empty_like(x)
        rc = lib.ps_gelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(),
                             dtype_tag(x.dtype), current_stream_ptr())
        if rc:
            raise RuntimeError(f"ps_gelu_fwd rejected n={x.numel()} {x.dtype}")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = require_lib()
        (x,) = ctx.saved_tensors
        dy = _vec16(dy)
        dx = torch.empty_like(x)
        rc = lib.ps_gelu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                             x.numel(), dtype_tag(x.dtype),
                             current_stream_ptr())
        if rc:
            raise RuntimeError(f"ps_gelu_bwd rejected n={x.numel()} {x.dtype}")
        return dx


class PsGELU(nn.Module):
    """GELU in the exact erf form. GPU path: layernorm.hip's streaming
    kernels (any shape with numel % 8 == 0; the backward recomputes from the
    saved x); PS_LN=0, CPU tensors and other sizes take F.gelu."""

    def __init__(self):
        super().__init__()
        self.kernel_calls = 0
        self.fallback_calls = 0

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if (_ln_on() and x.is_cuda and x.numel() >= 8 and x.numel() % 8 == 0
                and x.dtype in (torch.bfloat16, torch.float32)):
            self.kernel_calls += 1
            return _GELUFn.apply(x)
        self.fallback_calls += 1
        return F.gelu(x)


class _LayerScaleAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, res, lam):
        lib = require_lib()
        ctx.gtgt = getattr(lam, '_ps_flat_grad_fn', None)
        y, res, lam = _vec16(y), _vec16(res), _vec16(lam)
        N, C, H, W = y.shape
        M = N * H * W
        out = torch.empty_like(y)
        rpb, blocks = _ln_plan(M, C, y.element_size())
        rc = lib.ps_lscale_fwd(y.data_ptr(), res.data_ptr(), lam.data_ptr(),
                               out.data_ptr(), M, C, rpb, blocks,
                               dtype_tag(y.dtype), current_stream_ptr())
        if rc:
            raise RuntimeError(f"ps_lscale_fwd rejected M={M} C={C} plan="
                               f"{(rpb, blocks)} {y.dtype} (rc={rc})")
        ctx.save_for_backward(y, lam)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = require_lib()
        y, lam = ctx.saved_tensors
        dout = _vec16(dout)
        N, C, H, W = y.shape
        M = N * H * W
        dy = torch.empty_like(y)
        dlam = _steal(ctx.gtgt, lam)
        rpb, blocks = _ln_plan(M, C, y.element_size())
        partial = torch.empty(blocks * C, dtype=torch.float32, device=y.device)
        rc = lib.ps_lscale_bwd(y.data_ptr(), dout.data_ptr(), lam.data_ptr(),
                               dy.data_ptr(), dlam.data_ptr(),
                               partial.data_ptr(), M, C, rpb, blocks,
                               dtype_tag(y.dtype), current_stream_ptr())
        if rc:
            raise RuntimeError(f"ps_lscale_bwd rejected M={M} C={C} plan="
                               f"{(rpb, blocks)} {y.dtype} (rc={rc})")
        # the residual's gradient is dout itself, not a copy
        return dy, dout, dlam


class PsLayerScaleAdd(nn.Module):
    """forward(y, residual) == residual + weight[c] * y: the tail of a
    ConvNeXt block, `weight` the learned per-channel layer scale. GPU path:
    layernorm.hip (4-D, C % 8 == 0, C <= 2048); otherwise torch ops."""

    def __init__(self, num_channels: int, init: float = 1e-6):
        super().__init__()
        self.num_channels = num_channels
        self.weight = nn.Parameter(torch.full((num_channels,), float(init)))
        self.kernel_calls = 0
        self.fallback_calls = 0

    def forward(self, y: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
        if (_ln_ok(y, self.weight) and residual.shape == y.shape
                and residual.dtype == y.dtype and residual.device == y.device):
            self.kernel_calls += 1
            return _LayerScaleAddFn.apply(y, residual, self.weight)
        self.fallback_calls += 1
        return residual + self.weight.view(1, -1, 1, 1) * y

    def extra_repr(self) -> str:
        return f"{self.num_channels}"
