"""ctypes loader for the in-tree gfx950 kernel library.

Policy (per-framework contract): on a GPU box the HIP path is THE path — if
the extension is missing or fails to load while CUDA/ROCm devices are
visible, ops raise immediately rather than falling back to eager torch.
CPU-only processes (tests, the build container) use torch fallbacks in
ops.functional.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional

import torch

_LIB: Optional[ctypes.CDLL] = None
_LIB_ERR: Optional[str] = None

PS_F32 = 0
PS_BF16 = 1

_DTYPE_TAG = {torch.float32: PS_F32, torch.bfloat16: PS_BF16}

# entry points of the f32 kernel family (--compute-dtype fp32 on the GPU)
F32_SYMBOLS = (
    'ps_conv_fwd_f32', 'ps_conv_dgrad_f32', 'ps_conv_wgrad_f32',
    'ps_conv_bias_grad_f32',
    'ps_maxpool_fwd_f32', 'ps_maxpool_bwd_f32',
    'ps_gavgpool_fwd_f32', 'ps_gavgpool_bwd_f32',
    'ps_softmax_ce_fwd_f32', 'ps_softmax_ce_bwd_f32',
    'ps_ce_metrics_f32', 'ps_softmax_ce_fwd_metrics_f32',
)


def _so_path() -> Path:
    return Path(__file__).resolve().parent / "libps_hip.so"


def _try_load() -> None:
    global _LIB, _LIB_ERR
    if _LIB is not None or _LIB_ERR is not None:
        return
    p = _so_path()
    if not p.exists():
        _LIB_ERR = f"{p} not built (run ps_pytorch_amd.ops.build or __graft_entry__.build())"
        return
    try:
        lib = ctypes.CDLL(str(p))
        lib.ps_fused_sgd.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_long, ctypes.c_float, ctypes.c_float, ctypes.c_float,
            ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.ps_pack_bf16.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_long, ctypes.c_void_p]
        lib.ps_unpack_bf16.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_long, ctypes.c_void_p]
        lib.ps_pack_q8.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
        # error-feedback packs: the f32 residual rides after src
        lib.ps_pack_q8_ef.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_long,
                                      ctypes.c_int, ctypes.c_void_p]
        lib.ps_pack_bf16_ef.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_long,
                                        ctypes.c_void_p]
        lib.ps_unpack_q8.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
        lib.ps_acc.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
        # block top-k codec (topk.hip): payload, src, residual, n, k,
        # src_dtype, stream / dst, payload, n, k, accumulate, stream; both
        # return nonzero for a k they have no kernel for
        lib.ps_pack_topk_ef.argtypes = [ctypes.c_void_p] * 3 + [
            ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.ps_pack_topk_ef.restype = ctypes.c_int
        lib.ps_unpack_topk.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_long, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_void_p]
        lib.ps_unpack_topk.restype = ctypes.c_int
        # rank-ordered fan-in (fanin.hip): dst, srcs (host array of device
        # pointers), nsrc, codec, k, n, stream / w, m, wire, wire_dtype,
        # srcs, nsrc, codec, k, n, lr, mu, wd, scale, nesterov, stream;
        # both return nonzero and launch nothing for arguments they reject
        lib.ps_fanin_reduce.argtypes = [
            ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_void_p]
        lib.ps_fanin_reduce.restype = ctypes.c_int
        lib.ps_fanin_sgd.argtypes = [ctypes.c_void_p] * 3 + [
            ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_long] + [
            ctypes.c_float] * 4 + [ctypes.c_int, ctypes.c_void_p]
        lib.ps_fanin_sgd.restype = ctypes.c_int
        lib.ps_conv_fwd.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 11 + [ctypes.c_void_p]
        lib.ps_conv_dgrad.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 11 + [ctypes.c_void_p]
        lib.ps_conv_wgrad.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 12 + [ctypes.c_void_p]
        # test hook: dout, in, partial, Nb, H, W, C, K, P, Q, split,
        # variant (0 register kernel, 1 LDS-ring kernel), stream; one
        # row-halo wgrad kernel alone, no reduce; nonzero = shape not taken
        lib.ps_conv_wgrad_row_variant.argtypes = [ctypes.c_void_p] * 3 + [
            ctypes.c_int] * 9 + [ctypes.c_void_p]
        lib.ps_conv_wgrad_row_variant.restype = ctypes.c_int
        # test hook: dgrad (0 fwd, 1 dgrad), src, wgt (dgrad: wT), bias,
        # dst, carry, Nb, H, W, C, K, P, Q, variant (0 generic GEMM kernel,
        # 1 halo-resident 3x3 kernel), stream; one launch alone; nonzero =
        # not a shape the halo kernel takes, nothing launched
        lib.ps_conv_halo_variant.argtypes = [ctypes.c_int] + [
            ctypes.c_void_p] * 5 + [ctypes.c_int] * 8 + [ctypes.c_void_p]
        lib.ps_conv_halo_variant.restype = ctypes.c_int
        lib.ps_conv_bias_grad.argtypes = [ctypes.c_void_p] * 3 + [
            ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
        lib.ps_wt_transpose.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.ps_fused_adam.argtypes = [ctypes.c_void_p] * 6 + [
            ctypes.c_long] + [ctypes.c_float] * 7 + [
            ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        # fused LARS (lars.hip). norms: w, g, g_dtype, chunk_start,
        # chunk_len, chunk0, nchunk, seg_chunk0, seg_adapt, seg0, nseg,
        # partial, seg_sums, local_lr, wd_seg, lr_table, T, step_ctr, lr_cur,
        # advance, grad_scale, eta, wd, eps (f64), stream / update: w, g, m,
        # wire, g_dtype, wire_dtype, chunk_start, chunk_seg, chunk0, nchunk,
        # local_lr, wd_seg, mu, scale, stream; nonzero = rejected, no launch
        lib.ps_lars_norms.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_int] + [ctypes.c_double] * 4 + [
            ctypes.c_void_p]
        lib.ps_lars_norms.restype = ctypes.c_int
        lib.ps_lars_update.argtypes = [ctypes.c_void_p] * 4 + [
            ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
        lib.ps_lars_update.restype = ctypes.c_int
        lib.ps_bn_fwd.argtypes = [ctypes.c_void_p] * 13 + [
            ctypes.c_int,
            ctypes.c_long, ctypes.c_long, ctypes.c_float, ctypes.c_float,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.ps_bn_bwd.argtypes = [ctypes.c_void_p] * 12 + [
            ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int,
            ctypes.c_void_p]
        lib.ps_softmax_ce_fwd.argtypes = [ctypes.c_void_p] * 5 + [
            ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
        lib.ps_softmax_ce_bwd.argtypes = [ctypes.c_void_p] * 5 + [
            ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
        # fused loss + prec@k (metrics.hip). eval: state, row_ws, rank,
        # logits, target, M, C, nk, k0..k3, stream; the training entry
        # carries loss, lse in front (the ps_softmax_ce_fwd outputs)
        lib.ps_ce_metrics.argtypes = [ctypes.c_void_p] * 5 + [
            ctypes.c_long] + [ctypes.c_int] * 6 + [ctypes.c_void_p]
        lib.ps_softmax_ce_fwd_metrics.argtypes = [ctypes.c_void_p] * 7 + [
            ctypes.c_long] + [ctypes.c_int] * 6 + [ctypes.c_void_p]
        lib.ps_maxpool_fwd.argtypes = [ctypes.c_void_p] * 3 + [
            ctypes.c_int] * 10 + [ctypes.c_void_p]
        lib.ps_maxpool_bwd.argtypes = [ctypes.c_void_p] * 3 + [
            ctypes.c_int] * 10 + [ctypes.c_void_p]
        lib.ps_gavgpool_fwd.argtypes = [ctypes.c_void_p] * 2 + [
            ctypes.c_int] * 3 + [ctypes.c_void_p]
        lib.ps_gavgpool_bwd.argtypes = [ctypes.c_void_p] * 2 + [
            ctypes.c_int] * 3 + [ctypes.c_void_p]
        lib.ps_pad4.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
        lib.ps_padc.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                ctypes.c_void_p]
        # y, mask, x, n, dtype, relu, thr, scale, seed, salt_stream,
        # step_ptr, stream
        lib.ps_act_drop_fwd.argtypes = [ctypes.c_void_p] * 3 + [
            ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
            ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_void_p]
        lib.ps_act_drop_bwd.argtypes = [ctypes.c_void_p] * 3 + [
            ctypes.c_long, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
        lib.ps_rng_advance.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        # out, out_y, x_u8, y, idx, B, C, H, W, dtype, pad, reflect, hflip,
        # mean255 (host), inv_std255 (host), seed, stream, step_ptr, stream
        lib.ps_augment_batch.argtypes = [ctypes.c_void_p] * 5 + [
            ctypes.c_long] + [ctypes.c_int] * 7 + [
            ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
            ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p,
            ctypes.c_void_p]
        # f32 family (conv_f32.hip + the f32 twins in pool / softmaxce)
        lib.ps_conv_fwd_f32.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 11 + [ctypes.c_void_p]
        lib.ps_conv_dgrad_f32.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 11 + [ctypes.c_void_p]
        lib.ps_conv_wgrad_f32.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 12 + [ctypes.c_void_p]
        lib.ps_conv_bias_grad_f32.argtypes = [ctypes.c_void_p] * 3 + [
            ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
        lib.ps_softmax_ce_fwd_f32.argtypes = lib.ps_softmax_ce_fwd.argtypes
        lib.ps_softmax_ce_bwd_f32.argtypes = lib.ps_softmax_ce_bwd.argtypes
        lib.ps_ce_metrics_f32.argtypes = lib.ps_ce_metrics.argtypes
        lib.ps_softmax_ce_fwd_metrics_f32.argtypes = \
            lib.ps_softmax_ce_fwd_metrics.argtypes
        lib.ps_maxpool_fwd_f32.argtypes = lib.ps_maxpool_fwd.argtypes
        lib.ps_maxpool_bwd_f32.argtypes = lib.ps_maxpool_bwd.argtypes
        lib.ps_gavgpool_fwd_f32.argtypes = lib.ps_gavgpool_fwd.argtypes
        lib.ps_gavgpool_bwd_f32.argtypes = lib.ps_gavgpool_bwd.argtypes
        _LIB = lib
    except OSError as e:  # pragma: no cover
        _LIB_ERR = str(e)


def lib_or_none() -> Optional[ctypes.CDLL]:
    _try_load()
    return _LIB


def require_lib() -> ctypes.CDLL:
    """The GPU compute path: loud failure if the native library is absent."""
    _try_load()
    if _LIB is None:
        raise RuntimeError(
            f"ps_pytorch_amd HIP extension unavailable on a GPU host: {_LIB_ERR}")
    return _LIB


def dtype_tag(dt: torch.dtype) -> int:
    try:
        return _DTYPE_TAG[dt]
    except KeyError:
        raise TypeError(f"unsupported wire/compute dtype {dt}")


def current_stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


from . import functional  # noqa: E402,F401
