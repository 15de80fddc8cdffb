"""Fused softmax cross-entropy on the in-tree CDNA4 kernels
(ops/kernels/softmaxce.hip). Mean reduction, f32 loss from bf16 or f32
logits.

Replaces the at::native softmax/nll pair the reference reaches through
nn.CrossEntropyLoss (ref: src/distributed_worker.py:98, nn_ops.py:60) on
the GPU hot path; CPU path is F.cross_entropy on f32 (the reference)."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import require_lib, current_stream_ptr
from . import conv as _conv
from . import metrics as _metrics

_ENABLED = os.environ.get('PS_CE', '1') != '0'


class _SoftmaxCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        lib = require_lib()
        x = logits.contiguous()
        t = target.contiguous()
        if t.dtype != torch.int64:
            t = t.to(torch.int64)
        M, C = x.shape
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        # the f32 twin keeps its row workspaces in f64 (softmaxce.hip)
        f32 = x.dtype == torch.float32
        ws_dt = torch.float64 if f32 else torch.float32
        lse = torch.empty(M, dtype=ws_dt, device=x.device)
        row_ws = torch.empty(M, dtype=ws_dt, device=x.device)
        fwd = lib.ps_softmax_ce_fwd_f32 if f32 else lib.ps_softmax_ce_fwd
        fwd(loss.data_ptr(), lse.data_ptr(),
                              row_ws.data_ptr(), x.data_ptr(), t.data_ptr(),
                              M, C, current_stream_ptr())
        ctx.save_for_backward(x, lse, t)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        lib = require_lib()
        x, lse, t = ctx.saved_tensors
        M, C = x.shape
        dl = dloss.reshape(1).to(device=x.device, dtype=torch.float32) \
                  .contiguous()
        dx = torch.empty_like(x)
        bwd = (lib.ps_softmax_ce_bwd_f32 if x.dtype == torch.float32
               else lib.ps_softmax_ce_bwd)
        bwd(dx.data_ptr(), x.data_ptr(), lse.data_ptr(),
                              t.data_ptr(), dl.data_ptr(), M, C,
                              current_stream_ptr())
        return dx, None


class _SoftmaxCEMetricsFn(torch.autograd.Function):
    """_SoftmaxCEFn whose forward also adds the batch's loss sum and prec@k
    hit counts into a MetricAccumulator's state, in the same pass over the
    logits (ps_softmax_ce_fwd_metrics). loss / lse equal _SoftmaxCEFn's bit
    for bit; backward is the same kernel."""

    @staticmethod
    def forward(ctx, logits, target, metrics):
        lib = require_lib()
        x = logits.contiguous()
        t = target.contiguous()
        if t.dtype != torch.int64:
            t = t.to(torch.int64)
        M, C = x.shape
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        f32 = x.dtype == torch.float32
        ws_dt = torch.float64 if f32 else torch.float32
        lse = torch.empty(M, dtype=ws_dt, device=x.device)
        row_ws = torch.empty(M, dtype=ws_dt, device=x.device)
        rank = torch.empty(M, dtype=torch.int32, device=x.device)
        ks = metrics.ks
        fwd = (lib.ps_softmax_ce_fwd_metrics_f32 if f32
               else lib.ps_softmax_ce_fwd_metrics)
        fwd(loss.data_ptr(), lse.data_ptr(), row_ws.data_ptr(),
            rank.data_ptr(), metrics.state.data_ptr(), x.data_ptr(),
            t.data_ptr(), M, C, len(ks), *_metrics._k4(ks),
            current_stream_ptr())
        ctx.save_for_backward(x, lse, t)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        return _SoftmaxCEFn.backward(ctx, dloss) + (None,)


def cross_entropy(logits: torch.Tensor, target: torch.Tensor,
                  metrics=None) -> torch.Tensor:
    """Mean-reduced CE; fused GPU kernel for bf16 / f32 [M, C] logits. With a
    MetricAccumulator in `metrics` the batch's loss sum and prec@k counts are
    added to it on the way (no host sync) and the returned loss is the same."""
    fused = (_ENABLED and logits.is_cuda and logits.dim() == 2
             and _conv._dtype_ok(logits.dtype))
    if metrics is not None:
        if fused and _metrics._use_kernel(logits):
            return _SoftmaxCEMetricsFn.apply(logits, target, metrics)
        metrics.update(logits, target)
    if fused:
        return _SoftmaxCEFn.apply(logits, target)
    return F.cross_entropy(logits.float(), target)
