"""Fused on-device loss + prec@k on the in-tree CDNA4 kernels
(ops/kernels/metrics.hip): per batch two kernels and no host sync, against
the F.cross_entropy + topk/eq/expand/sum chain with three float() syncs the
evaluation loops used to run (ref: nn_ops.py:94-106,
distributed_evaluator.py:90-106).

The rank / invalid-row rule is functional.ce_topk_reference, which is also
the CPU path and the oracle of the kernel tests. GPU + [M, C] + bf16/f32
logits go to the kernels; anything else, or PS_METRICS=0 (read at import, for
A/B), to the oracle in torch ops. PS_F32=0 sends f32 logits there as in the
other ops."""
from __future__ import annotations

import dataclasses
import os
from typing import Dict

import torch

from . import require_lib, current_stream_ptr
from . import conv as _conv
from .functional import ce_topk_reference, check_ks
from ..utils.logging import get_logger

logger = get_logger('ps_pytorch_amd.metrics')

_ENABLED = os.environ.get('PS_METRICS', '1') != '0'

# state buffer slots (8 bytes each): f64 loss sum, i64 valid rows, i64 invalid
# rows, then i64 hits per k
_SLOT_LOSS, _SLOT_ROWS, _SLOT_INVALID, _SLOT_HITS = 0, 1, 2, 3


def _use_kernel(logits: torch.Tensor) -> bool:
    return (_ENABLED and logits.is_cuda and logits.dim() == 2
            and _conv._dtype_ok(logits.dtype))


def _new_state(device, nk: int) -> torch.Tensor:
    return torch.zeros(_SLOT_HITS + nk, dtype=torch.int64, device=device)


def _prep(logits: torch.Tensor, target: torch.Tensor):
    x = logits.detach().contiguous()
    t = target.contiguous()
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    if t.numel() != x.shape[0]:
        raise ValueError(f"{t.numel()} targets for {x.shape[0]} rows")
    return x, t


def _k4(ks):
    return list(ks) + [1] * (4 - len(ks))


def _accumulate(state: torch.Tensor, logits: torch.Tensor,
                target: torch.Tensor, ks) -> None:
    """state += this batch's totals; no host sync on either path."""
    if _use_kernel(logits):
        lib = require_lib()
        x, t = _prep(logits, target)
        M, C = x.shape
        f32 = x.dtype == torch.float32
        row_ws = torch.empty(M, dtype=torch.float64 if f32 else torch.float32,
                             device=x.device)
        rank = torch.empty(M, dtype=torch.int32, device=x.device)
        fn = lib.ps_ce_metrics_f32 if f32 else lib.ps_ce_metrics
        fn(state.data_ptr(), row_ws.data_ptr(), rank.data_ptr(),
           x.data_ptr(), t.data_ptr(), M, C, len(ks), *_k4(ks),
           current_stream_ptr())
        return
    loss_sum, hits, rows, invalid = ce_topk_reference(logits, target, ks)
    state[_SLOT_LOSS:_SLOT_LOSS + 1].view(torch.float64).add_(loss_sum)
    state[_SLOT_ROWS].add_(rows)
    state[_SLOT_INVALID].add_(invalid)
    state[_SLOT_HITS:].add_(hits)


def _split(state: torch.Tensor):
    return (state[_SLOT_LOSS:_SLOT_LOSS + 1].view(torch.float64)[0],
            state[_SLOT_HITS:], state[_SLOT_ROWS], state[_SLOT_INVALID])


def ce_topk(logits: torch.Tensor, target: torch.Tensor, ks=(1, 5)):
    """(loss_sum f64, hits i64 [len(ks)], rows, invalid) of one batch as
    device tensors; `rows` counts the valid rows."""
    ks = check_ks(ks)
    if logits.dim() != 2:
        raise ValueError(f"logits must be [M, C], got {tuple(logits.shape)}")
    state = _new_state(logits.device, len(ks))
    _accumulate(state, logits, target, ks)
    return _split(state)


@dataclasses.dataclass
class MetricResult:
    loss: float                 # loss sum / valid rows
    prec: Dict[int, float]      # k -> percent of valid rows
    rows: int                   # valid rows
    invalid: int                # rows whose target was outside [0, C)


class MetricAccumulator:
    """Running loss / prec@k over batches in one small device buffer.
    update() and reset() enqueue work only (update is capturable into a
    hipGraph); result() is the one host sync."""

    def __init__(self, device, ks=(1, 5)):
        self.ks = check_ks(ks)
        self.device = torch.device(device)
        self.state = _new_state(self.device, len(self.ks))

    def update(self, logits: torch.Tensor, target: torch.Tensor) -> None:
        if logits.dim() != 2:
            raise ValueError(f"logits must be [M, C], got "
                             f"{tuple(logits.shape)}")
        _accumulate(self.state, logits, target, self.ks)

    def reset(self) -> None:
        self.state.zero_()

    def result(self) -> MetricResult:
        s = self.state.cpu()
        loss_sum = float(s[:1].view(torch.float64)[0])
        rows, invalid = int(s[_SLOT_ROWS]), int(s[_SLOT_INVALID])
        if invalid:
            logger.warning('%d rows with a target outside the class range '
                           'were left out of loss and precision', invalid)
        den = max(rows, 1)
        prec = {k: 100.0 * int(s[_SLOT_HITS + i]) / den
                for i, k in enumerate(self.ks)}
        return MetricResult(loss_sum / den, prec, rows, invalid)
