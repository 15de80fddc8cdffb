"""PS-side LARS on the flat master buffer, with a device-resident LR schedule.

LARS (You, Gitman, Ginsburg: "Large Batch Training of Convolutional
Networks") scales every tensor's step by the trust ratio
eta*|w| / (|g| + wd*|w| + eps); 1-D tensors (biases, BN affine) get neither
the ratio nor the decay. Parameters never straddle buckets in the flat
layout, so a whole-buffer step, a per-bucket region step and the fused
fan-in's slice step all see whole tensors.

GPU path: three launches per step() whatever the number of tensors
(ops/kernels/lars.hip): per-chunk f64 sums of squares, a per-tensor fold to
the step sizes, the elementwise update with the wire re-pack. The learning
rate is read from an f32 table in device memory through a device step
counter, so a captured hipGraph follows the schedule on replay; no host
sync, no allocation after construction. CPU path: the torch reference of
ops.functional.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops.functional import LarsLayout, lars_norms, lars_step
from .schedule import LRSchedule


class FlatLARS:
    def __init__(self, flat_w: torch.Tensor, segments, schedule: LRSchedule,
                 momentum: float = 0.9, weight_decay: float = 0.0,
                 eta: float = 1e-3, eps: float = 1e-8, start_step: int = 0):
        """segments: (offset, numel, ndim) per parameter, FlatSpace.segments().
        start_step: where the schedule starts (--resume-step)."""
        if flat_w.dtype != torch.float32:
            raise TypeError("master weights must be f32")
        self.w = flat_w
        self.schedule = schedule
        self.momentum = float(momentum)
        self.weight_decay = float(weight_decay)
        self.eta = float(eta)
        self.eps = float(eps)
        self.m = torch.zeros_like(flat_w)
        dev = flat_w.device
        self.layout = LarsLayout(segments, flat_w.numel(), dev)
        self.lr_table = schedule.table(dev)
        self.step_ctr = torch.tensor([int(start_step)], dtype=torch.int64,
                                     device=dev)
        self.lr_cur = torch.tensor([schedule.lr_at(start_step)],
                                   dtype=torch.float32, device=dev)

    @property
    def lr(self) -> float:
        """The learning rate of the last step taken (one host sync)."""
        return float(self.lr_cur)

    @torch.no_grad()
    def step(self, grad_sum: torch.Tensor, grad_scale: float = 1.0,
             wire_out: Optional[torch.Tensor] = None,
             region=None, advance: bool = True) -> None:
        """region=(start, end): update only that flat slice (bucket
        boundaries); pass advance=True exactly once per logical step (first
        bucket): it moves the schedule on by one."""
        lars_norms(self.layout, self.w, grad_sum, self.lr_table,
                   self.step_ctr, self.lr_cur, grad_scale, self.eta,
                   self.weight_decay, self.eps, region, advance)
        lars_step(self.layout, self.w, grad_sum, self.m, self.momentum,
                  grad_scale, wire_out, region)

    def state_dict(self) -> dict:
        return {'momentum_buffer': self.m, 'step': int(self.step_ctr),
                'lr_cur': float(self.lr_cur), 'momentum': self.momentum,
                'weight_decay': self.weight_decay, 'eta': self.eta,
                'eps': self.eps}

    def load_state_dict(self, sd: dict) -> None:
        self.m.copy_(sd['momentum_buffer'])
        self.step_ctr.fill_(int(sd['step']))
        self.lr_cur.fill_(float(sd['lr_cur']))
        self.momentum = sd['momentum']
        self.weight_decay = sd['weight_decay']
        self.eta = sd['eta']
        self.eps = sd['eps']
