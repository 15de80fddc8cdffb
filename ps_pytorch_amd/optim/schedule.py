"""Learning-rate schedules, evaluated per optimizer step.

`LRSchedule.lr_at(step)` is computed in float64 and rounded to f32;
`table(device)` is the f32 table of `total_steps` entries built from it, so
what a host loop sets (`HostLR`, for the optimizers whose kernels take lr by
value) and what a device-side reader indexes (FlatLARS) agree bit for bit.

With w = warmup_steps, t = step - w and span = total_steps - w:

  step < w   lr = base_lr * (step + 1) / w          (linear, from base_lr/w)
  constant   lr = base_lr
  step       lr = base_lr * gamma ** (t // decay_steps)
  poly       lr = base_lr * (1 - t / span) ** 2     (zero at total_steps)
  cosine     lr = base_lr * (1 + cos(pi * t / span)) / 2

Steps at or past total_steps hold the value of the last step.
"""
from __future__ import annotations

import math

import numpy as np
import torch

KINDS = ('constant', 'step', 'poly', 'cosine')


class LRSchedule:
    def __init__(self, base_lr: float, kind: str = 'constant',
                 total_steps: int = 1, warmup_steps: int = 0,
                 decay_steps: int = 0, gamma: float = 0.1):
        if kind not in KINDS:
            raise ValueError(f"unknown LR schedule {kind!r}, one of {KINDS}")
        self.base_lr = float(base_lr)
        self.kind = kind
        self.total_steps = int(total_steps)
        self.warmup_steps = int(warmup_steps)
        self.decay_steps = int(decay_steps)
        self.gamma = float(gamma)
        if self.total_steps < 1:
            raise ValueError("total_steps must be >= 1")
        if self.warmup_steps < 0:
            raise ValueError("warmup_steps must be >= 0")
        if kind == 'step' and self.decay_steps < 1:
            raise ValueError("the step schedule needs decay_steps >= 1")

    @property
    def is_constant(self) -> bool:
        return self.kind == 'constant' and self.warmup_steps == 0

    def lr_at(self, step: int) -> float:
        step = min(max(int(step), 0), self.total_steps - 1)
        w = self.warmup_steps
        if step < w:
            lr = self.base_lr * (step + 1) / w
        else:
            t = step - w
            span = max(self.total_steps - w, 1)
            if self.kind == 'constant':
                lr = self.base_lr
            elif self.kind == 'step':
                lr = self.base_lr * self.gamma ** (t // self.decay_steps)
            elif self.kind == 'poly':
                lr = self.base_lr * (1.0 - t / span) ** 2
            else:
                lr = self.base_lr * 0.5 * (1.0 + math.cos(math.pi * t / span))
        return float(np.float32(lr))

    def table(self, device=None) -> torch.Tensor:
        return torch.tensor([self.lr_at(i) for i in range(self.total_steps)],
                            dtype=torch.float32, device=device)


class HostLR:
    """Drives `optimizer.lr` from a schedule on the eager paths: tick() once
    before every logical step. For FlatSGD / FlatAdam, whose kernels take lr
    by value (which is also why a captured graph cannot follow it)."""

    def __init__(self, optimizer, schedule: LRSchedule, start_step: int = 0):
        self.optimizer = optimizer
        self.schedule = schedule
        self.step = int(start_step)

    def tick(self) -> None:
        self.optimizer.lr = self.schedule.lr_at(self.step)
        self.step += 1
