"""Collective (all-reduce) data-parallel engine — no parameter server.

Reference parity: src/data_parallel_dist/data_parallel_dist.py — the repo's
vendored fork of early torch DistributedDataParallel (param bcast at init
:45-46, 1 MB gradient buckets :70-87, autograd hooks :146-179, per-bucket
reduction on dedicated CUDA streams :211-235, nccl.reduce + dist.all_reduce
:238-264). It is NOT used by the reference's main PS path — it is the repo's
own sketch of collective DP — so here it is built properly, MI355X-first:

  * ONE flat bucketed buffer (parallel/flat.py) instead of ad-hoc coalescing;
    autograd accumulates grads directly into it (no copy before reduce).
  * post-accumulate-grad hooks launch async ncclAllReduce per bucket in
    backward order, overlapped with the rest of backward — RCCL rings over
    all 8 GPUs' xGMI links (vs the PS star, which is bound by rank 0's 7
    incoming links).
  * every rank runs the IDENTICAL fused FlatSGD HIP kernel on a replicated
    f32 master (same summed bytes in -> same bytes out), which also re-packs
    the live bf16 compute params — no weight broadcast per step at all.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from ..ops.loss import cross_entropy as ps_cross_entropy

from ..config import JobConfig, input_shape_of, num_classes_of
from ..models import build_model
from ..optim import build_optimizer
from ..parallel.flat import FlatSpace, prep_model
from ..utils.logging import get_logger

logger = get_logger('ps_pytorch_amd.allreduce')


class AllReduceTrainer:
    def __init__(self, cfg: JobConfig, rank: int, world: int,
                 device: torch.device):
        self.cfg = cfg
        self.rank = rank
        self.world = world
        self.device = device
        self.compute_dtype = (torch.bfloat16
                              if (device.type == 'cuda' and cfg.compute_dtype == 'bf16')
                              else torch.float32)
        self.cur_step = 0
        self.network = None
        self.flat: Optional[FlatSpace] = None
        self._works: list = []

    def build_model(self, num_classes: Optional[int] = None) -> None:
        cfg = self.cfg
        nc = num_classes if num_classes is not None else num_classes_of(cfg.dataset)
        in_ch = input_shape_of(cfg.dataset)[0]
        torch.manual_seed(cfg.seed)
        net = build_model(cfg.network, num_classes=nc, in_channels=in_ch)
        net = prep_model(net, self.device, self.compute_dtype)
        self.network = net
        self.flat = FlatSpace(net, bucket_bytes=int(cfg.bucket_mb * 2 ** 20))
        self.flat.attach_grads(steal=(self.device.type == 'cuda'))
        # init-time param sync (ref data_parallel_dist.py:45-46) — one flat
        # broadcast (ranks are identically seeded; this guards non-determinism)
        if dist.is_initialized() and self.world > 1:
            dist.broadcast(self.flat.flat_w, src=0)
        self.master_w = self.flat.flat_w.detach().to(torch.float32).clone()
        # this engine runs the replicated FlatSGD whatever --optimizer says,
        # except lars
        name = 'lars' if getattr(cfg, 'optimizer', 'sgd') == 'lars' else 'sgd'
        self.optimizer, self._host_lr = build_optimizer(
            cfg, self.master_w, self.flat, name=name)
        if cfg.overlap:
            self._install_hooks()

    # -- overlap engine: same bucket bookkeeping as the PS worker --

    def _install_hooks(self) -> None:
        self._param_bucket = {}
        self._bucket_nparams = [0] * len(self.flat.buckets)
        for b in self.flat.buckets:
            for pid in b.param_ids:
                self._param_bucket[pid] = b.index
                if self.flat.params[pid].requires_grad:
                    self._bucket_nparams[b.index] += 1
        self._pending = list(self._bucket_nparams)
        self._ready = [False] * len(self.flat.buckets)
        self._next_launch = 0
        for pid, p in enumerate(self.flat.params):
            if p.requires_grad:
                p.register_post_accumulate_grad_hook(self._make_hook(pid))

    def _make_hook(self, pid: int):
        def hook(_param):
            self.flat.ensure_grad_in_flat(pid)
            bi = self._param_bucket[pid]
            self._pending[bi] -= 1
            if self._pending[bi] == 0:
                self._ready[bi] = True
                self._flush_ready()
        return hook

    def _flush_ready(self) -> None:
        while (self._next_launch < len(self._ready)
               and self._ready[self._next_launch]):
            self._push(self.flat.buckets[self._next_launch])
            self._next_launch += 1

    def _push(self, b) -> None:
        if dist.is_initialized() and self.world > 1:
            self._works.append(dist.all_reduce(
                self.flat.grad_slice(b), op=dist.ReduceOp.SUM, async_op=True))

    def _reset(self) -> None:
        self._next_launch = 0
        if self.cfg.overlap:
            self._pending = list(self._bucket_nparams)
            self._ready = [False] * len(self.flat.buckets)

    def train_step(self, data: torch.Tensor, target: torch.Tensor):
        if data.dim() == 4 and data.is_cuda:
            data = data.contiguous(memory_format=torch.channels_last)
        self.flat.zero_grads()
        self._reset()
        out = self.network(data)
        loss = ps_cross_entropy(out, target)
        loss.backward()
        if self.cfg.overlap:
            self._flush_ready()
        else:
            self.flat.harvest_grads()   # steal mode: catch fallback grads
        for b in self.flat.buckets[self._next_launch:]:
            self._push(b)
        self._next_launch = len(self.flat.buckets)
        for w in self._works:
            w.wait()
        self._works.clear()
        if self._host_lr is not None:
            self._host_lr.tick()
        # replicated fused update: summed grads / world, re-pack live params
        self.optimizer.step(self.flat.flat_g, grad_scale=1.0 / self.world,
                            wire_out=self.flat.flat_w)
        self.cur_step += 1
        return loss.detach()
