"""Single-machine trainer — the scalability yardstick and correctness oracle.

Reference parity: src/nn_ops.py:29-106 (NN_Trainer.build_model /
train_and_validate / validate) + src/single_machine.py. Uses the SAME engine
pieces as the distributed path (FlatSpace views + FlatSGD fused update) so
the 1-GPU bench measures the framework, not a different code path:
master weights f32, compute dtype bf16 on GPU (f32 on CPU), one fused
update kernel per step.
"""
from __future__ import annotations

import time
from typing import Optional

import torch
import torch.nn as nn

from .ops.loss import cross_entropy as ps_cross_entropy

from .config import JobConfig, num_classes_of, input_shape_of
from .models import build_model
from .optim import build_optimizer
from .parallel.flat import FlatSpace, prep_model
from .ops.metrics import MetricAccumulator
from .utils.logging import get_logger

logger = get_logger('ps_pytorch_amd.trainer')


class NNTrainer:
    def __init__(self, cfg: JobConfig, device: Optional[torch.device] = None):
        self.cfg = cfg
        if device is None:
            device = torch.device('cuda' if (cfg.enable_gpu and torch.cuda.is_available())
                                  else 'cpu')
        self.device = device
        self.compute_dtype = (torch.bfloat16 if (device.type == 'cuda' and
                                                 cfg.compute_dtype == 'bf16')
                              else torch.float32)
        self.network: Optional[nn.Module] = None
        self.flat: Optional[FlatSpace] = None
        self.optimizer = None
        self.cur_step = 0
        # --train-metrics: loss / prec@k of the training batches, summed on
        # the device inside the step (captured with it) and read at log time
        self.train_metrics = (MetricAccumulator(device, ks=(1, 5))
                              if getattr(cfg, 'train_metrics', False) else None)

    def build_model(self, num_classes: Optional[int] = None) -> None:
        cfg = self.cfg
        nc = num_classes if num_classes is not None else num_classes_of(cfg.dataset)
        in_ch = input_shape_of(cfg.dataset)[0]
        torch.manual_seed(cfg.seed)
        net = build_model(cfg.network, num_classes=nc, in_channels=in_ch)
        net = prep_model(net, self.device, self.compute_dtype)
        self.network = net
        self.flat = FlatSpace(net, bucket_bytes=int(cfg.bucket_mb * 2 ** 20))
        if getattr(cfg, 'resume_step', 0):
            from .utils.checkpoint import load_model_step
            load_model_step(net, cfg.train_dir, cfg.resume_step, strict=False)
        # f32 master copy + fused update; flat_g is the "wire" (local = trivially summed)
        self.master_w = self.flat.flat_w.detach().to(torch.float32).clone()
        # host_lr: the schedule driver of the by-value-lr optimizers (None
        # for a constant schedule, and for lars, which reads it on device)
        self.optimizer, self._host_lr = build_optimizer(cfg, self.master_w,
                                                        self.flat)
        # steal mode on GPU: Ps ops write grads into flat_g directly (no
        # per-param AccumulateGrad add kernels); view mode on CPU
        self.flat.attach_grads(steal=(self.device.type == 'cuda'))

    def _loss(self, data, target):
        out = self.network(data)
        return ps_cross_entropy(out, target, metrics=self.train_metrics), out

    def read_train_metrics(self):
        """Loss / prec@k of the training batches since the last read (one
        host sync), then an asynchronous reset; None without
        --train-metrics."""
        if self.train_metrics is None:
            return None
        res = self.train_metrics.result()
        self.train_metrics.reset()
        return res

    def _step_body(self, data, target) -> torch.Tensor:
        self.flat.zero_grads()
        loss, _ = self._loss(data, target)
        loss.backward()
        self.flat.harvest_grads()   # steal mode: catch torch-fallback grads
        if self._host_lr is not None:
            self._host_lr.tick()
        # fused: master update + re-pack into the live (possibly bf16) params
        self.optimizer.step(self.flat.flat_g, grad_scale=1.0,
                            wire_out=self.flat.flat_w)
        return loss.detach()

    def train_step(self, data, target) -> float:
        """forward/backward/update; returns loss."""
        if data.dim() == 4 and data.is_cuda:
            data = data.contiguous(memory_format=torch.channels_last)
        loss = self._step_body(data, target)
        self.cur_step += 1
        return float(loss)

    # ---- hipGraph-captured step (single-GPU hot path) ----
    # The whole step (zero -> forward -> backward -> fused update) replays as
    # ONE hipGraph: ~580 kernel dispatches/step collapse to one launch,
    # removing host launch overhead and inter-kernel gaps (MI355X guide:
    # 'graph-replay-floor'). Static input buffers; loss read lazily.

    def enable_graph(self, example_x: torch.Tensor,
                     example_y: torch.Tensor) -> bool:
        if self.device.type != 'cuda':
            return False
        if self._refuse_graph():
            return False
        example_x = example_x.contiguous(memory_format=torch.channels_last) \
            if example_x.dim() == 4 else example_x
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):     # warmup allocs/algos outside capture
                    self._step_body(example_x, example_y)
            torch.cuda.current_stream().wait_stream(side)
            if self.train_metrics is not None:
                # the warmup steps above are not counted in cur_step
                self.train_metrics.reset()
            self._gx = example_x.clone()
            self._gy = example_y.clone()
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._gloss = self._step_body(self._gx, self._gy)
            return True
        except Exception as e:   # pragma: no cover - depends on runtime
            import warnings
            warnings.warn(f"hipGraph capture failed, staying eager: {e}")
            self._graph = None
            return False

    def _refuse_graph(self) -> bool:
        """The sgd / adam kernels take lr by value, so a captured step would
        replay the learning rate of the capture for ever: with a
        non-constant schedule stay eager (lars reads its schedule on the
        device and captures)."""
        if self._host_lr is None:
            return False
        import warnings
        warnings.warn(f"--lr-schedule {self.cfg.lr_schedule} with "
                      f"--optimizer {self.cfg.optimizer} cannot be captured "
                      "into a graph (lr is a by-value kernel argument); "
                      "staying eager. --optimizer lars follows the schedule "
                      "under capture")
        return True

    def graph_step(self, data: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """Replay the captured step on new data; returns the (device) loss
        tensor — read it only when needed to avoid a sync per step."""
        self._gx.copy_(data, non_blocking=True)
        self._gy.copy_(target, non_blocking=True)
        return self._replay()

    def _replay(self) -> torch.Tensor:
        self._graph.replay()
        # host-side BN batch counters don't tick during replay (host code
        # doesn't run); keep them canonical here
        from .ops.modules import PsBatchNorm2d
        for m in self.network.modules():
            if isinstance(m, PsBatchNorm2d):
                m._nbt_host = getattr(m, '_nbt_host', 0) + 1
        self.cur_step += 1
        return self._gloss

    # ---- captured step INCLUDING the data loader (real data) ----
    # An rng='philox' RealResidentLoader produces a batch with one kernel
    # whose randomness is a device-side counter, so loader + step capture as
    # one graph: loader kernel -> static (_gx, _gy) -> _step_body. Per replay
    # the host only copies the next B dataset indices into the loader's
    # static index buffer (D2D, ordered on the stream). The 3 warmup steps
    # consume real batches, so `enable_graph_loader` + k `graph_loader_step`s
    # see the batch sequence of 3 + k eager next_batch()/train_step() calls.

    def enable_graph_loader(self, loader) -> bool:
        if self.device.type != 'cuda':
            return False
        if self._refuse_graph():
            return False
        ds = loader.dataset
        if ds.dtype != self.compute_dtype:
            raise ValueError(f"loader yields {ds.dtype}, the trainer computes "
                             f"in {self.compute_dtype}")
        loader.bind_static()             # raises unless a GPU philox loader
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):     # warmup allocs/algos outside capture
                    self._step_body(*loader.next_batch())
                    self.cur_step += 1
            torch.cuda.current_stream().wait_stream(side)
            B = loader.batch_size
            self._gx = torch.empty((B,) + tuple(ds.shape), dtype=ds.dtype,
                                   device=self.device,
                                   memory_format=torch.channels_last)
            self._gy = torch.empty(B, dtype=torch.int64, device=self.device)
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                loader.fill_static(self._gx, self._gy)
                self._gloss = self._step_body(self._gx, self._gy)
            self._gloader = loader
            return True
        except Exception as e:   # pragma: no cover - depends on runtime
            import warnings
            warnings.warn(f"hipGraph capture failed, staying eager: {e}")
            self._graph = None
            return False

    def graph_loader_step(self) -> torch.Tensor:
        """Replay the captured loader + step on the loader's next batch;
        returns the (device) loss tensor, as graph_step does."""
        self._gloader.stage_next()
        return self._replay()

    def train_and_validate(self, train_loader, test_loader,
                           max_steps: Optional[int] = None) -> None:
        cfg = self.cfg
        max_steps = max_steps or cfg.max_steps
        self.network.train()
        for epoch in range(cfg.epochs):
            for batch_idx, (data, target) in enumerate(train_loader):
                t0 = time.time()
                data = data.to(self.device, self.compute_dtype)
                target = target.to(self.device)
                loss = self.train_step(data, target)
                if self.cur_step % cfg.log_interval == 0:
                    line = 'Step: %d, Epoch: %d, Loss: %.4f, Time: %.4f' % (
                        self.cur_step, epoch, loss, time.time() - t0)
                    tm = self.read_train_metrics()
                    if tm is not None:   # the steps since the last log line
                        line += ', Prec@1: %.2f, Prec@5: %.2f' % (
                            tm.prec[1], tm.prec[5])
                    logger.info(line)
                if self.cur_step >= max_steps:
                    return
            self.validate(test_loader)

    @torch.no_grad()
    def validate(self, test_loader) -> float:
        self.network.eval()
        acc = MetricAccumulator(self.device, ks=(1, 5))
        for data, target in test_loader:
            data = data.to(self.device, self.compute_dtype)
            target = target.to(self.device)
            acc.update(self.network(data), target)
        res = acc.result()     # the one host sync of the evaluation
        self.network.train()
        logger.info('Validation: loss %.4f, prec@1 %.2f, prec@5 %.2f',
                    res.loss, res.prec[1], res.prec[5])
        return res.prec[1]
