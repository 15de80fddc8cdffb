#!/usr/bin/env python
"""Per-batch cost of an evaluation loop's metric work: the fused loss +
prec@k kernels against the torch paths.

  python tools/metrics_bench.py [--batches 1000] [--graph-batches 200]
                                [--warmup 20] [--rounds 5]
                                [--shapes 1000x10,1000x100,1024x1000]
  python tools/metrics_bench.py --trace fused|oracle|legacy [--shape 1000x10]
                                [--dtype bf16|fp32] [--batches 20]

Variants, each on `--sets` rotating logits/target pairs already on the GPU
(the model's forward pass is not part of the figure):

  fused   MetricAccumulator.update per batch on the in-tree kernels
          (ops/kernels/metrics.hip), one result() after the loop
  oracle  the same calls with the kernels switched off, what PS_METRICS=0
          selects: functional.ce_topk_reference in torch ops, no sync per
          batch either
  legacy  what the evaluation loops ran before the accumulator:
          F.cross_entropy(reduction='sum') + utils.metrics.accuracy and three
          float() host syncs per batch

Two figures per variant, the median of `--rounds` alternating rounds:
  wall_us    host clock around the loop of `--batches` batches, ending in
             the loop's final sync, per batch: what the evaluation loop pays,
             launch overhead included
  device_us  HIP events around one replay of `--graph-batches` batches of
             the same loop captured as a hipGraph, per batch (fused and
             oracle; legacy synchronises per batch and cannot be captured)

--trace runs one variant alone for a few batches, for a
`rocprofv3 --kernel-trace --stats -- python tools/metrics_bench.py --trace X`
run of its own. Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ps_pytorch_amd.ops import metrics as M  # noqa: E402
from ps_pytorch_amd.ops import require_lib  # noqa: E402
from ps_pytorch_amd.utils.metrics import accuracy  # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}


def make_sets(rows, classes, dtype, nsets):
    g = torch.Generator(device='cuda').manual_seed(rows + classes)
    return [((torch.randn(rows, classes, device='cuda', generator=g) * 3)
             .to(dtype),
             torch.randint(0, classes, (rows,), device='cuda', generator=g))
            for _ in range(nsets)]


class Loop:
    """One evaluation's metric work over `batches` batches."""

    def __init__(self, variant, sets, batches):
        self.variant, self.sets, self.batches = variant, sets, batches
        self.acc = M.MetricAccumulator('cuda', ks=(1, 5))
        self.graph = None

    def _updates(self):
        M._ENABLED = self.variant == 'fused'
        try:
            for i in range(self.batches):
                x, t = self.sets[i % len(self.sets)]
                self.acc.update(x, t)
        finally:
            M._ENABLED = True

    def run(self):
        """The whole loop including its host syncs; returns (loss, p1, p5)."""
        if self.variant == 'legacy':
            tot = loss = p1s = p5s = 0.0
            for i in range(self.batches):
                x, t = self.sets[i % len(self.sets)]
                loss += float(F.cross_entropy(x, t, reduction='sum'))
                p1, p5 = accuracy(x, t, topk=(1, min(5, x.shape[1])))
                p1s += float(p1) * len(t)
                p5s += float(p5) * len(t)
                tot += len(t)
            return loss / tot, p1s / tot, p5s / tot
        self.acc.reset()
        self._updates()
        r = self.acc.result()
        return r.loss, r.prec[1], r.prec[5]

    def wall_us(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / self.batches

    def capture(self):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._updates()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._updates()
        self.graph.replay()          # first replay uploads the graph
        torch.cuda.synchronize()

    def device_us(self):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self.graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / self.batches


def parse_shape(s):
    r, c = s.lower().split('x')
    return int(r), int(c)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1000x10,1000x100,1024x1000')
    ap.add_argument('--batches', type=int, default=1000)
    ap.add_argument('--graph-batches', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sets', type=int, default=4)
    ap.add_argument('--trace', choices=('fused', 'oracle', 'legacy'))
    ap.add_argument('--shape', default='1000x10')
    ap.add_argument('--dtype', choices=tuple(DTYPES), default='bf16')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a GPU")
    require_lib()

    if args.trace:
        rows, classes = parse_shape(args.shape)
        sets = make_sets(rows, classes, DTYPES[args.dtype], args.sets)
        loop = Loop(args.trace, sets, args.batches)
        vals = loop.run()
        torch.cuda.synchronize()
        print(json.dumps({'bench': 'metrics-trace', 'variant': args.trace,
                          'shape': [rows, classes], 'dtype': args.dtype,
                          'batches': args.batches,
                          'loss_p1_p5': [round(v, 4) for v in vals]}))
        return

    out = {'bench': 'metrics', 'batches': args.batches,
           'graph_batches': args.graph_batches, 'rounds': args.rounds,
           'sets': args.sets, 'device': torch.cuda.get_device_name(0),
           'results': []}
    for shape in args.shapes.split(','):
        rows, classes = parse_shape(shape)
        for dname, dtype in DTYPES.items():
            sets = make_sets(rows, classes, dtype, args.sets)
            loops = {v: Loop(v, sets, args.batches)
                     for v in ('fused', 'oracle', 'legacy')}
            vals = {}
            for v, lp in loops.items():
                warm = Loop(v, sets, args.warmup)
                vals[v] = warm.run()
            graphs = {v: Loop(v, sets, args.graph_batches)
                      for v in loops if v != 'legacy'}
            for g in graphs.values():
                g.capture()
            wall = {v: [] for v in loops}
            dev = {v: [] for v in graphs}
            for _ in range(args.rounds):
                for v, lp in loops.items():
                    wall[v].append(round(lp.wall_us(), 2))
                    if v in dev:
                        dev[v].append(round(graphs[v].device_us(), 3))
            row = {'shape': [rows, classes], 'dtype': dname}
            for v in loops:
                row[v] = {'wall_us': wall[v],
                          'wall_us_median': float(np.median(wall[v])),
                          'loss_p1_p5': [round(x, 4) for x in vals[v]]}
                if v in dev:
                    row[v]['device_us'] = dev[v]
                    row[v]['device_us_median'] = float(np.median(dev[v]))
            out['results'].append(row)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
