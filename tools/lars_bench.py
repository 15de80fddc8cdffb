#!/usr/bin/env python
"""Time of one PS-side optimizer step on the ResNet-18/CIFAR flat layout:
FlatLARS (three launches: per-chunk f64 norms, per-tensor fold, update)
against FlatSGD (one launch), for f32 and bf16 gradients, both with the bf16
wire re-pack.

  python tools/lars_bench.py [--network ResNet18] [--sets 3] [--steps 200]
                             [--warmup 6] [--rounds 5] [--eager]

HIP events around one replay of a graph of `steps` back-to-back steps on one
stream (mean per step, kernel boundaries included), `rounds` alternating
rounds of every variant, median reported. Steps rotate over `sets`
independent buffer sets so the working set (~18 B/element per set and more)
does not fit the 256 MiB Infinity Cache; --sets 1 gives the cache-resident
figure instead. The LARS step counter advances on the device every step; the
schedule is constant so every step does the same work.

Bytes per element, from the kernels' access patterns (G = 4 or 2, the
gradient's width):
  sgd  : G + 8 (w, m in) + 8 (w, m out) + 2 (wire)
  lars : sgd + 4 + G (the norm pass reads w and g once more)
Prints one JSON line: per gradient dtype both times, GB/s of each against
its own byte count, and what LARS costs over SGD in us and as a ratio.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ps_pytorch_amd.models import build_model  # noqa: E402
from ps_pytorch_amd.ops import require_lib  # noqa: E402
from ps_pytorch_amd.optim import FlatLARS, FlatSGD, LRSchedule  # noqa: E402
from ps_pytorch_amd.parallel.flat import FlatSpace  # noqa: E402
from quant_bench import Chain  # noqa: E402

LR, MU, WD = 0.1, 0.9, 5e-4


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--network', default='ResNet18')
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--eager', action='store_true',
                    help='launch from Python instead of replaying a graph')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lars_bench needs a GPU")
    require_lib()
    # the layout only: the model itself stays on the host
    fs = FlatSpace(build_model(args.network, num_classes=10, in_channels=3))
    segs, n = fs.segments(), fs.padded
    gen = torch.Generator(device='cuda').manual_seed(1)
    variants = {}   # name -> (calls, bytes per step)
    for gname, gdt, gw in (('f32', torch.float32, 4),
                           ('bf16', torch.bfloat16, 2)):
        sgd_calls, lars_calls = [], []
        for _ in range(args.sets):
            g = (torch.randn(n, device='cuda', generator=gen) * 0.01).to(gdt)
            wire = torch.zeros(n, dtype=torch.bfloat16, device='cuda')
            sgd = FlatSGD(torch.randn(n, device='cuda', generator=gen),
                          lr=LR, momentum=MU, weight_decay=WD)
            lars = FlatLARS(torch.randn(n, device='cuda', generator=gen),
                            segs, LRSchedule(LR, 'constant', total_steps=1),
                            momentum=MU, weight_decay=WD)
            sgd_calls.append(lambda o=sgd, g=g, w=wire: o.step(
                g, grad_scale=0.5, wire_out=w))
            lars_calls.append(lambda o=lars, g=g, w=wire: o.step(
                g, grad_scale=0.5, wire_out=w))
        variants[f'sgd_{gname}'] = (sgd_calls, (gw + 18) * n)
        variants[f'lars_{gname}'] = (lars_calls, (2 * gw + 22) * n)

    chains = {k: Chain(calls, args.steps, args.warmup, args.eager)
              for k, (calls, _) in variants.items()}
    us = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, chain in chains.items():
            us[k].append(round(chain.time_us(), 3))
    out = {'bench': 'lars', 'network': args.network, 'n': n,
           'tensors': len(segs), 'sets': args.sets, 'steps': args.steps,
           'rounds': args.rounds,
           'launch': 'eager' if args.eager else 'graph',
           'device': torch.cuda.get_device_name(0), 'rows': {}}
    for gname in ('f32', 'bf16'):
        rec = {}
        for v in ('sgd', 'lars'):
            key = f'{v}_{gname}'
            med = float(np.median(us[key]))
            nbytes = variants[key][1]
            rec[v] = {'us': us[key], 'us_median': med, 'bytes': nbytes,
                      'bytes_per_elem': round(nbytes / n, 3),
                      'gbps': round(nbytes / med / 1e3, 1)}
        rec['lars_minus_sgd_us'] = round(
            rec['lars']['us_median'] - rec['sgd']['us_median'], 3)
        rec['ratio_lars_over_sgd'] = round(
            rec['lars']['us_median'] / rec['sgd']['us_median'], 3)
        rec['byte_model_ratio'] = round(
            rec['lars']['bytes'] / rec['sgd']['bytes'], 3)
        out['rows'][gname] = rec
    print(json.dumps(out))


if __name__ == '__main__':
    main()
