#!/usr/bin/env python
"""Time of the gather-mode PS fan-in: the arrival chain against the fused
rank-ordered kernel.

  python tools/fanin_bench.py [--n 11200000] [--sets 3] [--steps 200]
                              [--warmup 6] [--rounds 5] [--eager]

For W in {2, 7} workers and the payload codecs raw bf16, q8 and topk16, on
`n` gradient elements (default 11.2 M, ResNet-18's flat gradient):

  chain : what `--fan-in arrival` launches per bucket, from the unchanged
          kernels: zero_ of the f32 accumulator, W accumulate-decodes
          (ps_acc / ps_unpack_q8 / ps_unpack_topk), ps_fused_sgd with a bf16
          wire;
  fused : one ps_fanin_sgd (`--fan-in fused`), same sources, same update.

HIP events around one replay of a graph of `steps` back-to-back repetitions
(mean per repetition, kernel boundaries included), `rounds` alternating
rounds of every variant, median reported. Repetitions rotate over `sets`
independent buffer sets so the working set of even the smallest row (W = 2,
topk16: ~14.4 B/element per set) does not fit the 256 MiB Infinity Cache at
the default sizes; --sets 1 gives the cache-resident figure instead.

Bytes per gradient element, from the kernels' access patterns:
  chain : 4 (zero) + W * (payload + 8) + 22 (g, w, m in; w, m, bf16 wire out)
  fused : W * payload + 8 (w, m in) + 8 (w, m out) + 2 (wire)
Prints one JSON line: per row both times, GB/s of each variant against its
own byte count, the measured ratio chain/fused and the byte-model ratio.
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

from ps_pytorch_amd.ops import functional as F, require_lib  # noqa: E402
from quant_bench import Chain  # noqa: E402

WORKERS = (2, 7)
TOPK_K = 16
LR, MU = 1e-3, 0.9


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=11_200_000)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--eager', action='store_true',
                    help='launch from Python instead of replaying a graph')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("fanin_bench needs a GPU")
    require_lib()
    n = args.n
    if n % 4:
        raise SystemExit("--n must be a multiple of 4")
    wmax = max(WORKERS)
    q8_tot = F.q8_layout(n)[1]
    tk_tot = F.topk_layout(n, TOPK_K)[1]
    g = torch.Generator(device='cuda').manual_seed(1)
    sets = []
    for _ in range(args.sets):
        s = {'w': torch.randn(n, device='cuda', generator=g),
             'm': torch.zeros(n, device='cuda'),
             'wire': torch.zeros(n, dtype=torch.bfloat16, device='cuda'),
             'acc': torch.zeros(n, device='cuda'),
             'bf16': [], 'q8': [], 'topk16': []}
        res = torch.zeros(n, device='cuda')
        for _ in range(wmax):
            x = torch.randn(n, device='cuda', generator=g) * 0.01
            s['bf16'].append(x.to(torch.bfloat16))
            p = torch.zeros(q8_tot, dtype=torch.uint8, device='cuda')
            F.pack_q8(p, x)
            s['q8'].append(p)
            p = torch.zeros(tk_tot, dtype=torch.uint8, device='cuda')
            F.pack_topk_ef(p, x, res.zero_(), TOPK_K)
            s['topk16'].append(p)
        sets.append(s)

    def chain_call(s, codec, W):
        def run():
            acc = s['acc']
            acc.zero_()
            for src in s[codec][:W]:
                if codec == 'q8':
                    F.unpack_q8(acc, src, accumulate=True)
                elif codec == 'topk16':
                    F.unpack_topk(acc, src, TOPK_K, accumulate=True)
                else:
                    F.acc_into(acc, src)
            F.fused_sgd_step(s['w'], acc, s['m'], LR, MU, 0.0, 1.0 / W,
                             False, s['wire'])
        return run

    def fused_call(s, codec, W):
        name, k = (('topk', TOPK_K) if codec == 'topk16' else
                   ('raw', None) if codec == 'bf16' else ('q8', None))

        def run():
            F.fanin_sgd(s['w'], s['m'], s[codec][:W], name, k, LR, MU, 0.0,
                        1.0 / W, False, s['wire'])
        return run

    payload = {'bf16': 2 * n, 'q8': q8_tot, 'topk16': tk_tot}
    variants = {}   # name -> (calls, bytes per repetition)
    for W in WORKERS:
        for codec in ('bf16', 'q8', 'topk16'):
            row = f'{codec}_w{W}'
            variants[f'chain_{row}'] = (
                [chain_call(s, codec, W) for s in sets],
                4 * n + W * (payload[codec] + 8 * n) + 22 * n)
            variants[f'fused_{row}'] = (
                [fused_call(s, codec, W) for s in sets],
                W * payload[codec] + 18 * n)

    chains = {k: Chain(calls, args.steps, args.warmup, args.eager)
              for k, (calls, _) in variants.items()}
    us = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, chain in chains.items():
            us[k].append(round(chain.time_us(), 3))
    out = {'bench': 'fanin', 'n': n, 'sets': args.sets, 'steps': args.steps,
           'rounds': args.rounds, 'launch': 'eager' if args.eager else 'graph',
           'device': torch.cuda.get_device_name(0), 'rows': {}}
    for W in WORKERS:
        for codec in ('bf16', 'q8', 'topk16'):
            row = f'{codec}_w{W}'
            rec = {}
            for v in ('chain', 'fused'):
                key = f'{v}_{row}'
                med = float(np.median(us[key]))
                nbytes = variants[key][1]
                rec[v] = {'us': us[key], 'us_median': med, 'bytes': nbytes,
                          'bytes_per_elem': round(nbytes / n, 3),
                          'gbps': round(nbytes / med / 1e3, 1)}
            rec['ratio_chain_over_fused'] = round(
                rec['chain']['us_median'] / rec['fused']['us_median'], 3)
            rec['byte_model_ratio'] = round(
                rec['chain']['bytes'] / rec['fused']['bytes'], 3)
            out['rows'][row] = rec
    print(json.dumps(out))


if __name__ == '__main__':
    main()
