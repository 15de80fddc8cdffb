#!/usr/bin/env python
"""Time of one fused GroupNorm(+residual)+ReLU layer (G = 32) on the GN
ResNet-18 / ResNet-50 layer shapes, forward alone and forward + backward, in
bf16 and f32:

  gn    : PsGroupNorm2d (ops/kernels/groupnorm.hip; the plan column says
          which form ran: slab channels forward/backward, 0 = streamed)
  torch : F.group_norm + add + relu on the same channels-last tensors, the
          path a user has without the kernels
  bn    : PsBatchNorm2d (ps_bn_fwd / ps_bn_bwd) on the same shapes, the
          in-tree yardstick for bytes moved

  python tools/gn_bench.py [--res cifar imagenet] [--dtypes bf16 f32]
                           [--steps 20] [--warmup 3] [--rounds 3] [--sets 2]
                           [--md FILE] [--torch-graph]

HIP events around one replay of a graph of `steps` back-to-back layer calls
on one stream (mean per call, kernel boundaries included; the torch variant
is launched eagerly between the same events unless --torch-graph); `rounds`
alternating rounds of every variant, median reported. Calls rotate over
`sets` independent tensor sets. Bytes per element moved by the GN kernels,
from their access patterns (E = element width; mask 1/8 B):
  forward  resident x + res + y = 3E + 1/8        streamed + E (x twice)
  backward resident x + dy + dx + dres = 4E + 1/8 streamed + 2E
Prints one JSON line per (shape, dtype); --md also writes a table.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ps_pytorch_amd.ops import require_lib  # noqa: E402
from ps_pytorch_amd.ops.modules import (  # noqa: E402
    PsBatchNorm2d, PsGroupNorm2d, _gn_plan)
from quant_bench import Chain  # noqa: E402

G = 32
# (N, H = W, C): the distinct norm-layer shapes of ResNet-18 and ResNet-50
SHAPES = {
    'cifar': [(256, 32, 64), (256, 16, 128), (256, 8, 256), (256, 4, 512),
              (256, 32, 256), (256, 16, 512), (256, 8, 1024), (256, 4, 2048)],
    'imagenet': [(32, 112, 64), (32, 56, 64), (32, 56, 256), (32, 28, 128),
                 (32, 28, 512), (32, 14, 256), (32, 14, 1024), (32, 7, 512),
                 (32, 7, 2048)],
}
DTYPES = {'bf16': torch.bfloat16, 'f32': torch.float32}


class _TorchGN(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(C))
        self.bias = torch.nn.Parameter(torch.zeros(C))

    def forward(self, x, residual=None):
        return F.relu(F.group_norm(x, G, self.weight, self.bias, 1e-5)
                      + residual)


def _calls(make, N, H, C, dtype, sets, backward):
    calls = []
    for _ in range(sets):
        m = make().to('cuda', dtype).train()
        x, r, dy = (torch.randn(N, C, H, H, device='cuda').to(dtype).contiguous(
            memory_format=torch.channels_last) for _ in range(3))
        if backward:
            x.requires_grad_(True)
            r.requires_grad_(True)
            ins = [x, r, m.weight, m.bias]
            calls.append(lambda m=m, x=x, r=r, dy=dy, ins=ins:
                         torch.autograd.grad(m(x, residual=r), ins, dy))
        else:
            def fwd(m=m, x=x, r=r):
                with torch.no_grad():
                    m(x, residual=r)
            calls.append(fwd)
    return calls


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', nargs='+', default=['cifar', 'imagenet'])
    ap.add_argument('--dtypes', nargs='+', default=['bf16', 'f32'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--sets', type=int, default=2)
    ap.add_argument('--md', default=None)
    ap.add_argument('--torch-graph', action='store_true',
                    help='capture the torch variant into a graph as well')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gn_bench needs a GPU")
    require_lib()
    makers = {'gn': lambda C: PsGroupNorm2d(G, C, relu=True),
              'torch': lambda C: _TorchGN(C),
              'bn': lambda C: PsBatchNorm2d(C, relu=True)}
    rows = []
    for res in args.res:
        for N, H, C in SHAPES[res]:
            for dname in args.dtypes:
                dtype = DTYPES[dname]
                elt = 2 if dname == 'bf16' else 4
                plan = [_gn_plan(H * H, C, C // G, elt, t) for t in (1, 2)]
                chains = {}
                for v, mk in makers.items():
                    for bwd in (False, True):
                        calls = _calls(lambda: mk(C), N, H, C, dtype,
                                       args.sets, bwd)
                        # torch's ops are launched eagerly unless asked:
                        # what they record into a graph is not ours to vouch
                        # for; their times then include launch gaps
                        eager = v == 'torch' and not args.torch_graph
                        chains[(v, bwd)] = Chain(calls, args.steps,
                                                 args.warmup, eager)
                us = {k: [] for k in chains}
                for _ in range(args.rounds):
                    for k, ch in chains.items():
                        us[k].append(ch.time_us())
                med = {k: float(np.median(v)) for k, v in us.items()}
                n = N * H * H * C
                fb = (3 * elt + 0.125 + (0 if plan[0] else elt)) * n
                bb = (4 * elt + 0.125 + (0 if plan[1] else 2 * elt)) * n
                row = {'bench': 'gn', 'res': res, 'N': N, 'HW': H * H, 'C': C,
                       'dtype': dname, 'plan_fwd': plan[0], 'plan_bwd': plan[1]}
                for v in makers:
                    row[f'{v}_fwd_us'] = round(med[(v, False)], 2)
                    row[f'{v}_fwdbwd_us'] = round(med[(v, True)], 2)
                row['gn_fwd_gbps'] = round(fb / med[('gn', False)] / 1e3, 1)
                row['gn_fwdbwd_gbps'] = round(
                    (fb + 0.125 * n + bb) / med[('gn', True)] / 1e3, 1)
                row['torch_over_gn_fwd'] = round(
                    med[('torch', False)] / med[('gn', False)], 2)
                row['torch_over_gn_fwdbwd'] = round(
                    med[('torch', True)] / med[('gn', True)], 2)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del chains
                torch.cuda.empty_cache()
    if args.md:
        cols = ['res', 'N', 'HW', 'C', 'dtype', 'plan_fwd', 'plan_bwd',
                'gn_fwd_us', 'torch_fwd_us', 'bn_fwd_us', 'gn_fwdbwd_us',
                'torch_fwdbwd_us', 'bn_fwdbwd_us', 'gn_fwd_gbps',
                'gn_fwdbwd_gbps', 'torch_over_gn_fwd', 'torch_over_gn_fwdbwd']
        with open(args.md, 'w') as f:
            f.write('| ' + ' | '.join(cols) + ' |\n')
            f.write('|' + '---|' * len(cols) + '\n')
            for r in rows:
                f.write('| ' + ' | '.join(str(r[c]) for c in cols) + ' |\n')


if __name__ == '__main__':
    main()
