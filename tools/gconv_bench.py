#!/usr/bin/env python
"""Per-shape time of the grouped 3x3 convolutions of ResNeXt29_32x4d at the
bench batch size: the in-tree kernels (ops/kernels/conv_group.hip, or
ops/kernels/conv_group_f32.hip with --dtype fp32) against PS_GCONV=0, i.e.
torch/MIOpen, which is what PsConv2d(groups=G) ran on before the kernels
existed.

  python tools/gconv_bench.py [--batch 1024] [--iters 200] [--warmup 5]
                              [--rounds 5] [--dtype {bf16,fp32}]
                              [--net {resnext29,resnext50}]

The model has nine grouped convolutions in five distinct shapes (the three
blocks of a stage share one shape except the strided first block of stages
2 and 3). Per shape and setting: HIP events around `iters` back-to-back
eager calls on one stream, after `warmup` calls of the same shape; `rounds`
rounds alternating the two settings, median reported. "fwd" is the forward
alone, "bwd" the backward alone (dgrad + wgrad of one retained forward,
`iters` times in one window). FLOPs are the useful ones, 2 * M * C * Cg * 9
per pass. Outputs of the two settings are compared on the same inputs
before timing (max error over the reference's max). Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ps_pytorch_amd.ops import conv as ps_conv  # noqa: E402
from ps_pytorch_amd.ops import require_lib  # noqa: E402

# (C, H = W, stride) of the grouped convs; cardinality 32, 3x3, pad 1
SHAPES = [(128, 32, 1), (256, 32, 2), (256, 16, 1), (512, 16, 2), (512, 8, 1)]
# resnext50_32x4d on 32x32 inputs adds a fourth stage
SHAPES50 = SHAPES + [(1024, 8, 2), (1024, 4, 1)]
G = 32


def _events(fn, iters):
    beg, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e3 / iters


def _time(conv, x, dy, hand, iters, warmup):
    """(fwd us, bwd us) of one setting. The backward window replays the
    backward of ONE forward (retain_graph, gradients returned rather than
    accumulated), so it holds the backward kernels alone."""
    ps_conv._GCONV = hand
    out = conv(x)
    bwd_fn = lambda: torch.autograd.grad(out, (x, conv.weight), dy,
                                         retain_graph=True)
    for _ in range(warmup):
        conv(x)
        bwd_fn()
    with torch.no_grad():
        fwd = _events(lambda: conv(x), iters)
    return fwd, _events(bwd_fn, iters)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtype', choices=('bf16', 'fp32'), default='bf16')
    ap.add_argument('--net', choices=('resnext29', 'resnext50'),
                    default='resnext29')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gconv_bench needs a GPU")
    require_lib()
    cl = torch.channels_last
    bf = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
    rows = []
    for C, H, stride in (SHAPES if args.net == 'resnext29' else SHAPES50):
        torch.manual_seed(C + H)
        conv = ps_conv.PsConv2d(C, C, 3, stride=stride, padding=1, groups=G,
                                bias=False).to('cuda', bf)
        x = torch.randn(args.batch, C, H, H, device='cuda', dtype=bf) \
            .contiguous(memory_format=cl).requires_grad_(True)
        P = (H + 2 - 3) // stride + 1
        dy = torch.randn(args.batch, C, P, P, device='cuda', dtype=bf) \
            .contiguous(memory_format=cl)
        res = {}
        for hand in (True, False):
            ps_conv._GCONV = hand
            x.grad = conv.weight.grad = None
            out = conv(x)
            out.backward(dy)
            res[hand] = [t.detach().float() for t in
                         (out, x.grad, conv.weight.grad)]
        err = [float((a - b).abs().max() / b.abs().max())
               for a, b in zip(res[True], res[False])]
        us = {True: [], False: []}
        for _ in range(args.rounds):
            for hand in (True, False):
                us[hand].append(_time(conv, x, dy, hand, args.iters,
                                      args.warmup))
        med = {h: np.median(np.array(v), axis=0) for h, v in us.items()}
        flop = 2.0 * args.batch * P * P * C * (C // G) * 9
        rows.append({
            'shape': [args.batch, C, H, H], 'groups': G, 'stride': stride,
            'hand_fwd_us': round(float(med[True][0]), 1),
            'torch_fwd_us': round(float(med[False][0]), 1),
            'hand_bwd_us': round(float(med[True][1]), 1),
            'torch_bwd_us': round(float(med[False][1]), 1),
            'fwd_speedup': round(float(med[False][0] / med[True][0]), 3),
            'bwd_speedup': round(float(med[False][1] / med[True][1]), 3),
            'hand_fwd_tflops': round(flop / med[True][0] / 1e6, 2),
            'hand_bwd_tflops': round(2 * flop / med[True][1] / 1e6, 2),
            'max_err_vs_torch': [round(e, 5) for e in err]})
    ps_conv._GCONV = True
    extra = {} if args.dtype == 'bf16' else {'dtype': args.dtype}
    if args.net != 'resnext29':
        extra['net'] = args.net
    print(json.dumps({'bench': 'gconv', **extra, 'batch': args.batch,
                      'iters': args.iters, 'rounds': args.rounds,
                      'device': torch.cuda.get_device_name(0), 'rows': rows}))


if __name__ == '__main__':
    main()
