#!/usr/bin/env python
"""Per-shape time of the 13 depthwise 3x3 convolutions of MobileNet: the
in-tree kernels (ops/kernels/conv_dw.hip) against PS_DWCONV=0, i.e.
torch/MIOpen, which is what a depthwise PsConv2d ran on before the kernels
existed.

  python tools/dwconv_bench.py [--layout cifar|imagenet] [--batch N]
                               [--dtype bf16|fp32] [--iters 100]
                               [--warmup 5] [--rounds 5]

The batch defaults to 1024 (cifar) or 256 (imagenet). Shapes that repeat in
the model are timed once and carry their count. Per shape and setting: HIP
events around `iters` back-to-back eager calls on one stream, after `warmup`
calls of the same shape; `rounds` rounds alternating the two settings,
median reported, and the spread of the torch setting (max - min over its
median) as the run-to-run noise. "fwd" is the forward alone, "fb" forward +
backward (dgrad + wgrad). The memory floor of a pass is one read and one
write of the activation (fwd: x + out; fb: x + out, then dout + dx and
x + dout again for wgrad) at 5 TB/s, the streaming rate of
profiles/r06_error_feedback.md. Outputs of the two settings are compared on
the same inputs before timing. Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ps_pytorch_amd.models.mobilenet import BLOCKS  # noqa: E402
from ps_pytorch_amd.ops import conv as ps_conv  # noqa: E402
from ps_pytorch_amd.ops import require_lib  # noqa: E402

STREAM_BPS = 5e12


def shapes(layout: str):
    """[(C, H = W, stride, count)] of the depthwise convs, in model order."""
    h, c, out = (112 if layout == 'imagenet' else 32), 32, []
    for width, stride in BLOCKS:
        if out and out[-1][:3] == (c, h, stride):
            out[-1] = (c, h, stride, out[-1][3] + 1)
        else:
            out.append((c, h, stride, 1))
        h, c = (h - 1) // stride + 1, width
    return out


def _events(fn, iters):
    beg, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e3 / iters


def _time(conv, x, dy, hand, iters, warmup):
    """(fwd us, fwd+bwd us) of one setting."""
    ps_conv._DWCONV = hand

    def fb():
        torch.autograd.grad(conv(x), (x, conv.weight), dy)

    for _ in range(warmup):
        fb()
    with torch.no_grad():
        fwd = _events(lambda: conv(x), iters)
    return fwd, _events(fb, iters)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--layout', choices=('cifar', 'imagenet'), default='cifar')
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--dtype', choices=('bf16', 'fp32'), default='bf16')
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_bench needs a GPU")
    require_lib()
    batch = args.batch or (256 if args.layout == 'imagenet' else 1024)
    dt = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
    cl = torch.channels_last
    rows = []
    for C, H, stride, count in shapes(args.layout):
        torch.manual_seed(C + H)
        conv = ps_conv.PsConv2d(C, C, 3, stride=stride, padding=1, groups=C,
                                bias=False).to('cuda', dt)
        x = torch.randn(batch, C, H, H, device='cuda', dtype=dt) \
            .contiguous(memory_format=cl).requires_grad_(True)
        P = (H - 1) // stride + 1
        dy = torch.randn(batch, C, P, P, device='cuda', dtype=dt) \
            .contiguous(memory_format=cl)
        res = {}
        for hand in (True, False):
            ps_conv._DWCONV = hand
            out = conv(x)
            gx, gw = torch.autograd.grad(out, (x, conv.weight), dy)
            res[hand] = [t.detach().float() for t in (out, gx, gw)]
        err = [float((a - b).abs().max() / b.abs().max())
               for a, b in zip(res[True], res[False])]
        del res
        us = {True: [], False: []}
        for _ in range(args.rounds):
            for hand in (True, False):
                us[hand].append(_time(conv, x, dy, hand, args.iters,
                                      args.warmup))
        arr = {h: np.array(v) for h, v in us.items()}
        med = {h: np.median(a, axis=0) for h, a in arr.items()}
        spread = (arr[False].max(0) - arr[False].min(0)) / med[False]
        nx, ny = x.numel() * x.element_size(), dy.numel() * dy.element_size()
        floor_fwd = (nx + ny) / STREAM_BPS * 1e6
        floor_fb = 3 * (nx + ny) / STREAM_BPS * 1e6
        rows.append({
            'shape': [batch, C, H, H], 'stride': stride, 'count': count,
            'hand_fwd_us': round(float(med[True][0]), 1),
            'torch_fwd_us': round(float(med[False][0]), 1),
            'hand_fb_us': round(float(med[True][1]), 1),
            'torch_fb_us': round(float(med[False][1]), 1),
            'fwd_speedup': round(float(med[False][0] / med[True][0]), 3),
            'fb_speedup': round(float(med[False][1] / med[True][1]), 3),
            'fwd_floor_frac': round(floor_fwd / float(med[True][0]), 3),
            'fb_floor_frac': round(floor_fb / float(med[True][1]), 3),
            'torch_spread': [round(float(s), 3) for s in spread],
            'max_err_vs_torch': [round(e, 5) for e in err]})
    ps_conv._DWCONV = True
    print(json.dumps({'bench': 'dwconv', 'layout': args.layout,
                      'dtype': args.dtype, 'batch': batch,
                      'iters': args.iters, 'rounds': args.rounds,
                      'device': torch.cuda.get_device_name(0), 'rows': rows}))


if __name__ == '__main__':
    main()
