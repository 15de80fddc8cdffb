#!/usr/bin/env python
"""Time of the gradient wire codecs: the packs with and without error
feedback, the block top-k codec, and the PS-side decodes.

  python tools/quant_bench.py [--n 11200000] [--sets 4] [--steps 2000]
                              [--warmup 20] [--rounds 5] [--eager]
                              [--baseline-lib other/libps_hip.so]

Times pack_q8 against pack_q8_ef (f32 and bf16 sources) and pack_wire
f32->bf16 against pack_wire_ef on `n` elements (default 11.2 M, ResNet-18's
flat gradient), and next to them the block top-k codec: pack_topk_ef (f32
and bf16 sources) for every K, its worst case (`_ties`: all-equal blocks,
on which the threshold search cannot stop early), and the accumulating
decodes unpack_topk and
unpack_q8 the PS runs per arrival. HIP events around one replay of a graph
of `steps` back-to-back launches (mean per launch, kernel boundaries
included), `rounds` alternating rounds of every variant, median reported.
GB/s counts the bytes each kernel actually moves: source read, payload
write, for the EF kernels one f32 residual read and one write per element,
and for the decodes the payload read plus one f32 accumulator read and
write. Launches rotate over `sets` independent buffer sets (the EF packs
carry their residual from launch to launch, as training does) so that with
the default 4 the working set (~1.1 GB) does not fit the 256 MiB Infinity
Cache; --sets 1 gives the cache-resident figure instead.

--baseline-lib names another build of the kernel library (the parent
commit's, say); its plain packs are timed in the same rounds on the same
buffers, and the ratio to this build's is reported. Prints one JSON line;
`wire_bytes_per_elem` is the payload size of each codec per gradient
element, and `time_ratio` holds every top-k row against its q8 counterpart
(pack_q8_ef of the same source, unpack_q8) from the same run.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ps_pytorch_amd.ops import (current_stream_ptr, dtype_tag,  # noqa: E402
                                functional as F, require_lib)


class Chain:
    """`steps` back-to-back launches cycling through `calls`, captured once
    into a HIP graph: these kernels take ~10 us, about what one launch
    through Python costs the host, so an eager loop would time the host."""

    def __init__(self, calls, steps: int, warmup: int, eager: bool):
        self.calls, self.steps, self.graph = calls, steps, None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for i in range(warmup):
                calls[i % len(calls)]()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if not eager:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._run()
            self.graph.replay()          # first replay uploads the graph
            torch.cuda.synchronize()

    def _run(self) -> None:
        for i in range(self.steps):
            self.calls[i % len(self.calls)]()

    def time_us(self) -> float:
        """Device us per launch over one pass of the chain."""
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        if self.graph is not None:
            self.graph.replay()
        else:
            self._run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / self.steps


def load_baseline(path: str) -> ctypes.CDLL:
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.ps_pack_q8.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
    lib.ps_pack_bf16.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_long, ctypes.c_void_p]
    return lib


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=11_200_000)
    ap.add_argument('--sets', type=int, default=4)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--eager', action='store_true',
                    help='launch from Python instead of replaying a graph')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("quant_bench needs a GPU")
    require_lib()
    base = load_baseline(args.baseline_lib) if args.baseline_lib else None
    n = args.n
    qb, tot = F.q8_layout(n)
    nblk = (tot - qb) // 4
    g = torch.Generator(device='cuda').manual_seed(1)
    sets = []
    for _ in range(args.sets):
        x = torch.randn(n, device='cuda', generator=g) * 0.01
        sets.append({
            'f32': x, 'bf16': x.to(torch.bfloat16),
            'res': torch.randn(n, device='cuda', generator=g) * 1e-4,
            'payload': torch.zeros(tot, dtype=torch.uint8, device='cuda'),
            'wire': torch.zeros(n, dtype=torch.bfloat16, device='cuda'),
            'acc': torch.zeros(n, device='cuda'),
            'zero': torch.zeros(n, device='cuda'),
            'zero_res': torch.zeros(n, device='cuda'),
            # sliced per K; any bytes decode (u8 index, bf16 value)
            'tk_payload': torch.zeros(F.topk_layout(n, max(F.TOPK_KS))[1],
                                      dtype=torch.uint8, device='cuda')})

    q8_bytes = n + 4 * nblk
    variants = {}   # name -> (calls, bytes moved per launch)
    for src, sz in (('f32', 4), ('bf16', 2)):
        variants[f'pack_q8_{src}'] = (
            [lambda s=s, k=src: F.pack_q8(s['payload'], s[k]) for s in sets],
            sz * n + q8_bytes)
        variants[f'pack_q8_ef_{src}'] = (
            [lambda s=s, k=src: F.pack_q8_ef(s['payload'], s[k], s['res'])
             for s in sets], sz * n + q8_bytes + 8 * n)
        if base is not None:
            variants[f'baseline_pack_q8_{src}'] = (
                [lambda s=s, k=src: base.ps_pack_q8(
                    s['payload'].data_ptr(), s[k].data_ptr(), n,
                    dtype_tag(s[k].dtype), current_stream_ptr())
                 for s in sets], sz * n + q8_bytes)
        for k in F.TOPK_KS:
            tk = F.topk_layout(n, k)[1]
            variants[f'pack_topk_ef_{src}_k{k}'] = (
                [lambda s=s, key=src, k=k, tk=tk: F.pack_topk_ef(
                    s['tk_payload'][:tk], s[key], s['res'], k)
                 for s in sets], sz * n + tk + 8 * n)
    # the threshold search stops early on distinct magnitudes; all-equal
    # blocks (here: zeros, which stay zeros) take every round — the worst case
    tk = F.topk_layout(n, 16)[1]
    variants['pack_topk_ef_f32_k16_ties'] = (
        [lambda s=s, tk=tk: F.pack_topk_ef(s['tk_payload'][:tk], s['zero'],
                                           s['zero_res'], 16)
         for s in sets], 4 * n + tk + 8 * n)
    # the PS-side decodes, accumulating as the drain does
    variants['unpack_q8'] = (
        [lambda s=s: F.unpack_q8(s['acc'], s['payload'], accumulate=True)
         for s in sets], q8_bytes + 8 * n)
    for k in F.TOPK_KS:
        tk = F.topk_layout(n, k)[1]
        variants[f'unpack_topk_k{k}'] = (
            [lambda s=s, k=k, tk=tk: F.unpack_topk(
                s['acc'], s['tk_payload'][:tk], k, accumulate=True)
             for s in sets], tk + 8 * n)
    variants['pack_wire_bf16'] = (
        [lambda s=s: F.pack_wire(s['wire'], s['f32']) for s in sets], 6 * n)
    variants['pack_wire_ef_bf16'] = (
        [lambda s=s: F.pack_wire_ef(s['wire'], s['f32'], s['res'])
         for s in sets], 14 * n)
    if base is not None:
        variants['baseline_pack_wire_bf16'] = (
            [lambda s=s: base.ps_pack_bf16(
                s['wire'].data_ptr(), s['f32'].data_ptr(), n,
                current_stream_ptr()) for s in sets], 6 * n)

    chains = {k: Chain(calls, args.steps, args.warmup, args.eager)
              for k, (calls, _) in variants.items()}
    us = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, chain in chains.items():
            us[k].append(round(chain.time_us(), 3))
    out = {'bench': 'quant', 'n': n, 'sets': args.sets, 'steps': args.steps,
           'rounds': args.rounds, 'launch': 'eager' if args.eager else 'graph',
           'device': torch.cuda.get_device_name(0)}
    for k, (_, nbytes) in variants.items():
        med = float(np.median(us[k]))
        out[k] = {'us': us[k], 'us_median': med, 'bytes': nbytes,
                  'gbps': round(nbytes / med / 1e3, 1)}
    ratios = {}
    for plain, ef in (('pack_q8_f32', 'pack_q8_ef_f32'),
                      ('pack_q8_bf16', 'pack_q8_ef_bf16'),
                      ('pack_wire_bf16', 'pack_wire_ef_bf16')):
        ratios[f'{ef}/{plain}'] = round(
            out[ef]['us_median'] / out[plain]['us_median'], 3)
        if base is not None:
            ratios[f'{plain}/baseline'] = round(
                out[plain]['us_median']
                / out[f'baseline_{plain}']['us_median'], 3)
    for k in F.TOPK_KS:
        for src in ('f32', 'bf16'):
            ratios[f'pack_topk_ef_{src}_k{k}/pack_q8_ef_{src}'] = round(
                out[f'pack_topk_ef_{src}_k{k}']['us_median']
                / out[f'pack_q8_ef_{src}']['us_median'], 3)
        ratios[f'unpack_topk_k{k}/unpack_q8'] = round(
            out[f'unpack_topk_k{k}']['us_median']
            / out['unpack_q8']['us_median'], 3)
    out['time_ratio'] = ratios
    wire = {'f32': 4.0, 'bf16': 2.0, 'q8': round(q8_bytes / n, 4)}
    for k in F.TOPK_KS:
        wire[f'topk_k{k}'] = round(F.topk_layout(n, k)[1] / n, 4)
    out['wire_bytes_per_elem'] = wire
    print(json.dumps(out))


if __name__ == '__main__':
    main()
