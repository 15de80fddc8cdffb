#!/usr/bin/env python
"""Per-batch time of the two real-data loader modes on the GPU.

  python tools/loader_bench.py [--batch 1024] [--dtype bf16] [--images 50000]
                               [--steps 200] [--warmup 20] [--rounds 5]

Writes a CIFAR-10-shaped fake dataset (random bytes, standard pickle
batches) to a temporary directory, loads it GPU-resident and times
`next_batch()` of RealResidentLoader(rng='torch') — plus the channels-last
copy NNTrainer.train_step adds to it — against rng='philox', which yields
channels-last batches from one kernel. HIP events around `steps` back-to-back
batches (mean per batch), `rounds` alternating rounds of each mode; the host
clock around the same window (ending in a synchronize) is reported next to
it, since the torch mode also does host work per batch. Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ps_pytorch_amd.data import RealDataset, RealResidentLoader  # noqa: E402


def write_fake_cifar10(root: str, n_train: int) -> None:
    d = os.path.join(root, 'cifar-10-batches-py')
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(1)
    sizes = [len(a) for a in np.array_split(np.arange(n_train), 5)]
    names = [f'data_batch_{i}' for i in range(1, 6)] + ['test_batch']
    for name, n in zip(names, sizes + [16]):
        with open(os.path.join(d, name), 'wb') as f:
            pickle.dump({'data': rng.integers(0, 256, (n, 3072),
                                              dtype=np.uint8),
                         'labels': rng.integers(0, 10, n).tolist()}, f)


def time_mode(loader, steps: int, channels_last_copy: bool):
    """(device ms/batch, host ms/batch) over `steps` back-to-back batches."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        x, _ = loader.next_batch()
        if channels_last_copy:
            x = x.contiguous(memory_format=torch.channels_last)
    e1.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) * 1e3 / steps
    return e0.elapsed_time(e1) / steps, host


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--images', type=int, default=50000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench needs a GPU")
    dtype = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
    dev = torch.device('cuda', 0)
    with tempfile.TemporaryDirectory() as root:
        write_fake_cifar10(root, args.images)
        ds = RealDataset('Cifar10', 'train', root, device=dev, dtype=dtype)
    modes = {
        'torch': (RealResidentLoader(ds, args.batch, seed=1), True),
        'fused': (RealResidentLoader(ds, args.batch, seed=1, rng='philox'),
                  False),
    }
    for loader, cl in modes.values():
        time_mode(loader, args.warmup, cl)
    res = {k: {'device_ms': [], 'host_ms': []} for k in modes}
    for _ in range(args.rounds):
        for k, (loader, cl) in modes.items():
            d, h = time_mode(loader, args.steps, cl)
            res[k]['device_ms'].append(round(d, 4))
            res[k]['host_ms'].append(round(h, 4))
    out = {'bench': 'loader', 'batch': args.batch, 'dtype': args.dtype,
           'images': args.images, 'steps': args.steps, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(0)}
    for k, r in res.items():
        out[k] = dict(r, device_ms_median=float(np.median(r['device_ms'])),
                      host_ms_median=float(np.median(r['host_ms'])))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
