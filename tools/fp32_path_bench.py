"""fp32 compute path bench: hand-written exact-f32 MFMA kernels vs torch.

bench.py measures the bf16 flagship and has no dtype flag; this tool covers
--compute-dtype fp32. Three modes, all HIP-event timed on one GPU:

  e2e     NNTrainer steps with compute_dtype='fp32', graph-captured, with
          warmup; prints img/s. --torch runs the same with the PS_F32
          kill-switch off (conv / linear / pool / CE back on torch).
  shapes  per-shape: the three f32 conv entry points (C API, as in
          tools/conv_microbench.py) against F.conv2d fp32, on that tool's
          shape list.
  curve   same-seed training loss curve on label-correlated synthetic data
          for --dtype bf16|fp32 (and --torch), printed every --every steps.

Run on a GPU box, e.g.
  python tools/fp32_path_bench.py --mode e2e --network ResNet18 --batch-size 256
  python tools/fp32_path_bench.py --mode e2e --network LeNet --dataset MNIST \\
      --batch-size 8192 --torch
  python tools/fp32_path_bench.py --mode shapes --batch 256
  python tools/fp32_path_bench.py --mode curve --dtype fp32 --steps 200
"""
import argparse
import json
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, '.')
from ps_pytorch_amd.ops import require_lib, current_stream_ptr  # noqa: E402
from ps_pytorch_amd.ops import conv as ps_conv  # noqa: E402

_CL = torch.channels_last


def event_time_ms(fn, iters, warmup):
    """Mean ms per call: warmup, then `iters` calls between two HIP events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _trainer(args, dtype):
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network=args.network, dataset=args.dataset,
                    batch_size=args.batch_size, lr=args.lr, momentum=0.9,
                    enable_gpu=True, compute_dtype=dtype, seed=args.seed)
    tr = NNTrainer(cfg, device=torch.device('cuda', 0))
    tr.build_model()
    return tr


def _route(args):
    return 'torch (PS_F32=0)' if args.torch else 'hand kernels'


def mode_e2e(args):
    from ps_pytorch_amd.config import input_shape_of
    tr = _trainer(args, 'fp32')
    assert tr.compute_dtype == torch.float32
    g = torch.Generator().manual_seed(1234)
    bs = args.batch_size
    x = torch.randn(bs, *input_shape_of(args.dataset), generator=g).to('cuda')
    y = torch.randint(0, 10, (bs,), generator=g).to('cuda')
    graphed = (not args.eager) and tr.enable_graph(x, y)
    if graphed:
        def step():
            tr.graph_step(x, y)
    else:
        def step():
            tr._step_body(x.contiguous(memory_format=_CL)
                          if x.dim() == 4 else x, y)
    ms = event_time_ms(step, args.steps, args.warmup)
    loss = float(tr._gloss) if graphed else float('nan')
    print(json.dumps({
        'mode': 'e2e', 'network': args.network, 'dataset': args.dataset,
        'batch_size': bs, 'compute_dtype': 'fp32', 'route': _route(args),
        'graph': bool(graphed), 'warmup': args.warmup, 'steps': args.steps,
        'ms_per_step': round(ms, 3), 'img_per_s': round(bs / ms * 1e3, 1),
        'last_loss': loss, 'device': torch.cuda.get_device_name(0)}))


def mode_shapes(args):
    sys.path.insert(0, 'tools')
    from conv_microbench import SHAPES
    torch.backends.cudnn.benchmark = True
    lib = require_lib()
    Nb = args.batch
    it, wu = args.steps, args.warmup
    print(f"# f32 conv entry points vs F.conv2d fp32, batch {Nb}, "
          f"HIP-event timed, {wu} warmup + {it} iters, "
          f"{torch.cuda.get_device_name(0)}")
    print(f"{'shape':>20} {'impl':>6} {'fwd us':>9} {'dgrad us':>9} "
          f"{'wgrad us':>9} {'TF fwd':>7} {'TF dx':>7} {'TF dw':>7}")
    for name, C, H, W, K, R, stride, pad in SHAPES:
        P = (H + 2 * pad - R) // stride + 1
        x = torch.randn(Nb, C, H, W, device='cuda') \
            .contiguous(memory_format=_CL)
        w = torch.randn(K, C, R, R, device='cuda').mul(0.05) \
            .contiguous(memory_format=_CL)
        dout = torch.randn(Nb, K, P, P, device='cuda') \
            .contiguous(memory_format=_CL)
        out = torch.empty_like(dout)
        dx = torch.empty_like(x)
        dw = torch.empty_like(w)
        M = Nb * P * P
        split = ps_conv._wgrad_split_f32(M, K, R * R * C)
        partial = torch.empty(split * K * R * R * C, dtype=torch.float32,
                              device='cuda')
        flops = 2.0 * M * K * R * R * C
        strm = current_stream_ptr()

        def fwd():
            lib.ps_conv_fwd_f32(x.data_ptr(), w.data_ptr(), 0,
                                out.data_ptr(), Nb, H, W, C, K, P, P,
                                R, R, stride, pad, strm)

        def bwd_x():
            lib.ps_conv_dgrad_f32(dout.data_ptr(), w.data_ptr(),
                                  dx.data_ptr(), 0, Nb, H, W, C, K, P, P,
                                  R, R, stride, pad, strm)

        def bwd_w():
            lib.ps_conv_wgrad_f32(dout.data_ptr(), x.data_ptr(),
                                  partial.data_ptr(), dw.data_ptr(),
                                  Nb, H, W, C, K, P, P, R, R, stride,
                                  pad, split, strm)

        xg = x.clone().requires_grad_(True)
        og = F.conv2d(xg, w, None, stride=stride, padding=pad)
        wg = w.clone().requires_grad_(True)
        og2 = F.conv2d(x, wg, None, stride=stride, padding=pad)

        def t_fwd():
            return F.conv2d(x, w, None, stride=stride, padding=pad)

        def t_bwd_x():
            return torch.autograd.grad(og, xg, dout, retain_graph=True)

        def t_bwd_w():
            return torch.autograd.grad(og2, wg, dout, retain_graph=True)

        for impl, fns in (('ps', (fwd, bwd_x, bwd_w)),
                          ('torch', (t_fwd, t_bwd_x, t_bwd_w))):
            us = [event_time_ms(f, it, wu) * 1e3 for f in fns]
            print(f"{name:>20} {impl:>6} {us[0]:>9.1f} {us[1]:>9.1f} "
                  f"{us[2]:>9.1f} {flops / us[0] / 1e6:>7.1f} "
                  f"{flops / us[1] / 1e6:>7.1f} {flops / us[2] / 1e6:>7.1f}")


def mode_curve(args):
    from ps_pytorch_amd.data.synthetic import SyntheticDataset
    tr = _trainer(args, args.dtype)
    bs = args.batch_size
    nb = 8
    ds = SyntheticDataset(args.dataset, size=nb * bs, seed=args.seed)
    xs = ds.x.to('cuda', tr.compute_dtype)
    ys = ds.y.to('cuda')
    losses = []
    for s in range(args.steps):
        i = (s % nb) * bs
        losses.append(tr.train_step(xs[i:i + bs], ys[i:i + bs]))
    torch.cuda.synchronize()
    tag = args.dtype + (' torch' if args.torch else ' hand')
    # dense early (where the routes can differ visibly), then every N
    marks = sorted({1, 2, 3, 5, 8, 12, 16} |
                   set(range(args.every, args.steps + 1, args.every)))
    pts = {str(s): round(losses[s - 1], 6) for s in marks if s <= args.steps}
    print(json.dumps({'mode': 'curve', 'route': tag, 'network': args.network,
                      'batch_size': bs, 'lr': args.lr, 'seed': args.seed,
                      'first': round(losses[0], 6), 'loss_at_step': pts}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('e2e', 'shapes', 'curve'),
                    default='e2e')
    ap.add_argument('--network', default='ResNet18')
    ap.add_argument('--dataset', default='Cifar10')
    ap.add_argument('--batch-size', type=int, default=256)
    ap.add_argument('--batch', type=int, default=256,
                    help='shapes mode: conv batch')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--lr', type=float, default=0.05)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--dtype', choices=('bf16', 'fp32'), default='fp32',
                    help='curve mode: compute dtype')
    ap.add_argument('--every', type=int, default=20)
    ap.add_argument('--eager', action='store_true',
                    help='e2e mode: no graph capture')
    ap.add_argument('--torch', action='store_true',
                    help='fp32 ops on torch, as with PS_F32=0')
    args = ap.parse_args()
    if args.torch:
        ps_conv._F32 = False
    {'e2e': mode_e2e, 'shapes': mode_shapes, 'curve': mode_curve}[args.mode](args)


if __name__ == '__main__':
    main()
