"""--fan-in fused through the gather-mode PS protocol over gloo (CPU).

The bitwise tests push fixed seeded tensors written into flat_g (no
autograd, so nothing rests on run-to-run conv determinism) and compare the
master weights with the arrival run and with a rank-ordered CPU oracle; the
model-level runs use real worker steps against a serial simulation."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ps_pytorch_amd.config import JobConfig
from ps_pytorch_amd.models import build_model
from ps_pytorch_amd.optim import FlatAdam, FlatSGD
from ps_pytorch_amd.parallel.flat import FlatSpace
from ps_pytorch_amd.ops import functional as ops_f

from dist_utils import run_dist

STEPS = 3
BS = 16
SEED = 5
LR, MOM = 0.1, 0.9
K = 16

CODEC_KW = {
    'raw': dict(compress_grad='None'),
    'q8': dict(compress_grad='compress', compress_codec='q8'),
    'topk': dict(compress_grad='compress', compress_codec='topk', topk_k=K,
                 error_feedback=True),
}


def _cfg(**kw) -> JobConfig:
    base = dict(network='LeNet', dataset='MNIST', batch_size=BS,
                lr=LR, momentum=MOM, seed=SEED, max_steps=STEPS,
                compress_grad='None', wire_dtype='fp32', compute_dtype='fp32',
                overlap=True, aggregation='gather', num_aggregate=64,
                bucket_mb=0.25, log_interval=10 ** 9, eval_freq=10 ** 9)
    base.update(kw)
    return JobConfig(**base)


def _fixed_grad(rank: int, step: int, n: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(7000 + 100 * rank + step)
    return torch.randn(n, generator=g) * 0.01


# ---- fixed-gradient roles: bitwise ----

def _role_fixed(rank: int, world: int, port: int, cfg_kw: dict,
                delays: dict):
    """Workers push _fixed_grad(rank, step) instead of a backward's result;
    `delays` maps rank -> seconds slept before each step's pushes."""
    from ps_pytorch_amd.parallel.transport import init_distributed
    from ps_pytorch_amd.parallel.ps import ParameterServer
    from ps_pytorch_amd.parallel.worker import DistributedWorker
    cfg = _cfg(overlap=False, **cfg_kw)
    env = init_distributed(backend='gloo')
    if rank == 0:
        ps = ParameterServer(cfg, rank, world, env['device'])
        ps.build_model(10)
        assert ps.fan_in == cfg.fan_in
        for _ in range(STEPS):
            ps.step()
        return ps.master_w[:ps.flat.total].clone()
    w = DistributedWorker(cfg, rank, world, env['device'])
    w.build_model(10)
    for step in range(STEPS):
        w.fetch_weights()
        w.flat.flat_g.copy_(_fixed_grad(rank, step, w.flat.padded))
        w._reset_bucket_state()
        if delays.get(rank):
            time.sleep(delays[rank])
        w.push_gradients()
    return None


def _oracle(codec: str, workers, scale: float) -> torch.Tensor:
    """Rank-ordered CPU oracle of the fixed-gradient job: per step and
    bucket, encode every worker's slice as its push does (top-k with the
    worker's carried residual), fold `workers` in ascending rank with
    fanin_sgd at the one averaging scale."""
    torch.manual_seed(SEED)
    net = build_model('LeNet', num_classes=10, in_channels=1)
    fs = FlatSpace(net, bucket_bytes=int(0.25 * 2 ** 20))
    master = fs.flat_w.detach().to(torch.float32).clone()
    mom = torch.zeros_like(master)
    residual = {r: torch.zeros(fs.padded) for r in workers}
    for step in range(STEPS):
        grads = {r: _fixed_grad(r, step, fs.padded) for r in workers}
        for b in fs.buckets:
            srcs = []
            for r in sorted(workers):
                g = grads[r][b.start:b.end]
                if codec == 'raw':
                    srcs.append(g.clone())
                elif codec == 'q8':
                    p = torch.zeros(ops_f.q8_layout(b.numel)[1],
                                    dtype=torch.uint8)
                    ops_f.pack_q8(p, g)
                    srcs.append(p)
                else:
                    p = torch.zeros(ops_f.topk_layout(b.numel, K)[1],
                                    dtype=torch.uint8)
                    ops_f.pack_topk_ef(p, g, residual[r][b.start:b.end], K)
                    srcs.append(p)
            ops_f.fanin_sgd(master[b.start:b.end], mom[b.start:b.end], srcs,
                            codec, K if codec == 'topk' else None, LR, MOM,
                            0.0, scale, False)
    return master[:fs.total]


def _bits(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.numpy()
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize('codec', ['raw', 'q8', 'topk'])
def test_fused_equals_arrival_world3(codec):
    """Two-term sums commute and both modes scale by the same float: with
    full quota the fused run reproduces the arrival run bit for bit, which
    pins the new glue to the old path."""
    kw = CODEC_KW[codec]
    arrival = run_dist(_role_fixed, world=3,
                       args=(dict(kw, fan_in='arrival'), {}))[0]
    fused = run_dist(_role_fixed, world=3,
                     args=(dict(kw, fan_in='fused'), {}))[0]
    assert np.array_equal(_bits(arrival), _bits(fused))
    assert np.array_equal(_bits(fused),
                          _bits(_oracle(codec, (1, 2), 1.0 / 2)))


def test_arrival_order_does_not_matter_world4():
    """Three-term f32 sums depend on their order; the fused fan-in takes
    them in rank order whichever worker is late."""
    kw = dict(CODEC_KW['q8'], fan_in='fused')
    a = run_dist(_role_fixed, world=4, args=(kw, {1: 0.3}))[0]
    b = run_dist(_role_fixed, world=4, args=(kw, {2: 0.3, 3: 0.15}))[0]
    assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(a), _bits(_oracle('q8', (1, 2, 3), 1.0 / 3)))


def test_first_k_selection_world4():
    """num_aggregate=2 with rank 3 late: ranks 1 and 2 are the counted set,
    averaged with the single scale 1/2."""
    kw = dict(CODEC_KW['raw'], fan_in='fused', num_aggregate=2)
    got = run_dist(_role_fixed, world=4, args=(kw, {3: 0.5}))[0]
    assert np.array_equal(_bits(got), _bits(_oracle('raw', (1, 2), 1.0 / 2)))


# ---- model-level runs: real worker steps ----

def _batches(rank: int, same: bool = False):
    g = torch.Generator().manual_seed(1000 + (0 if same else rank))
    xs = [torch.randn(BS, 1, 28, 28, generator=g) for _ in range(STEPS)]
    ys = [torch.randint(0, 10, (BS,), generator=g) for _ in range(STEPS)]
    return xs, ys


def _role(rank: int, world: int, port: int, cfg_kw: dict, same_data: bool,
          slow_rank: int = -1, slow_s: float = 0.0):
    from ps_pytorch_amd.parallel.transport import init_distributed
    from ps_pytorch_amd.parallel.ps import ParameterServer
    from ps_pytorch_amd.parallel.worker import DistributedWorker
    cfg = _cfg(**cfg_kw)
    env = init_distributed(backend='gloo')
    if rank == 0:
        ps = ParameterServer(cfg, rank, world, env['device'])
        ps.build_model(10)
        assert ps.fan_in == 'fused'
        for _ in range(STEPS):
            ps.step()
        return ps.master_w[:ps.flat.total].clone()
    w = DistributedWorker(cfg, rank, world, env['device'])
    w.build_model(10)
    if rank == slow_rank and slow_s:
        # straggle inside the step, after the synchronizing broadcast
        w.network.register_forward_pre_hook(lambda *a: time.sleep(slow_s))
    xs, ys = _batches(rank, same=same_data)
    kills = 0
    for i in range(STEPS):
        if w.train_step(xs[i], ys[i]) is None:
            kills += 1
    return kills


def _serial(make_opt, workers=(1, 2)) -> torch.Tensor:
    """Serial simulation: per-step summed worker grads -> flat optimizer."""
    torch.manual_seed(SEED)
    net = build_model('LeNet', num_classes=10, in_channels=1)
    fs = FlatSpace(net, bucket_bytes=int(0.25 * 2 ** 20))
    fs.attach_grads()
    master = fs.flat_w.detach().to(torch.float32).clone()
    opt = make_opt(master)
    data = {r: _batches(r) for r in workers}
    for step in range(STEPS):
        grad_sum = torch.zeros_like(master)
        for r in workers:
            fs.load_flat(master)
            fs.zero_grads()
            xs, ys = data[r]
            F.cross_entropy(net(xs[step]).float(), ys[step]).backward()
            grad_sum += fs.flat_g
        opt.step(grad_sum, grad_scale=1.0 / len(workers))
    return master[:fs.total]


def test_fused_golden_sgd():
    res = run_dist(_role, world=3, args=({'fan_in': 'fused'}, False))
    got = torch.from_numpy(res[0])
    ref = _serial(lambda w: FlatSGD(w, lr=LR, momentum=MOM))
    assert torch.allclose(got, ref, atol=1e-5, rtol=1e-5), (got - ref).abs().max()


def test_fused_golden_adam():
    res = run_dist(_role, world=3,
                   args=({'fan_in': 'fused', 'optimizer': 'adam',
                          'lr': 1e-3}, False))
    got = torch.from_numpy(res[0])
    ref = _serial(lambda w: FlatAdam(w, lr=1e-3))
    assert torch.allclose(got, ref, atol=1e-5, rtol=1e-5), (got - ref).abs().max()
    # three steps of Adam moved the weights (t advanced once per step, not
    # once per bucket: a per-bucket advance changes the bias correction)
    torch.manual_seed(SEED)
    w0 = FlatSpace(build_model('LeNet', num_classes=10, in_channels=1)
                   ).flat_w[:got.numel()]
    assert (got - w0).abs().max() > 1e-3


def test_fused_kill_mode_aborts_straggler():
    """kill mode + num_aggregate=1 under the fused fan-in: quota from the
    fast worker fires the verdict while rank 2 sleeps; rank 2 aborts its
    backward, training stays live."""
    res = run_dist(_role, world=3,
                   args=({'num_aggregate': 1, 'mode': 'kill',
                          'fan_in': 'fused'}, True, 2, 1.5),
                   timeout=300.0)
    assert res[2] >= 1, f"straggler was never killed: {res}"
    assert res[0] is not None
