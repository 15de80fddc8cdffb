"""--compress-codec topk through the gather-mode PS protocol over gloo (CPU):
the PS result equals a serial simulation that keeps one residual per worker
and runs pack_topk_ef / unpack_topk, differs from the q8 run, and aborted
steps leave the residual untouched."""
import torch
import torch.nn.functional as F

from ps_pytorch_amd.config import JobConfig
from ps_pytorch_amd.models import build_model
from ps_pytorch_amd.optim import FlatSGD
from ps_pytorch_amd.parallel.flat import FlatSpace
from ps_pytorch_amd.ops import functional as ops_f

from dist_utils import run_dist

STEPS = 3
BS = 16
SEED = 5
LR, MOM = 0.1, 0.9
WORKERS = (1, 2)
K = 16


def _cfg(**kw) -> JobConfig:
    base = dict(network='LeNet', dataset='MNIST', batch_size=BS,
                lr=LR, momentum=MOM, seed=SEED, max_steps=STEPS,
                compress_grad='compress', wire_dtype='fp32',
                compute_dtype='fp32', overlap=True, aggregation='gather',
                num_aggregate=64, bucket_mb=0.25, error_feedback=True,
                compress_codec='topk', topk_k=K,
                log_interval=10 ** 9, eval_freq=10 ** 9)
    base.update(kw)
    return JobConfig(**base)


def _batches(rank: int):
    g = torch.Generator().manual_seed(1000 + rank)
    xs = [torch.randn(BS, 1, 28, 28, generator=g) for _ in range(STEPS)]
    ys = [torch.randint(0, 10, (BS,), generator=g) for _ in range(STEPS)]
    return xs, ys


def _role(rank: int, world: int, port: int, cfg_kw: dict):
    from ps_pytorch_amd.parallel.transport import init_distributed
    from ps_pytorch_amd.parallel.ps import ParameterServer
    from ps_pytorch_amd.parallel.worker import DistributedWorker
    cfg = _cfg(**cfg_kw)
    env = init_distributed(backend='gloo')
    if rank == 0:
        ps = ParameterServer(cfg, rank, world, env['device'])
        ps.build_model(10)
        for _ in range(STEPS):
            ps.step()
        return ps.master_w[:ps.flat.total].clone()
    w = DistributedWorker(cfg, rank, world, env['device'])
    w.build_model(10)
    assert w.transport.ef_active
    assert w.transport.codec == cfg.compress_codec
    xs, ys = _batches(rank)
    kills = sum(w.train_step(xs[i], ys[i]) is None for i in range(STEPS))
    return kills, float(w.transport.residual.abs().max())


def _serial(codec: str) -> torch.Tensor:
    """Serial simulation of the wire: per worker and bucket, encode with the
    worker's carried residual, decode into the sum, FlatSGD."""
    torch.manual_seed(SEED)
    net = build_model('LeNet', num_classes=10, in_channels=1)
    fs = FlatSpace(net, bucket_bytes=int(0.25 * 2 ** 20))  # match bucket_mb
    fs.attach_grads()
    master = fs.flat_w.detach().to(torch.float32).clone()
    opt = FlatSGD(master, lr=LR, momentum=MOM)
    data = {r: _batches(r) for r in WORKERS}
    residual = {r: torch.zeros(fs.padded) for r in WORKERS}
    for step in range(STEPS):
        grad_sum = torch.zeros_like(master)
        for r in WORKERS:
            fs.load_flat(master)
            fs.zero_grads()
            xs, ys = data[r]
            F.cross_entropy(net(xs[step]).float(), ys[step]).backward()
            g = fs.flat_g.clone()
            for b in fs.buckets:
                res = residual[r][b.start:b.end]
                acc = grad_sum[b.start:b.end]
                if codec == 'topk':
                    _, tot = ops_f.topk_layout(b.numel, K)
                    payload = torch.zeros(tot, dtype=torch.uint8)
                    ops_f.pack_topk_ef(payload, g[b.start:b.end], res, K)
                    ops_f.unpack_topk(acc, payload, K, accumulate=True)
                else:
                    _, tot = ops_f.q8_layout(b.numel)
                    payload = torch.zeros(tot, dtype=torch.uint8)
                    ops_f.pack_q8_ef(payload, g[b.start:b.end], res)
                    ops_f.unpack_q8(acc, payload, accumulate=True)
        opt.step(grad_sum, grad_scale=1.0 / len(WORKERS))
    return master[:fs.total]


def test_gather_golden_topk():
    res = run_dist(_role, world=3, args=({},))
    got = torch.from_numpy(res[0])
    ref = _serial('topk')
    assert torch.allclose(got, ref, atol=1e-5, rtol=1e-5), (got - ref).abs().max()
    assert all(res[r][0] == 0 and res[r][1] > 0 for r in WORKERS)
    # the sparse codec really ran: neither the serial q8 simulation nor the
    # q8 run of the same job gives this result
    assert not torch.allclose(got, _serial('q8'), atol=1e-5, rtol=1e-5)
    q8 = run_dist(_role, world=3, args=({'compress_codec': 'q8'},))
    assert not torch.allclose(got, torch.from_numpy(q8[0]),
                              atol=1e-5, rtol=1e-5)


def _role_codec_mismatch(rank: int, world: int, port: int):
    """Ranks launched with different codec settings frame their payloads
    differently: the layout fingerprint must catch it at transport init."""
    from ps_pytorch_amd.parallel.transport import PSTransport, init_distributed
    env = init_distributed(backend='gloo')
    torch.manual_seed(0)
    fs = FlatSpace(build_model('LeNet', num_classes=10, in_channels=1))
    kw = [dict(codec='topk', topk_k=16), dict(codec='topk', topk_k=8),
          dict(codec='q8')][rank]
    try:
        PSTransport(fs, torch.float32, env['device'], rank, world,
                    mode='gather', compress=True, **kw)
        return 'no error'
    except RuntimeError as e:
        return 'raised' if 'fingerprint' in str(e) else f'other: {e}'


def test_codec_mismatch_raises_at_transport_init():
    res = run_dist(_role_codec_mismatch, world=3)
    assert res[0] == 'no error'      # rank 0 is the reference fingerprint
    assert res[1] == 'raised' and res[2] == 'raised', res


def test_killed_steps_leave_residual_untouched():
    """timeout mode with an instant threshold: every step aborts at the
    first backward hook, only all-zero payloads go out, and the residual
    must stay exactly zero; the PS decodes them and completes."""
    res = run_dist(_role, world=3,
                   args=({'mode': 'timeout', 'kill_threshold': 0.0},))
    for r in WORKERS:
        kills, resid_max = res[r]
        assert kills == STEPS
        assert resid_max == 0.0
    assert res[0] is not None
