"""--error-feedback through the gather-mode PS protocol over gloo (CPU):
the PS result equals a serial simulation that keeps one residual per worker,
differs from the same run without feedback, and aborted steps leave the
residual untouched."""
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


def _cfg(**kw) -> JobConfig:
    base = dict(network='LeNet', dataset='MNIST', batch_size=BS,
                lr=LR, momentum=MOM, seed=SEED, max_steps=STEPS,
                compress_grad='compress', wire_dtype='fp32',
                compute_dtype='fp32', overlap=True, aggregation='gather',
                num_aggregate=64, bucket_mb=0.25, error_feedback=True,
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
    xs, ys = _batches(rank)
    kills = sum(w.train_step(xs[i], ys[i]) is None for i in range(STEPS))
    return kills, float(w.transport.residual.abs().max())


def _serial(feedback: bool) -> torch.Tensor:
    """Serial simulation of the q8 wire: per worker and bucket, encode with
    (feedback) or without the worker's carried residual, decode, sum,
    FlatSGD."""
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
                _, tot = ops_f.q8_layout(b.numel)
                payload = torch.zeros(tot, dtype=torch.uint8)
                if feedback:
                    ops_f.pack_q8_ef(payload, g[b.start:b.end],
                                     residual[r][b.start:b.end])
                else:
                    ops_f.pack_q8(payload, g[b.start:b.end])
                ops_f.unpack_q8(grad_sum[b.start:b.end], payload,
                                accumulate=True)
        opt.step(grad_sum, grad_scale=1.0 / len(WORKERS))
    return master[:fs.total]


def test_gather_golden_q8_error_feedback():
    res = run_dist(_role, world=3, args=({},))
    got = torch.from_numpy(res[0])
    ref = _serial(feedback=True)
    assert torch.allclose(got, ref, atol=1e-5, rtol=1e-5), (got - ref).abs().max()
    # the residual is really applied: the run is NOT the plain q8 roundtrip
    plain = _serial(feedback=False)
    assert not torch.allclose(got, plain, atol=1e-5, rtol=1e-5)
    assert all(res[r][0] == 0 and res[r][1] > 0 for r in WORKERS)


def test_killed_steps_leave_residual_untouched():
    """timeout mode with an instant threshold: every step aborts at the
    first backward hook, only zero payloads go out, and the residual must
    stay exactly zero; the PS still completes."""
    res = run_dist(_role, world=3,
                   args=({'mode': 'timeout', 'kill_threshold': 0.0},))
    for r in WORKERS:
        kills, resid_max = res[r]
        assert kills == STEPS
        assert resid_max == 0.0
    assert res[0] is not None
