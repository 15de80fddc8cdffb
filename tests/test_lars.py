"""LARS and the LR schedule on the CPU: the schedule against closed forms,
the reference path of ops.functional against a plain per-tensor loop, the
region / advance contract, flags and wiring, and the distributed engines
against a single-process reference (gloo)."""
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from ps_pytorch_amd.config import JobConfig, parse_args
from ps_pytorch_amd.models import build_model
from ps_pytorch_amd.ops import functional as F
from ps_pytorch_amd.optim import (FlatAdam, FlatLARS, FlatSGD, HostLR,
                                  LRSchedule, build_optimizer)
from ps_pytorch_amd.parallel.flat import FlatSpace

from dist_utils import run_dist
from lars_utils import (f32_bits, own_mask, synthetic_buckets,
                        synthetic_segments)


def f32(x: float) -> float:
    return float(np.float32(x))


# ---- the schedule ----

BASE, TOTAL, WARM = 0.8, 50, 5


def _closed(kind, step, decay=7, gamma=0.5):
    t, span = step - WARM, TOTAL - WARM
    if kind == 'constant':
        return BASE
    if kind == 'step':
        return BASE * gamma ** (t // decay)
    if kind == 'poly':
        return BASE * (1 - t / span) ** 2
    return BASE * (1 + math.cos(math.pi * t / span)) / 2


@pytest.mark.parametrize('kind', ['constant', 'step', 'poly', 'cosine'])
def test_schedule_closed_forms(kind):
    s = LRSchedule(BASE, kind, total_steps=TOTAL, warmup_steps=WARM,
                   decay_steps=7, gamma=0.5)
    assert s.lr_at(0) == f32(BASE / WARM)             # first step
    assert s.lr_at(WARM - 1) == f32(BASE)             # last warmup step
    assert s.lr_at(WARM) == f32(BASE)                 # first step after it
    assert s.lr_at(WARM + 1) == f32(_closed(kind, WARM + 1))
    assert s.lr_at(TOTAL - 1) == f32(_closed(kind, TOTAL - 1))   # final
    assert s.lr_at(TOTAL + 9) == s.lr_at(TOTAL - 1)   # held past the end
    if kind == 'poly':
        assert s.lr_at(TOTAL - 1) == f32(BASE / (TOTAL - WARM) ** 2)
    if kind == 'step':
        assert s.lr_at(WARM + 7) == f32(BASE * 0.5)
        assert s.lr_at(WARM + 6) == f32(BASE)
    tab = s.table()
    assert tab.dtype == torch.float32 and tab.numel() == TOTAL
    assert tab.tolist() == [s.lr_at(i) for i in range(TOTAL)]
    # without warmup the first step is the base rate
    s0 = LRSchedule(BASE, kind, total_steps=TOTAL, decay_steps=7)
    assert s0.lr_at(0) == f32(BASE)
    assert s0.is_constant == (kind == 'constant')
    assert not s.is_constant


def test_schedule_rejects_bad_arguments():
    with pytest.raises(ValueError):
        LRSchedule(0.1, 'linear', total_steps=10)
    with pytest.raises(ValueError):
        LRSchedule(0.1, 'step', total_steps=10)        # no decay_steps
    with pytest.raises(ValueError):
        LRSchedule(0.1, 'poly', total_steps=0)


# ---- the reference LARS ----

LR, MU, WD, ETA, EPS = 0.5, 0.9, 5e-4, 1e-2, 1e-8


def _inputs(seed=0, gdtype=torch.float32):
    segs, total = synthetic_segments()
    g = torch.Generator().manual_seed(seed)
    own = own_mask(segs, total)
    w = torch.randn(total, generator=g)
    grad = (torch.randn(total, generator=g) * 0.01) * own   # gaps: zero grad
    m = torch.randn(total, generator=g) * 0.01 * own
    return segs, total, w, grad.to(gdtype), m


def _lars(w, segs, kind='constant', total_steps=10, **kw):
    sched = LRSchedule(LR, kind, total_steps=total_steps,
                       decay_steps=kw.pop('decay_steps', 0),
                       gamma=kw.pop('gamma', 0.1))
    return FlatLARS(w, segs, sched, momentum=MU, weight_decay=WD, eta=ETA,
                    eps=EPS, **kw)


@pytest.mark.parametrize('gdtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('scale', [1.0, 1.0 / 7])
def test_reference_matches_per_tensor_loop(gdtype, scale):
    segs, total, w0, grad, m0 = _inputs(1, gdtype)
    w = w0.clone()
    opt = _lars(w, segs)
    opt.m.copy_(m0)
    wire = torch.zeros(total, dtype=torch.bfloat16)
    opt.step(grad, grad_scale=scale, wire_out=wire)
    assert int(opt.step_ctr) == 1 and opt.lr == f32(LR)
    for s, (off, n, ndim) in enumerate(segs):
        ws, gs = w0[off:off + n], grad[off:off + n].float()
        wn = float(ws.double().norm())
        gn = scale * float(gs.double().norm())
        ratio = ETA * wn / (gn + WD * wn + EPS) if ndim > 1 else 1.0
        wd = WD if ndim > 1 else 0.0
        llr = f32(f32(LR) * ratio)
        # sqrt of a differently ordered float64 sum: a few f64 ulps
        assert float(opt.layout.local_lr[s]) == pytest.approx(llr, rel=1e-6)
        assert float(opt.layout.wd_seg[s]) == f32(wd)
        gk = gs * scale + wd * ws
        m = MU * m0[off:off + n] + llr * gk
        assert torch.allclose(opt.m[off:off + n], m, rtol=1e-5, atol=1e-7)
        assert torch.allclose(w[off:off + n], ws - m, rtol=1e-5, atol=1e-6)
    assert torch.equal(wire, w.to(torch.bfloat16))
    # alignment gaps: zero gradient and momentum, no decay on 1-D tensors;
    # behind a decayed tensor the gap weight only decays
    assert torch.isfinite(w).all()


def test_one_dim_tensors_get_ratio_one_and_no_decay():
    segs, total, w, grad, _ = _inputs(2)
    opt = _lars(w.clone(), segs)
    opt.step(grad)
    for s, (_, _, ndim) in enumerate(segs):
        if ndim == 1:
            assert float(opt.layout.local_lr[s]) == f32(LR)
            assert float(opt.layout.wd_seg[s]) == 0.0
        else:
            assert float(opt.layout.local_lr[s]) != f32(LR)
            assert float(opt.layout.wd_seg[s]) == f32(WD)


@pytest.mark.parametrize('zero', ['w', 'g'])
def test_zero_norm_gives_ratio_one_and_finite_outputs(zero):
    segs, total, w, grad, _ = _inputs(3)
    if zero == 'w':
        w.zero_()
    else:
        grad.zero_()
    w = w.clone()
    opt = _lars(w, segs)
    opt.step(grad)
    assert (opt.layout.local_lr == f32(LR)).all()
    assert torch.isfinite(w).all() and torch.isfinite(opt.m).all()
    col = 0 if zero == 'w' else 1
    assert not opt.layout.seg_sums[:, col].any()


def test_region_steps_equal_one_full_step_bitwise():
    segs, total, w0, grad, m0 = _inputs(4)
    full_w, part_w = w0.clone(), w0.clone()
    full = _lars(full_w, segs, 'step', decay_steps=1, gamma=0.5)
    part = _lars(part_w, segs, 'step', decay_steps=1, gamma=0.5)
    fw, pw = torch.zeros(total), torch.zeros(total)
    for step in range(3):
        full.step(grad, grad_scale=0.5, wire_out=fw)
        for i, region in enumerate(synthetic_buckets(segs, total)):
            part.step(grad, grad_scale=0.5, wire_out=pw, region=region,
                      advance=(i == 0))
        assert int(part.step_ctr) == step + 1
        assert part.lr == f32(LR * 0.5 ** step)
        assert np.array_equal(f32_bits(full_w), f32_bits(part_w))
        assert np.array_equal(f32_bits(full.m), f32_bits(part.m))
        assert torch.equal(fw, pw)
    with pytest.raises(ValueError):
        part.step(grad, region=(4, total))      # not a parameter start


def test_gap_weights_do_not_change_norms_cpu():
    segs, total, w, grad, _ = _inputs(5)
    a = _lars(w.clone(), segs)
    a.step(grad)
    w2 = w.clone()
    w2[~own_mask(segs, total)] = 1e6
    b = _lars(w2, segs)
    b.step(grad)
    assert torch.equal(a.layout.seg_sums, b.layout.seg_sums)
    assert torch.equal(a.layout.local_lr, b.layout.local_lr)


def test_start_step_and_state_dict_round_trip():
    segs, total, w, grad, _ = _inputs(6)
    a = _lars(w.clone(), segs, 'step', decay_steps=2, gamma=0.5, start_step=3)
    assert int(a.step_ctr) == 3
    a.step(grad)
    assert a.lr == f32(LR * 0.5) and int(a.step_ctr) == 4
    sd = a.state_dict()
    assert sd['step'] == 4 and torch.equal(sd['momentum_buffer'], a.m)
    b = _lars(a.w.clone(), segs, 'step', decay_steps=2, gamma=0.5)
    b.load_state_dict(sd)
    a.step(grad)
    b.step(grad)
    assert torch.equal(a.w, b.w) and torch.equal(a.m, b.m)
    assert b.lr == f32(LR * 0.25)


def test_flatspace_segments():
    fs = FlatSpace(build_model('LeNet', num_classes=10, in_channels=1))
    segs = fs.segments()
    assert segs == [(off, p.numel(), p.dim())
                    for p, off in zip(fs.params, fs.offsets)]
    lay = F.LarsLayout(segs, fs.padded)
    for b in fs.buckets:            # every bucket is a valid region
        s0, s1, c0, c1, st, en = lay.ranges((b.start, b.end))
        assert (st, en) == (b.start, b.end) and s1 > s0 and c1 > c0
        assert list(range(s0, s1)) == b.param_ids


# ---- flags and wiring ----

def test_jobconfig_normalisation():
    cfg = JobConfig()
    assert (cfg.weight_decay, cfg.lars_eta, cfg.lr_schedule, cfg.warmup_steps,
            cfg.lr_decay_steps, cfg.lr_decay_gamma) == (0.0, 1e-3, 'constant',
                                                        0, 0, 0.1)
    assert JobConfig(optimizer='lars').optimizer == 'lars'
    with pytest.raises(ValueError):
        JobConfig(optimizer='lamb')
    with pytest.raises(ValueError):
        JobConfig(lr_schedule='linear')
    with pytest.raises(ValueError):
        JobConfig(lr_schedule='step')                    # no decay steps
    with pytest.raises(ValueError):
        JobConfig(weight_decay=-1.0)
    with pytest.warns(UserWarning, match='warmup'):
        cfg = JobConfig(max_steps=10, warmup_steps=10)
    assert cfg.warmup_steps == 9
    args = parse_args(['--optimizer', 'lars', '--weight-decay', '5e-4',
                       '--lars-eta', '0.02', '--lr-schedule', 'step',
                       '--warmup-steps', '3', '--lr-decay-steps', '40',
                       '--lr-decay-gamma', '0.2', '--max-steps', '100'])
    cfg = JobConfig.from_args(args)
    assert (cfg.optimizer, cfg.weight_decay, cfg.lars_eta, cfg.lr_schedule,
            cfg.warmup_steps, cfg.lr_decay_steps, cfg.lr_decay_gamma) == (
                'lars', 5e-4, 0.02, 'step', 3, 40, 0.2)


def _trainer(**kw):
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='LeNet', dataset='MNIST', batch_size=8,
                    compute_dtype='fp32', **kw)
    tr = NNTrainer(cfg, device=torch.device('cpu'))
    tr.build_model()
    return tr


def test_weight_decay_reaches_sgd_and_adam():
    tr = _trainer(weight_decay=5e-4)
    assert isinstance(tr.optimizer, FlatSGD)
    assert tr.optimizer.weight_decay == 5e-4 and tr._host_lr is None
    tr = _trainer(weight_decay=5e-4, optimizer='adam')
    assert isinstance(tr.optimizer, FlatAdam)
    assert tr.optimizer.weight_decay == 5e-4
    assert _trainer().optimizer.weight_decay == 0.0
    # and it acts: one step with a zero gradient moves the weights
    w = torch.ones(8)
    cfg = JobConfig(weight_decay=0.5, lr=0.1, momentum=0.0)

    class _Flat:
        def segments(self):
            return [(0, 8, 2)]
    opt, host = build_optimizer(cfg, w, _Flat())
    opt.step(torch.zeros(8))
    assert host is None and torch.allclose(w, torch.full((8,), 0.95))


def test_host_schedule_drives_sgd_on_the_eager_path():
    tr = _trainer(lr=0.1, lr_schedule='poly', warmup_steps=2, max_steps=6)
    assert isinstance(tr._host_lr, HostLR)
    sched = LRSchedule(0.1, 'poly', total_steps=6, warmup_steps=2)
    x, y = torch.randn(8, 1, 28, 28), torch.randint(0, 10, (8,))
    for step in range(4):
        tr.train_step(x, y)
        assert tr.optimizer.lr == sched.lr_at(step)
    # --resume-step starts the schedule there
    cfg = JobConfig(lr=0.1, lr_schedule='poly', max_steps=6)
    cfg.resume_step = 3

    class _Flat:
        def segments(self):
            return [(0, 8, 2)]
    opt, host = build_optimizer(cfg, torch.ones(8), _Flat())
    host.tick()
    assert opt.lr == LRSchedule(0.1, 'poly', total_steps=6).lr_at(3)
    cfg.optimizer = 'lars'
    opt, host = build_optimizer(cfg, torch.ones(8), _Flat())
    assert host is None and int(opt.step_ctr) == 3


def test_graph_is_cpu_noop_and_lars_trainer_builds():
    tr = _trainer(optimizer='lars', lr_schedule='cosine', max_steps=9,
                  weight_decay=1e-4, lars_eta=0.01, momentum=0.9)
    assert isinstance(tr.optimizer, FlatLARS) and tr._host_lr is None
    assert tr.optimizer.eta == 0.01 and tr.optimizer.weight_decay == 1e-4
    assert tr.optimizer.lr_table.numel() == 9
    assert tr.enable_graph(torch.randn(8, 1, 28, 28),
                           torch.randint(0, 10, (8,))) is False


def test_lenet_lars_poly_warmup_loss_decreases():
    from ps_pytorch_amd.data import prepare_data
    from ps_pytorch_amd.trainer import NNTrainer
    args = parse_args(['--optimizer', 'lars', '--lr-schedule', 'poly',
                       '--warmup-steps', '5', '--max-steps', '30',
                       '--batch-size', '64', '--lr', '0.5', '--lars-eta',
                       '0.02', '--momentum', '0.9', '--weight-decay', '1e-4',
                       '--log-interval', '1000'])
    cfg = JobConfig.from_args(args)
    tr = NNTrainer(cfg, device=torch.device('cpu'))
    tr.build_model()
    train_loader, _ = prepare_data(cfg, device=tr.device, train_size=2048,
                                   test_size=256)
    losses = []
    for i, (x, y) in enumerate(train_loader):
        if i >= 30:
            break
        losses.append(tr.train_step(x, y))
    assert int(tr.optimizer.step_ctr) == 30
    assert losses[-1] < losses[0] * 0.8, losses[:3] + losses[-3:]


def test_fused_apply_lars_cpu():
    from ps_pytorch_amd.parallel.transport import PSTransport
    torch.manual_seed(0)
    fs = FlatSpace(build_model('LeNet', num_classes=10, in_channels=1),
                   bucket_bytes=16384)
    assert len(fs.buckets) >= 4
    t = PSTransport(fs, torch.float32, torch.device('cpu'), rank=0, world=4,
                    mode='gather')
    g = torch.Generator().manual_seed(8)
    for st in t.stages:
        st.copy_(torch.randn(fs.padded, generator=g) * 0.01)
    w0 = fs.flat_w.detach().float().clone()
    got, ref = w0.clone(), w0.clone()
    opt, ropt = _lars(got, fs.segments()), _lars(ref, fs.segments())
    wire, rwire = torch.zeros(fs.padded), torch.zeros(fs.padded)
    sets = [[1, 2, 3], [1, 3], []]
    for step in range(2):
        for i, b in enumerate(fs.buckets):
            ws = sets[i % 3]
            t.fused_apply(b, ws, opt, wire_out=wire, advance=(i == 0))
            gsum = torch.zeros(fs.padded)
            for wk in ws:                      # ascending worker rank
                gsum[b.start:b.end] += t.stages[wk - 1][b.start:b.end]
            ropt.step(gsum, grad_scale=1.0 / len(ws) if ws else 1.0,
                      wire_out=rwire, region=(b.start, b.end),
                      advance=(i == 0))
        assert int(opt.step_ctr) == step + 1
        assert torch.equal(got, ref) and torch.equal(opt.m, ropt.m)
        assert torch.equal(wire, rwire)
    assert not torch.equal(got, w0)


# ---- the distributed engines (gloo) ----

STEPS, BS, SEED = 3, 16, 5


def _dist_cfg(engine: str) -> JobConfig:
    return JobConfig(network='LeNet', dataset='MNIST', batch_size=BS,
                     lr=0.5, momentum=0.9, seed=SEED, max_steps=STEPS,
                     compress_grad='None', wire_dtype='fp32',
                     compute_dtype='fp32', overlap=True, bucket_mb=0.25,
                     engine=engine, optimizer='lars', weight_decay=1e-4,
                     lars_eta=0.02, lr_schedule='poly', warmup_steps=1,
                     log_interval=10 ** 9, eval_freq=10 ** 9)


def _batches(rank: int):
    g = torch.Generator().manual_seed(1000 + rank)
    xs = [torch.randn(BS, 1, 28, 28, generator=g) for _ in range(STEPS)]
    ys = [torch.randint(0, 10, (BS,), generator=g) for _ in range(STEPS)]
    return xs, ys


def _serial(cfg: JobConfig, ranks) -> torch.Tensor:
    torch.manual_seed(SEED)
    net = build_model('LeNet', num_classes=10, in_channels=1)
    fs = FlatSpace(net, bucket_bytes=int(cfg.bucket_mb * 2 ** 20))
    fs.attach_grads()
    master = fs.flat_w.detach().to(torch.float32).clone()
    opt, host = build_optimizer(cfg, master, fs)
    assert isinstance(opt, FlatLARS) and host is None
    data = {r: _batches(r) for r in ranks}
    for step in range(STEPS):
        grad_sum = torch.zeros_like(master)
        for r in ranks:
            fs.load_flat(master)
            fs.zero_grads()
            xs, ys = data[r]
            TF.cross_entropy(net(xs[step]).float(), ys[step]).backward()
            grad_sum += fs.flat_g
        opt.step(grad_sum, grad_scale=1.0 / len(ranks))
    return master[:fs.total]


def _role_ps(rank: int, world: int, port: int):
    from ps_pytorch_amd.parallel.transport import init_distributed
    from ps_pytorch_amd.parallel.ps import ParameterServer
    from ps_pytorch_amd.parallel.worker import DistributedWorker
    cfg = _dist_cfg('ps')
    env = init_distributed(backend='gloo')
    if rank == 0:
        ps = ParameterServer(cfg, rank, world, env['device'])
        ps.build_model(10)
        for _ in range(STEPS):
            ps.step()
        assert int(ps.optimizer.step_ctr) == STEPS
        return ps.master_w[:ps.flat.total].clone()
    w = DistributedWorker(cfg, rank, world, env['device'])
    w.build_model(10)
    xs, ys = _batches(rank)
    for i in range(STEPS):
        w.train_step(xs[i], ys[i])
    return None


def _role_allreduce(rank: int, world: int, port: int):
    from ps_pytorch_amd.parallel.transport import init_distributed
    from ps_pytorch_amd.parallel.allreduce import AllReduceTrainer
    env = init_distributed(backend='gloo')
    tr = AllReduceTrainer(_dist_cfg('allreduce'), rank, world, env['device'])
    tr.build_model(10)
    xs, ys = _batches(rank)
    for i in range(STEPS):
        tr.train_step(xs[i], ys[i])
    return tr.master_w[:tr.flat.total].clone()


def test_ps_golden_step_lars():
    """World 3, the pipelined per-bucket path (collective + Bcast): region
    steps with advance on the first bucket only."""
    res = run_dist(_role_ps, world=3)
    got = torch.from_numpy(res[0])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ref = _serial(_dist_cfg('ps'), (1, 2))
    assert torch.allclose(got, ref, atol=1e-5, rtol=1e-5), \
        (got - ref).abs().max()


def test_allreduce_golden_step_lars():
    res = run_dist(_role_allreduce, world=2)
    ref = _serial(_dist_cfg('allreduce'), (0, 1))
    for r in (0, 1):
        got = torch.from_numpy(res[r])
        assert torch.allclose(got, ref, atol=1e-5, rtol=1e-5), \
            (got - ref).abs().max()
