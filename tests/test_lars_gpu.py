"""LARS kernels (ops/kernels/lars.hip) on the GPU: exact sums on a lattice,
float64-accurate sums on random inputs, the elementwise update against the
CPU chain, region / replay / schedule equalities bit for bit, graph capture
through the trainer and the fused fan-in glue."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from ps_pytorch_amd.ops import functional as F
from ps_pytorch_amd.optim import FlatLARS, LRSchedule

from lars_utils import (f32_bits, f64_bits, lattice, own_mask,
                        synthetic_buckets, synthetic_segments)

pytestmark = pytest.mark.gpu

LR, MU, WD, ETA, EPS = 0.5, 0.9, 5e-4, 1e-2, 1e-8
GDTYPES = [torch.float32, torch.bfloat16]
SCALES = [1.0, 1.0 / 7]


@functools.lru_cache(maxsize=None)
def _layout():
    return synthetic_segments()


@functools.lru_cache(maxsize=None)
def _draw(kind: str):
    """(w, g, m) on the CPU, built once: g and m are zero in the alignment
    gaps (as in training), w is not."""
    segs, total = _layout()
    own = own_mask(segs, total)
    if kind == 'lattice':
        w, g = lattice(total, 1), lattice(total, 2) * own
        m = lattice(total, 3) * own
    else:
        gen = torch.Generator().manual_seed(7)
        w = torch.randn(total, generator=gen)
        g = torch.randn(total, generator=gen) * 0.01 * own
        m = torch.randn(total, generator=gen) * 0.01 * own
    return w, g, m


def _opt(w, kind='constant', total_steps=10, **kw):
    segs, _ = _layout()
    sched = LRSchedule(kw.pop('lr', LR), kind, total_steps=total_steps,
                       decay_steps=kw.pop('decay_steps', 0),
                       gamma=kw.pop('gamma', 0.1))
    return FlatLARS(w, segs, sched, momentum=MU, weight_decay=WD, eta=ETA,
                    eps=EPS, **kw)


def _norms(opt, g, scale, region=None, advance=True):
    F.lars_norms(opt.layout, opt.w, g, opt.lr_table, opt.step_ctr, opt.lr_cur,
                 scale, opt.eta, opt.weight_decay, opt.eps, region, advance)


def _formula(sw, sg, ndim, scale):
    """local_lr of one segment from its float64 sums, in numpy float64
    (sqrt and / correctly rounded), rounded to f32 once."""
    wn = np.sqrt(np.float64(sw))
    gn = np.float64(scale) * np.sqrt(np.float64(sg))
    ratio = np.float64(1.0)
    if ndim > 1 and wn > 0 and gn > 0:
        ratio = np.float64(ETA) * wn / (gn + np.float64(WD) * wn
                                        + np.float64(EPS))
    return np.float32(np.float64(np.float32(LR)) * ratio)


def _ulps(a, b) -> int:
    return int(np.abs(f32_bits(np.asarray(a, np.float32)).astype(np.int64)
                      - f32_bits(np.asarray(b, np.float32)).astype(np.int64)
                      ).max())


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('gdtype', GDTYPES)
def test_lattice_sums_and_step_sizes_are_exact(gdtype, scale):
    segs, total = _layout()
    w, g, _ = _draw('lattice')
    assert torch.equal(g.to(torch.bfloat16).float(), g)   # exact in bf16
    opt = _opt(w.cuda())
    _norms(opt, g.to(gdtype).cuda(), scale)
    sums = opt.layout.seg_sums.cpu().numpy()
    llr = opt.layout.local_lr.cpu().numpy()
    wds = opt.layout.wd_seg.cpu().numpy()
    w64, g64 = w.numpy().astype(np.float64), g.numpy().astype(np.float64)
    for s, (off, n, ndim) in enumerate(segs):
        sw = np.sum(w64[off:off + n] ** 2)
        sg = np.sum(g64[off:off + n] ** 2)
        print(f"seg {s} n={n} Sw={sums[s, 0]!r}/{sw!r} Sg={sums[s, 1]!r}/"
              f"{sg!r} llr={llr[s]!r}/{_formula(sw, sg, ndim, scale)!r}")
        assert f64_bits(sums[s, 0]) == f64_bits(sw), (s, n)
        assert f64_bits(sums[s, 1]) == f64_bits(sg), (s, n)
        assert f32_bits(llr[s]) == f32_bits(_formula(sw, sg, ndim, scale)), \
            (s, n, ndim)
        assert wds[s] == (np.float32(WD) if ndim > 1 else 0.0)
    assert int(opt.step_ctr) == 1


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('gdtype', GDTYPES)
def test_random_sums_within_f64_accumulation_bound(gdtype, scale):
    segs, total = _layout()
    w, g, _ = _draw('random')
    gd = g.to(gdtype)
    opt = _opt(w.cuda())
    _norms(opt, gd.cuda(), scale)
    sums = opt.layout.seg_sums.cpu().numpy()
    llr = opt.layout.local_lr.cpu().numpy()
    w64 = w.numpy().astype(np.float64)
    g64 = gd.float().numpy().astype(np.float64)
    for s, (off, n, ndim) in enumerate(segs):
        # squares of f32 values are exact in float64: fsum is the true sum
        sw = math.fsum((w64[off:off + n] ** 2).tolist())
        sg = math.fsum((g64[off:off + n] ** 2).tolist())
        bound = n * 2.0 ** -52
        ew, eg = abs(sums[s, 0] - sw) / sw, abs(sums[s, 1] - sg) / sg
        u = _ulps(llr[s], _formula(sw, sg, ndim, scale))
        print(f"seg {s} n={n} relerr Sw={ew:.3e} Sg={eg:.3e} "
              f"bound={bound:.3e} llr ulps={u}")
        assert ew <= bound and eg <= bound, (s, n, ew, eg, bound)
        assert u <= 1, (s, n, ndim)


@pytest.mark.parametrize('wire_dtype', [None, torch.float32, torch.bfloat16])
@pytest.mark.parametrize('gdtype', GDTYPES)
def test_update_matches_cpu_chain_on_device_step_sizes(gdtype, wire_dtype):
    segs, total = _layout()
    w0, g, m0 = _draw('random')
    gd = g.to(gdtype)
    scale = 1.0 / 7
    w = w0.cuda()
    opt = _opt(w)
    opt.m.copy_(m0)
    wire = (torch.zeros(total, dtype=wire_dtype, device='cuda')
            if wire_dtype is not None else None)
    opt.step(gd.cuda(), grad_scale=scale, wire_out=wire)
    # the CPU chain (fmaf through float64) on the device's own step sizes
    ref_w, ref_m = w0.clone(), m0.clone()
    lay = F.LarsLayout(segs, total)
    lay.local_lr.copy_(opt.layout.local_lr)
    lay.wd_seg.copy_(opt.layout.wd_seg)
    F.lars_step(lay, ref_w, gd, ref_m, MU, scale)
    dm = (opt.m.cpu() - ref_m).abs()
    dw = (w.cpu() - ref_w).abs()
    eps = 2.0 ** -23
    print(f"max dm/|m|={float((dm / ref_m.abs().clamp_min(1e-30)).max()):.3e}"
          f" max dw/(|w|+|m|)="
          f"{float((dw / (ref_w.abs() + ref_m.abs()).clamp_min(1e-30)).max()):.3e}")
    assert (dm <= eps * ref_m.abs()).all()
    assert (dw <= eps * (ref_w.abs() + ref_m.abs())).all()
    assert not torch.equal(w.cpu(), w0)
    if wire is not None:
        assert torch.equal(wire, w.to(wire_dtype))


def test_gap_weights_do_not_change_any_norm():
    segs, total = _layout()
    w, g, _ = _draw('random')
    own = own_mask(segs, total)
    clean = w * own
    planted = clean.clone()
    planted[~own] = 3.0e4
    gd = g.cuda()
    a, b = _opt(clean.cuda()), _opt(planted.cuda())
    _norms(a, gd, 0.5)
    _norms(b, gd, 0.5)
    assert (~own).sum() > 0
    assert np.array_equal(f64_bits(a.layout.seg_sums),
                          f64_bits(b.layout.seg_sums))
    assert np.array_equal(f32_bits(a.layout.local_lr),
                          f32_bits(b.layout.local_lr))


@pytest.mark.parametrize('gdtype', GDTYPES)
def test_region_steps_equal_whole_buffer_step_and_runs_repeat(gdtype):
    segs, total = _layout()
    w0, g, m0 = _draw('random')
    gd = g.to(gdtype).cuda()
    runs = []
    for mode in ('whole', 'whole', 'regions'):
        w = w0.cuda()
        opt = _opt(w, 'step', decay_steps=1, gamma=0.5)
        opt.m.copy_(m0)
        wire = torch.zeros(total, dtype=torch.bfloat16, device='cuda')
        for _ in range(2):
            if mode == 'whole':
                opt.step(gd, grad_scale=0.25, wire_out=wire)
            else:
                for i, region in enumerate(synthetic_buckets(segs, total)):
                    opt.step(gd, grad_scale=0.25, wire_out=wire,
                             region=region, advance=(i == 0))
        assert int(opt.step_ctr) == 2
        runs.append((f32_bits(w), f32_bits(opt.m), wire.cpu()))
    for other in runs[1:]:
        assert np.array_equal(runs[0][0], other[0])
        assert np.array_equal(runs[0][1], other[1])
        assert torch.equal(runs[0][2], other[2])


def test_three_steps_follow_the_schedule():
    """A step schedule whose LR changes at step 2: every step must equal a
    constant-schedule step at lr_at(step) from the same state."""
    w0, g, m0 = _draw('random')
    gd = g.cuda()
    w = w0.cuda()
    opt = _opt(w, 'step', decay_steps=2, gamma=0.5)
    sched = opt.schedule
    assert [sched.lr_at(i) for i in range(3)] == [0.5, 0.5, 0.25]
    ref_w, ref_m = w0.cuda(), torch.zeros_like(w)
    for step in range(3):
        opt.step(gd, grad_scale=0.5)
        one = _opt(ref_w, 'constant', lr=sched.lr_at(step))
        one.m.copy_(ref_m)
        one.step(gd, grad_scale=0.5)
        ref_m = one.m
        assert np.array_equal(f32_bits(w), f32_bits(ref_w)), step
        assert np.array_equal(f32_bits(opt.m), f32_bits(ref_m)), step
    assert opt.lr == 0.25 and int(opt.step_ctr) == 3


# ---- the trainer: graph capture ----

def _trainer(**kw):
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='LeNet', dataset='MNIST', batch_size=32,
                    momentum=0.9, enable_gpu=True, seed=3, max_steps=12, **kw)
    tr = NNTrainer(cfg, device=torch.device('cuda', 0))
    tr.build_model()
    torch.manual_seed(17)
    x = torch.randn(32, 1, 28, 28, device='cuda', dtype=tr.compute_dtype)
    y = torch.randint(0, 10, (32,), device='cuda')
    return tr, x, y


def test_graph_replay_follows_the_schedule_bitwise():
    kw = dict(optimizer='lars', lr=0.5, lars_eta=0.02, weight_decay=1e-4,
              lr_schedule='poly', warmup_steps=2)
    tr_e, x, y = _trainer(**kw)
    for _ in range(8):                  # 3 warmup-equivalent + 5
        tr_e.train_step(x, y)
    tr_g, x2, y2 = _trainer(**kw)
    assert tr_g.enable_graph(x2, y2), "hipGraph capture failed"
    for _ in range(5):
        tr_g.graph_step(x2, y2)
    torch.cuda.synchronize()
    assert int(tr_g.optimizer.step_ctr) == int(tr_e.optimizer.step_ctr) == 8
    assert tr_g.optimizer.lr == tr_e.optimizer.lr \
        == tr_e.optimizer.schedule.lr_at(7)
    assert torch.isfinite(tr_e.master_w).all()
    assert np.array_equal(f32_bits(tr_g.master_w), f32_bits(tr_e.master_w))
    assert np.array_equal(f32_bits(tr_g.optimizer.m),
                          f32_bits(tr_e.optimizer.m))


def test_graph_refused_for_sgd_with_a_schedule():
    tr, x, y = _trainer(lr=0.05, lr_schedule='cosine')
    with pytest.warns(UserWarning, match='cannot be captured'):
        assert tr.enable_graph(x, y) is False
    tr.train_step(x, y)                 # the eager path follows the schedule
    assert tr.optimizer.lr == LRSchedule(0.05, 'cosine',
                                         total_steps=12).lr_at(0)
    tr, x, y = _trainer(lr=0.05)        # the constant default still captures
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        assert tr.enable_graph(x, y) is True
    assert not [w for w in seen if 'captured' in str(w.message)]
    w0 = tr.master_w.clone()
    tr.graph_step(x, y)
    torch.cuda.synchronize()
    assert not torch.equal(w0, tr.master_w)


# ---- the fused fan-in glue ----

@pytest.mark.parametrize('codec_name', ['raw', 'q8', 'topk'])
def test_fused_apply_lars(codec_name):
    from test_fanin_gpu import (_fill_stages, _oracle_sum, _transport,
                                _worker_sets)
    fs, t = _transport(codec_name)
    cpu = _fill_stages(fs, t, codec_name)
    sets = _worker_sets(fs)
    gsum = _oracle_sum(fs, cpu, codec_name, sets).cuda()
    master = fs.flat_w.detach().float().clone()
    ref_w = master.clone()

    def make(w):
        return FlatLARS(w, fs.segments(),
                        LRSchedule(LR, 'step', total_steps=4, decay_steps=1,
                                   gamma=0.5),
                        momentum=MU, weight_decay=WD, eta=ETA, eps=EPS)
    opt, ref = make(master), make(ref_w)
    ref_wire = torch.zeros_like(t.wire_w)
    for step in range(2):               # second step: momentum, the next LR
        t.acc_g.fill_(float('nan'))     # no zero pass is relied on
        for i, (b, ws) in enumerate(zip(fs.buckets, sets)):
            t.fused_apply(b, ws, opt, wire_out=t.wire_w, advance=(i == 0))
            ref.step(gsum, grad_scale=1.0 / len(ws) if ws else 1.0,
                     wire_out=ref_wire, region=(b.start, b.end),
                     advance=(i == 0))
        assert int(opt.step_ctr) == step + 1
        assert np.array_equal(f32_bits(t.acc_g), f32_bits(gsum))
        assert np.array_equal(f32_bits(master), f32_bits(ref_w))
        assert np.array_equal(f32_bits(opt.m), f32_bits(ref.m))
        assert torch.equal(t.wire_w, ref_wire)
    assert not torch.equal(master, fs.flat_w.detach().float())
