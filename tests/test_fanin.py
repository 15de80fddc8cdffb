"""Rank-ordered fan-in on the CPU paths (the bitwise oracle of fanin.hip and
the gloo path): fanin_reduce against an independent numpy-float32 left fold,
the defined add order, zero and hand-made payloads, fanin_sgd as the
composition reduce -> fused_sgd_step, and the --fan-in flag."""
import itertools
import warnings

import numpy as np
import pytest
import torch

from ps_pytorch_amd.config import JobConfig, parse_args
from ps_pytorch_amd.ops import functional as F

from fanin_utils import (CODECS, CODEC_IDS, bits, make_sources, numpy_fold,
                         order_triple, topk_edge_payload, zero_payload)

WS = (0, 1, 2, 3, 7, 16)
NS = (4, 248, 256, 260, 4104)


def _reduce(srcs, codec, k, n):
    dst = torch.full((n,), float('nan'))
    F.fanin_reduce(dst, srcs, codec, k)
    return dst


@pytest.mark.parametrize('name,codec,k,dtype', CODECS, ids=CODEC_IDS)
def test_left_fold(name, codec, k, dtype):
    for n in NS:
        pool = make_sources(codec, k, dtype, max(WS), n, seed=1)
        for W in WS:
            got = _reduce(pool[:W], codec, k, n)
            ref = numpy_fold(pool[:W], codec, k, n)
            assert np.array_equal(bits(got), bits(ref)), (name, n, W)
            if W == 0:
                # +0 everywhere, sign included
                assert not bits(got).any()


@pytest.mark.parametrize('name,codec,k,dtype', CODECS, ids=CODEC_IDS)
def test_order_is_defined(name, codec, k, dtype):
    n = 260
    srcs = order_triple(codec, k, dtype, n)
    seen = {}
    for perm in itertools.permutations(range(3)):
        ps = [srcs[i] for i in perm]
        got = _reduce(ps, codec, k, n)
        assert np.array_equal(bits(got), bits(numpy_fold(ps, codec, k, n))), \
            (name, perm)
        seen[perm] = bits(got)
    # (1e8 + -1e8) + 1 keeps the 1, (1e8 + 1) + -1e8 loses it
    assert not np.array_equal(seen[(0, 1, 2)], seen[(0, 2, 1)]), name


@pytest.mark.parametrize('name,codec,k,dtype', CODECS, ids=CODEC_IDS)
def test_zero_payloads(name, codec, k, dtype):
    """All-zero payloads (a killed worker's) add +0 wherever they sit."""
    for n in (4, 260):
        live = make_sources(codec, k, dtype, 2, n, seed=2)
        z = zero_payload(codec, k, dtype, n)
        ref = numpy_fold(live, codec, k, n)
        for srcs in ([z, live[0], live[1]], [live[0], z, live[1]],
                     [live[0], live[1], z, z]):
            got = _reduce(srcs, codec, k, n)
            assert np.array_equal(bits(got), bits(numpy_fold(srcs, codec, k, n)))
            assert np.array_equal(got.numpy(), ref)
        assert not bits(_reduce([z, z], codec, k, n)).any()


@pytest.mark.parametrize('k', F.TOPK_KS)
def test_topk_repeated_and_out_of_range(k):
    for n in (4, 248, 260, 4104):
        srcs = [topk_edge_payload(n, k, seed=10 * k + j) for j in range(3)]
        got = _reduce(srcs, 'topk', k, n)
        ref = numpy_fold(srcs, 'topk', k, n)
        assert np.array_equal(bits(got), bits(ref)), (k, n)
    # spelled out: index 2 three times, index 9 past n = 8
    p = torch.zeros(3 * k, dtype=torch.uint8)
    p[:4] = torch.tensor([2, 2, 2, 9], dtype=torch.uint8)
    p[4:k] = 7                                    # value 0 entries
    vals = torch.zeros(k, dtype=torch.bfloat16)
    vals[:4] = torch.tensor([1.0, 2.0, 4.0, 100.0]).to(torch.bfloat16)
    p[k:] = vals.view(torch.uint8)
    out = _reduce([p, p], 'topk', k, 8)
    assert out.tolist() == [0, 0, 14.0, 0, 0, 0, 0, 0]


def test_reduce_rejects_bad_arguments():
    n = 256
    dst = torch.zeros(n)
    x = [torch.zeros(n) for _ in range(17)]
    with pytest.raises(ValueError):
        F.fanin_reduce(dst, x, 'raw')                # 17 sources
    with pytest.raises(ValueError):
        F.fanin_reduce(dst, x[:2], 'snappy')         # unknown codec
    with pytest.raises(ValueError):
        F.fanin_reduce(dst, [], 'topk', 5)           # bad K
    with pytest.raises(ValueError):
        F.fanin_reduce(dst, [torch.zeros(7, dtype=torch.uint8)], 'q8')
    with pytest.raises(TypeError):
        F.fanin_reduce(dst, [x[0], x[1].to(torch.bfloat16)], 'raw')
    assert not dst.any()


@pytest.mark.parametrize('name,codec,k,dtype',
                         [CODECS[0], CODECS[2], CODECS[5]],
                         ids=['raw_f32', 'q8', 'topk16'])
def test_fanin_sgd_is_reduce_then_sgd(name, codec, k, dtype):
    n = 4104
    srcs = make_sources(codec, k, dtype, 3, n, seed=3)
    g0 = torch.Generator().manual_seed(4)
    w0, m0 = torch.randn(n, generator=g0), torch.randn(n, generator=g0) * 0.1
    for nesterov, wd, wire_dt in itertools.product(
            (False, True), (0.0, 5e-4), (None, torch.float32, torch.bfloat16)):
        w1, m1, w2, m2 = w0.clone(), m0.clone(), w0.clone(), m0.clone()
        wire1 = None if wire_dt is None else torch.zeros(n, dtype=wire_dt)
        wire2 = None if wire_dt is None else torch.zeros(n, dtype=wire_dt)
        F.fanin_sgd(w1, m1, srcs, codec, k, 0.1, 0.9, wd, 1.0 / 3, nesterov,
                    wire1)
        g = torch.empty(n)
        F.fanin_reduce(g, srcs, codec, k)
        F.fused_sgd_step(w2, g, m2, 0.1, 0.9, wd, 1.0 / 3, nesterov, wire2)
        assert np.array_equal(bits(w1), bits(w2))
        assert np.array_equal(bits(m1), bits(m2))
        assert not np.array_equal(bits(w1), bits(w0))
        if wire_dt is not None:
            assert torch.equal(wire1, wire2)
            assert torch.equal(wire1, w1.to(wire_dt))


def test_flat_sgd_step_fanin_region():
    from ps_pytorch_amd.optim import FlatSGD
    n, st, en = 1024, 256, 776
    g0 = torch.Generator().manual_seed(5)
    w = torch.randn(n, generator=g0)
    ref_w = w.clone()
    opt = FlatSGD(w, lr=0.1, momentum=0.9)
    ref = FlatSGD(ref_w, lr=0.1, momentum=0.9)
    wire, ref_wire = torch.zeros(n), torch.zeros(n)
    srcs = make_sources('q8', None, None, 3, en - st, seed=6)
    opt.step_fanin(srcs, 'q8', None, grad_scale=1.0 / 3, wire_out=wire,
                   region=(st, en))
    g = torch.zeros(n)
    F.fanin_reduce(g[st:en], srcs, 'q8')
    ref.step(g, grad_scale=1.0 / 3, wire_out=ref_wire, region=(st, en))
    assert torch.equal(w, ref_w) and torch.equal(opt.m, ref.m)
    assert torch.equal(wire, ref_wire)
    assert not wire[:st].any() and not wire[en:].any()


# ---- drain_fused bookkeeping, scripted arrivals, no process group ----

def _scripted_transport(arrivals, killed=()):
    from ps_pytorch_amd.models import build_model
    from ps_pytorch_amd.parallel.flat import FlatSpace
    from ps_pytorch_amd.parallel.transport import PSTransport
    torch.manual_seed(0)
    fs = FlatSpace(build_model('LeNet', num_classes=10, in_channels=1),
                   bucket_bytes=int(0.25 * 2 ** 20))
    assert len(fs.buckets) == 2
    t = PSTransport(fs, torch.float32, torch.device('cpu'), rank=0, world=4,
                    mode='gather')
    t._arrivals = lambda: iter(arrivals)
    if killed:
        t.track_killed = True
        t._recv_killed_flag = lambda w: w in killed
    return t


def test_drain_fused_selects_first_k_and_sorts():
    # bucket 0: 3, 1, 2 -> final at its 2nd arrival with {1, 3}; bucket 1
    # reaches quota last, when only worker 2 still has a recv in flight
    arrivals = [(0, 3), (0, 1), (1, 3), (1, 1), (0, 2), (1, 2)]
    t = _scripted_transport(arrivals)
    finals, quota = [], []
    counts = t.drain_fused(2, lambda b, ws: finals.append((b.index, ws)),
                           on_quota=quota.append)
    assert finals == [(0, [1, 3]), (1, [1, 3])]
    assert counts == [2, 2]
    assert quota == [[2]]
    # full quota: a bucket is final at its last arrival, ascending ranks
    t = _scripted_transport(arrivals)
    finals, quota = [], []
    counts = t.drain_fused(64, lambda b, ws: finals.append((b.index, ws)),
                           on_quota=quota.append)
    assert finals == [(0, [1, 2, 3]), (1, [1, 2, 3])]
    assert counts == [3, 3] and quota == [[]]


def test_drain_fused_excludes_killed_workers():
    # worker 3 flagged killed: never counted; with k = 3 the buckets stay
    # under quota and finalise at their last arrival
    arrivals = [(0, 3), (1, 3), (0, 2), (0, 1), (1, 1), (1, 2)]
    t = _scripted_transport(arrivals, killed={3})
    finals, quota = [], []
    counts = t.drain_fused(3, lambda b, ws: finals.append((b.index, ws)),
                           on_quota=quota.append)
    assert finals == [(0, [1, 2]), (1, [1, 2])]
    assert counts == [2, 2]
    assert quota == [[]]          # quota never met: the end-of-drain call
    # every worker killed: finalised with nobody
    t = _scripted_transport(arrivals, killed={1, 2, 3})
    finals = []
    t.drain_fused(3, lambda b, ws: finals.append((b.index, ws)))
    assert finals == [(0, []), (1, [])]


def test_fused_apply_scales_by_counted_workers_cpu():
    from ps_pytorch_amd.optim import FlatAdam, FlatSGD
    t = _scripted_transport([])
    fs = t.flat
    g = torch.Generator().manual_seed(8)
    for st in t.stages:
        st.copy_(torch.randn(fs.padded, generator=g) * 0.01)
    b = fs.buckets[1]
    w = torch.randn(fs.padded, generator=g)
    for make in (lambda p: FlatSGD(p, lr=0.1, momentum=0.9),
                 lambda p: FlatAdam(p, lr=1e-3)):
        got, ref = w.clone(), w.clone()
        opt, ropt = make(got), make(ref)
        wire, rwire = torch.zeros(fs.padded), torch.zeros(fs.padded)
        t.fused_apply(b, [1, 3], opt, wire_out=wire)
        gsum = torch.zeros(fs.padded)
        gsum[b.start:b.end] = (t.stages[0][b.start:b.end]
                               + t.stages[2][b.start:b.end])
        ropt.step(gsum, grad_scale=0.5, wire_out=rwire,
                  region=(b.start, b.end))
        assert torch.equal(got, ref) and torch.equal(wire, rwire)
        assert torch.equal(got[:b.start], w[:b.start])
        # nobody counted: zero gradient at scale 1, momentum still decays
        t.fused_apply(b, [], opt, wire_out=wire)
        ropt.step(torch.zeros(fs.padded), grad_scale=1.0, wire_out=rwire,
                  region=(b.start, b.end))
        assert torch.equal(got, ref)


# ---- --fan-in flag ----

def test_config_default_and_cli():
    assert JobConfig().fan_in == 'arrival'
    assert JobConfig.from_args(parse_args([])).fan_in == 'arrival'
    cfg = JobConfig.from_args(parse_args(
        ['--fan-in', 'fused', '--aggregation', 'gather']))
    assert cfg.fan_in == 'fused'


def test_config_bad_value_raises():
    with pytest.raises(ValueError):
        JobConfig(fan_in='sorted')


@pytest.mark.parametrize('kw', [dict(aggregation='collective'),
                                dict(aggregation='gather',
                                     engine='allreduce')])
def test_config_fused_falls_back_with_warning(kw):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        cfg = JobConfig(fan_in='fused', **kw)
    assert cfg.fan_in == 'arrival'
    assert any('--fan-in fused' in str(w.message) for w in rec)


def test_ps_falls_back_past_16_workers():
    """The kernel takes 16 payload pointers: a PS with more workers warns
    and runs the arrival fan-in; up to 16 the setting passes through."""
    from ps_pytorch_amd.parallel.ps import ParameterServer
    cfg = JobConfig(fan_in='fused', aggregation='gather')
    dev = torch.device('cpu')
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        assert ParameterServer(cfg, 0, 17, dev).fan_in == 'fused'
        assert not rec
        assert ParameterServer(cfg, 0, 18, dev).fan_in == 'arrival'
    assert any('--fan-in fused' in str(w.message) for w in rec)
    assert ParameterServer(JobConfig(), 0, 3, dev).fan_in == 'arrival'


def test_config_fused_gather_is_kept_without_warning():
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        cfg = JobConfig(fan_in='fused', aggregation='gather')
        # kill mode normalises to gather first, so fused survives
        cfg2 = JobConfig(fan_in='fused', aggregation='gather', mode='kill')
    assert cfg.fan_in == 'fused' and cfg2.fan_in == 'fused'
    assert not [w for w in rec if 'fan-in' in str(w.message)]
