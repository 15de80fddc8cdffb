"""Fan-in kernels (ops/kernels/fanin.hip) against the CPU oracle of
ops.functional, bit for bit: the rank-ordered sum for every codec, the fused
SGD update against ps_fused_sgd on the materialised sum, interior slices
with canaries, rejected arguments, the PSTransport.fused_apply glue and
graph capture."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from ps_pytorch_amd.ops import functional as F

from fanin_utils import (CODECS, CODEC_IDS, bits, make_sources, order_triple,
                         topk_edge_payload, zero_payload)

pytestmark = pytest.mark.gpu

WS = (0, 1, 3, 7, 16)
# quad and block tails, more than one workgroup, one size past the
# 2048-workgroup launch cap (grid-stride loop)
BIG = (1 << 21) + 264
NS = (4, 8, 248, 252, 256, 260, 4104, BIG)
CANARY = 0xAB
BY_NAME = {c[0]: c[1:] for c in CODECS}


@functools.lru_cache(maxsize=None)
def _pool(name: str, n: int):
    """16 CPU sources of one codec and size, built once with the CPU
    packers and shared by the tests below."""
    codec, k, dtype = BY_NAME[name]
    return tuple(make_sources(codec, k, dtype, 16, n, seed=11))


@functools.lru_cache(maxsize=None)
def _oracle(name: str, n: int, W: int) -> torch.Tensor:
    codec, k, _ = BY_NAME[name]
    dst = torch.empty(n)
    F.fanin_reduce(dst, _pool(name, n)[:W], codec, k)
    return dst


def _check_reduce(srcs, codec, k, n, what):
    ref = torch.empty(n)
    F.fanin_reduce(ref, srcs, codec, k)
    dst = torch.full((n,), float('nan'), device='cuda')
    F.fanin_reduce(dst, [s.cuda() for s in srcs], codec, k)
    assert np.array_equal(bits(dst), bits(ref)), what


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('name', CODEC_IDS)
def test_reduce_bitwise_matches_cpu(name, n):
    codec, k, dtype = BY_NAME[name]
    dev = [s.cuda() for s in _pool(name, n)]
    for W in WS:
        dst = torch.full((n,), float('nan'), device='cuda')
        F.fanin_reduce(dst, dev[:W], codec, k)
        assert np.array_equal(bits(dst), bits(_oracle(name, n, W))), W
    if n == BIG:
        return
    pool = _pool(name, n)
    z = zero_payload(codec, k, dtype, n)
    _check_reduce([z, pool[0], z, pool[1]], codec, k, n, 'zero payloads')
    _check_reduce([z, z], codec, k, n, 'only zero payloads')
    tri = order_triple(codec, k, dtype, n)
    for perm in itertools.permutations(range(3)):
        _check_reduce([tri[i] for i in perm], codec, k, n, perm)
    if codec == 'topk':
        edge = [topk_edge_payload(n, k, seed=100 + j) for j in range(5)]
        _check_reduce(edge, codec, k, n, 'repeated / out-of-range indices')


def test_order_changes_bits_on_device():
    n = 260
    tri = [s.cuda() for s in order_triple('raw', None, torch.float32, n)]
    a = torch.empty(n, device='cuda')
    b = torch.empty(n, device='cuda')
    F.fanin_reduce(a, [tri[0], tri[1], tri[2]], 'raw')
    F.fanin_reduce(b, [tri[0], tri[2], tri[1]], 'raw')
    assert (a == 1).all() and (b == 0).all()


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('name', CODEC_IDS)
def test_sgd_bitwise_matches_fused_sgd_on_oracle_sum(name, n):
    codec, k, _ = BY_NAME[name]
    g0 = torch.Generator().manual_seed(n)
    w0 = torch.randn(n, generator=g0).cuda()
    m0 = (torch.randn(n, generator=g0) * 0.1).cuda()
    for W in (1, 7):
        srcs = [s.cuda() for s in _pool(name, n)[:W]]
        gsum = _oracle(name, n, W).cuda()
        for nesterov, wd, wire_dt in itertools.product(
                (False, True), (0.0, 5e-4),
                (None, torch.float32, torch.bfloat16)):
            w1, m1, w2, m2 = w0.clone(), m0.clone(), w0.clone(), m0.clone()
            wire1 = wire2 = None
            if wire_dt is not None:
                wire1 = torch.zeros(n, dtype=wire_dt, device='cuda')
                wire2 = torch.zeros(n, dtype=wire_dt, device='cuda')
            F.fanin_sgd(w1, m1, srcs, codec, k, 0.1, 0.9, wd, 1.0 / W,
                        nesterov, wire1)
            F.fused_sgd_step(w2, gsum, m2, 0.1, 0.9, wd, 1.0 / W, nesterov,
                             wire2)
            what = (W, nesterov, wd, wire_dt)
            assert np.array_equal(bits(w1), bits(w2)), what
            assert np.array_equal(bits(m1), bits(m2)), what
            if wire_dt is not None:
                assert torch.equal(wire1, wire2), what
        assert not torch.equal(w1, w0)


def _guarded(n: int, dtype, off_elems: int = 8):
    """An n-element slice at an 8-element offset inside a canary buffer."""
    esz = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full(((n + 2 * off_elems) * esz,), CANARY, dtype=torch.uint8,
                     device='cuda')
    buf = raw.view(dtype)
    return raw, buf[off_elems:off_elems + n]


def _canaries_intact(raw: torch.Tensor, n: int, dtype, off_elems: int = 8):
    esz = torch.empty(0, dtype=dtype).element_size()
    lo, hi = off_elems * esz, (off_elems + n) * esz
    return bool((raw[:lo] == CANARY).all() and (raw[hi:] == CANARY).all())


@pytest.mark.parametrize('n', (248, 260, 4104))
@pytest.mark.parametrize('name', CODEC_IDS)
def test_slice_safety(name, n):
    """Outputs on interior slices at an 8-element offset, compressed
    payloads at a byte offset that is 4-B but not 16-B aligned inside one
    stage buffer per worker: nothing outside the slices changes and the
    stage buffers stay as they were."""
    codec, k, dtype = BY_NAME[name]
    W = 3
    pool = _pool(name, n)[:W]
    stages, srcs = [], []
    for p in pool:
        # raw sources are read as whole quads: an 8-element offset; payload
        # bytes: offset 20
        off = 8 if codec == 'raw' else 20
        st = torch.full(((p.numel() + 2 * off) * p.element_size(),), CANARY,
                        dtype=torch.uint8, device='cuda').view(p.dtype)
        sl = st[off:off + p.numel()]
        sl.copy_(p)
        if codec != 'raw':
            assert sl.data_ptr() % 16 == 4
        stages.append(st)
        srcs.append(sl)
    before = [st.clone() for st in stages]
    ref = _oracle(name, n, W)

    raw_d, dst = _guarded(n, torch.float32)
    F.fanin_reduce(dst, srcs, codec, k)
    assert np.array_equal(bits(dst), bits(ref))
    assert _canaries_intact(raw_d, n, torch.float32)

    g0 = torch.Generator().manual_seed(n + 1)
    w0 = torch.randn(n, generator=g0).cuda()
    m0 = torch.randn(n, generator=g0).cuda()
    for wire_dt in (torch.float32, torch.bfloat16):
        raw_w, w = _guarded(n, torch.float32)
        raw_m, m = _guarded(n, torch.float32)
        raw_x, wire = _guarded(n, wire_dt)
        w.copy_(w0)
        m.copy_(m0)
        F.fanin_sgd(w, m, srcs, codec, k, 0.05, 0.9, 1e-4, 1.0 / W, True,
                    wire)
        w2, m2 = w0.clone(), m0.clone()
        wire2 = torch.zeros(n, dtype=wire_dt, device='cuda')
        F.fused_sgd_step(w2, ref.cuda(), m2, 0.05, 0.9, 1e-4, 1.0 / W, True,
                         wire2)
        assert np.array_equal(bits(w), bits(w2))
        assert np.array_equal(bits(m), bits(m2))
        assert torch.equal(wire, wire2)
        assert _canaries_intact(raw_w, n, torch.float32)
        assert _canaries_intact(raw_m, n, torch.float32)
        assert _canaries_intact(raw_x, n, wire_dt)
    for st, b in zip(stages, before):
        assert torch.equal(st.view(torch.uint8), b.view(torch.uint8))


def test_rejected_arguments_leave_outputs_untouched():
    from ps_pytorch_amd.ops import current_stream_ptr, require_lib
    lib = require_lib()
    n = 256
    src = torch.zeros(n, device='cuda')
    q8 = torch.zeros(F.q8_layout(n)[1], dtype=torch.uint8, device='cuda')
    tk = torch.zeros(F.topk_layout(n, 4)[1], dtype=torch.uint8, device='cuda')
    outs = [torch.full((n,), 7.0, device='cuda') for _ in range(3)]
    dst, w, m = outs
    wire = torch.full((n,), 7.0, device='cuda')
    # the wrappers raise before anything is launched
    with pytest.raises(ValueError):
        F.fanin_reduce(dst, [src] * 17, 'raw')
    with pytest.raises(ValueError):
        F.fanin_sgd(w, m, [src] * 17, 'raw', None, 0.1, wire_out=wire)
    with pytest.raises(ValueError):
        F.fanin_reduce(dst, [tk], 'topk', 5)
    with pytest.raises(ValueError):
        F.fanin_sgd(w, m, [tk], 'topk', 12, 0.1, wire_out=wire)
    with pytest.raises(ValueError):
        F.fanin_reduce(dst, [q8], 'zip')
    with pytest.raises(ValueError):
        F.fanin_sgd(w, m, [q8], 'zip', None, 0.1, wire_out=wire)
    with pytest.raises(ValueError):
        F.fanin_reduce(dst[:254], [src[:254]], 'raw')      # n % 4
    # and so do the native entry points: nonzero, nothing launched
    p17 = (ctypes.c_void_p * 17)(*([src.data_ptr()] * 17))
    p1 = (ctypes.c_void_p * 16)(tk.data_ptr())
    s = current_stream_ptr()
    for nsrc, codec, k, ptrs in ((17, 0, 0, p17), (1, 3, 5, p1),
                                 (1, 9, 0, p1), (-1, 0, 0, p1)):
        assert lib.ps_fanin_reduce(dst.data_ptr(), ptrs, nsrc, codec, k, n,
                                   s) != 0
        assert lib.ps_fanin_sgd(w.data_ptr(), m.data_ptr(), wire.data_ptr(),
                                0, ptrs, nsrc, codec, k, n, 0.1, 0.9, 0.0,
                                1.0, 0, s) != 0
    torch.cuda.synchronize()
    for t in outs + [wire]:
        assert (t == 7.0).all()


# ---- PSTransport.fused_apply on the device, no process group ----

def _transport(codec_name: str):
    from ps_pytorch_amd.models import build_model
    from ps_pytorch_amd.parallel.flat import FlatSpace
    from ps_pytorch_amd.parallel.transport import PSTransport
    torch.manual_seed(3)
    net = build_model('LeNet', num_classes=10, in_channels=1).cuda()
    fs = FlatSpace(net, bucket_bytes=16384)     # four buckets on LeNet
    assert len(fs.buckets) >= 4
    dev = torch.device('cuda')
    if codec_name == 'raw':
        t = PSTransport(fs, torch.bfloat16, dev, rank=0, world=4,
                        mode='gather', compress=False)
    else:
        t = PSTransport(fs, torch.bfloat16, dev, rank=0, world=4,
                        mode='gather', compress=True, codec=codec_name,
                        topk_k=8)
    return fs, t


def _fill_stages(fs, t, codec_name: str):
    """Hand-made stages: per worker and bucket a payload built on the CPU.
    Returns {(worker, bucket index): cpu payload}."""
    cpu = {}
    g = torch.Generator().manual_seed(17)
    for w in (1, 2, 3):
        for b in fs.buckets:
            x = torch.randn(b.numel, generator=g) * 0.01 * w
            if codec_name == 'raw':
                p = x.to(torch.bfloat16)
            elif codec_name == 'q8':
                p = torch.zeros(F.q8_layout(b.numel)[1], dtype=torch.uint8)
                F.pack_q8(p, x)
            else:
                p = torch.zeros(F.topk_layout(b.numel, 8)[1],
                                dtype=torch.uint8)
                F.pack_topk_ef(p, x, torch.zeros(b.numel), 8)
            t._stage_slice(w, b).copy_(p)
            cpu[(w, b.index)] = p
    return cpu


def _worker_sets(fs):
    """Per bucket: everyone, a pair, nobody, then everyone again."""
    sets = [[1, 2, 3], [1, 3], []]
    return [sets[b.index] if b.index < 3 else [1, 2, 3] for b in fs.buckets]


def _oracle_sum(fs, cpu, codec_name: str, sets) -> torch.Tensor:
    g = torch.zeros(fs.padded)
    k = 8 if codec_name == 'topk' else None
    for b, ws in zip(fs.buckets, sets):
        F.fanin_reduce(g[b.start:b.end], [cpu[(w, b.index)] for w in ws],
                       codec_name, k)
    return g


@pytest.mark.parametrize('codec_name', ['raw', 'q8', 'topk'])
def test_fused_apply_sgd(codec_name):
    from ps_pytorch_amd.optim import FlatSGD
    fs, t = _transport(codec_name)
    cpu = _fill_stages(fs, t, codec_name)
    sets = _worker_sets(fs)
    gsum = _oracle_sum(fs, cpu, codec_name, sets).cuda()
    master = fs.flat_w.detach().float().clone()
    ref_w = master.clone()
    opt = FlatSGD(master, lr=0.1, momentum=0.9, nesterov=True)
    ref = FlatSGD(ref_w, lr=0.1, momentum=0.9, nesterov=True)
    ref_wire = torch.zeros_like(t.wire_w)
    for step in range(2):       # second step: momentum is live
        for b, ws in zip(fs.buckets, sets):
            t.fused_apply(b, ws, opt, wire_out=t.wire_w)
            ref.step(gsum, grad_scale=1.0 / len(ws) if ws else 1.0,
                     wire_out=ref_wire, region=(b.start, b.end))
        assert np.array_equal(bits(master), bits(ref_w)), step
        assert np.array_equal(bits(opt.m), bits(ref.m)), step
        assert torch.equal(t.wire_w, ref_wire), step
    # the bucket nobody counted for saw a zero gradient: after step 1 its
    # momentum is 0 and its weights are where they started
    b = fs.buckets[2]
    assert not gsum[b.start:b.end].any()
    assert torch.equal(master[b.start:b.end],
                       fs.flat_w.detach().float()[b.start:b.end])


@pytest.mark.parametrize('codec_name', ['raw', 'q8', 'topk'])
def test_fused_apply_adam(codec_name):
    from ps_pytorch_amd.optim import FlatAdam
    fs, t = _transport(codec_name)
    cpu = _fill_stages(fs, t, codec_name)
    sets = _worker_sets(fs)
    gsum = _oracle_sum(fs, cpu, codec_name, sets).cuda()
    master = fs.flat_w.detach().float().clone()
    ref_w = master.clone()
    opt, ref = FlatAdam(master, lr=1e-3), FlatAdam(ref_w, lr=1e-3)
    ref_wire = torch.zeros_like(t.wire_w)
    t.acc_g.fill_(float('nan'))          # no zero pass is relied on
    for i, (b, ws) in enumerate(zip(fs.buckets, sets)):
        t.fused_apply(b, ws, opt, wire_out=t.wire_w, advance=(i == 0))
        ref.step(gsum, grad_scale=1.0 / len(ws) if ws else 1.0,
                 wire_out=ref_wire, region=(b.start, b.end),
                 advance=(i == 0))
    assert opt.t == 1
    assert np.array_equal(bits(t.acc_g), bits(gsum))
    assert not t.acc_g[fs.buckets[2].start:fs.buckets[2].end].any()
    assert np.array_equal(bits(master), bits(ref_w))
    assert np.array_equal(bits(opt.exp_avg_sq), bits(ref.exp_avg_sq))
    assert torch.equal(t.wire_w, ref_wire)


def test_graph_capture_replays_eager_result():
    name, n, W = 'q8', 4104, 7
    codec, k, _ = BY_NAME[name]
    srcs = [s.cuda() for s in _pool(name, n)[:W]]
    g0 = torch.Generator().manual_seed(9)
    w0 = torch.randn(n, generator=g0).cuda()
    m0 = torch.randn(n, generator=g0).cuda()
    we, me = w0.clone(), m0.clone()
    wire_e = torch.zeros(n, dtype=torch.bfloat16, device='cuda')
    F.fanin_sgd(we, me, srcs, codec, k, 0.1, 0.9, 5e-4, 1.0 / W, True, wire_e)

    w, m = w0.clone(), m0.clone()
    wire = torch.zeros(n, dtype=torch.bfloat16, device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):     # one kernel node: a single branch
        F.fanin_sgd(w, m, srcs, codec, k, 0.1, 0.9, 5e-4, 1.0 / W, True, wire)
    w.copy_(w0)
    m.copy_(m0)
    wire.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(w), bits(we))
    assert np.array_equal(bits(m), bits(me))
    assert torch.equal(wire, wire_e)
