"""Fused augmentation loader kernel (ops/kernels/augment.hip) bit for bit
against the CPU oracle: the op, its device step counter, bare hipGraph
replay, GPU-vs-CPU loader parity, and the trainer's captured loader + step
against eager stepping."""
import functools

import pytest
import torch

from augment_utils import (SEED, SHAPES, STREAM, bits, fake_dataset,
                           fake_indices, norm_consts, write_cifar10)

pytestmark = pytest.mark.gpu


def _cases():
    for C, H, W, p in SHAPES:
        for mode in ('reflect', 'constant'):
            for hflip in (True, False):
                yield C, H, W, p, (mode if p else None), hflip
        yield C, H, W, 0, None, True
        yield C, H, W, 0, None, False


CASES = sorted(set(_cases()), key=str)


@functools.lru_cache(maxsize=None)
def _gpu_dataset(C, H, W):
    x, y = fake_dataset(C, H, W)
    return x.cuda(), y.cuda()


@functools.lru_cache(maxsize=None)
def _gpu_indices(B):
    return fake_indices(B).cuda()


@functools.lru_cache(maxsize=None)
def _ref(C, H, W, p, mode, hflip, dtype, B, step):
    from ps_pytorch_amd.ops.functional import augment_draws, augment_ref
    x, y = fake_dataset(C, H, W)
    mean, inv = norm_consts(C)
    draws = (augment_draws(B, p, hflip, SEED, STREAM, step)
             if p or hflip else None)
    return augment_ref(x, y, fake_indices(B), mean, inv, p, mode, hflip,
                       draws, dtype)


def _run(C, H, W, p, mode, hflip, dtype, B, step, **kw):
    from ps_pytorch_amd.ops.augment import augment_batch
    x, y = _gpu_dataset(C, H, W)
    mean, inv = norm_consts(C)
    return augment_batch(x, y, _gpu_indices(B), mean, inv, pad=p,
                         pad_mode=mode, hflip=hflip, seed=SEED, stream=STREAM,
                         step=step, dtype=dtype, **kw)


def _same(got, got_y, want, want_y):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert got.is_contiguous(memory_format=torch.channels_last)
    # same memory order on both sides: compare NHWC raw bits
    assert torch.equal(bits(got.permute(0, 2, 3, 1)).cpu(),
                       bits(want.permute(0, 2, 3, 1)))
    assert torch.equal(got_y.cpu(), want_y)


@pytest.mark.parametrize('B', [1, 37, 130])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('C,H,W,p,mode,hflip', CASES)
def test_kernel_bitwise_vs_oracle(C, H, W, p, mode, hflip, dtype, B):
    rng = bool(p or hflip)
    step = torch.full((), 0 if rng else 7, dtype=torch.int64, device='cuda')
    for k in range(2 if rng else 1):
        got, got_y = _run(C, H, W, p, mode, hflip, dtype, B, step)
        torch.cuda.synchronize()
        _same(got, got_y, *_ref(C, H, W, p, mode, hflip, dtype, B, k))
        # advanced by an RNG call, untouched by a no-RNG call
        assert int(step) == (k + 1 if rng else 7)


def test_no_rng_call_takes_no_step():
    got, got_y = _run(1, 28, 28, 0, None, False, torch.float32, 37, None)
    torch.cuda.synchronize()
    _same(got, got_y, *_ref(1, 28, 28, 0, None, False, torch.float32, 37, 0))
    # augment=False switches the draws off whatever the dataset's recipe is
    got, got_y = _run(3, 32, 32, 4, 'reflect', True, torch.bfloat16, 37, None,
                      augment=False)
    torch.cuda.synchronize()
    _same(got, got_y, *_ref(3, 32, 32, 0, None, False, torch.bfloat16, 37, 0))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_writes_stay_inside_caller_buffers(dtype):
    C, H, W, p, B = 3, 5, 7, 4, 37
    n = B * C * H * W
    buf = torch.full((n + 256,), 77.0, dtype=dtype, device='cuda')
    ybuf = torch.full((B + 16,), -5, dtype=torch.int64, device='cuda')
    out = buf[128:128 + n].view(B, H, W, C).permute(0, 3, 1, 2)
    out_y = ybuf[8:8 + B]
    step = torch.zeros((), dtype=torch.int64, device='cuda')
    got, got_y = _run(C, H, W, p, 'reflect', True, dtype, B, step, out=out,
                      out_y=out_y)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    _same(got, got_y, *_ref(C, H, W, p, 'reflect', True, dtype, B, 0))
    assert (buf[:128] == 77).all() and (buf[128 + n:] == 77).all()
    assert (ybuf[:8] == -5).all() and (ybuf[8 + B:] == -5).all()


def test_dataset_offsets_past_2_31():
    """A resident set of more than 2^31 bytes: image offsets need 64 bits."""
    from ps_pytorch_amd.ops.augment import augment_batch
    from ps_pytorch_amd.ops.functional import augment_draws, augment_ref
    C, H, W, p = 3, 32, 32, 4
    n_big = (1 << 31) // (C * H * W) + 40
    xs, ys = fake_dataset(C, H, W)
    where = torch.tensor([n_big - 1, n_big - 7, (1 << 31) // (C * H * W) + 1,
                          3, n_big - 1])
    xb = torch.zeros((n_big, C, H, W), dtype=torch.uint8, device='cuda')
    yb = torch.zeros(n_big, dtype=torch.int64, device='cuda')
    small = torch.arange(5) % 4          # images 0..3 of the small set
    xb[where.cuda()] = xs[small].cuda()
    yb[where.cuda()] = ys[small].cuda()
    mean, inv = norm_consts(C)
    step = torch.zeros((), dtype=torch.int64, device='cuda')
    got, got_y = augment_batch(xb, yb, where.cuda(), mean, inv, pad=p,
                               pad_mode='reflect', hflip=True, seed=SEED,
                               stream=STREAM, step=step,
                               dtype=torch.bfloat16)
    torch.cuda.synchronize()
    want = augment_ref(xs, ys, small, mean, inv, p, 'reflect', True,
                       augment_draws(5, p, True, SEED, STREAM, 0),
                       torch.bfloat16)
    _same(got, got_y, *want)


def test_gpu_value_error_guards():
    from ps_pytorch_amd.ops.augment import augment_batch
    x, y = _gpu_dataset(3, 5, 7)
    mean, inv = norm_consts(3)
    idx = fake_indices(4).cuda()
    kw = dict(pad=4, pad_mode='reflect', hflip=True, seed=1)
    with pytest.raises(ValueError):          # RNG call without a counter
        augment_batch(x, y, idx, mean, inv, step=None, **kw)
    with pytest.raises(ValueError):          # counter on the wrong device
        augment_batch(x, y, idx, mean, inv,
                      step=torch.zeros((), dtype=torch.int64), **kw)
    with pytest.raises(ValueError):          # indices on the wrong device
        augment_batch(x, y, idx.cpu(), mean, inv, step=torch.zeros(
            (), dtype=torch.int64, device='cuda'), **kw)
    with pytest.raises(ValueError):          # NCHW-contiguous out buffer
        augment_batch(x, y, idx, mean, inv, augment=False,
                      out=torch.empty(4, 3, 5, 7, device='cuda'),
                      out_y=torch.empty(4, dtype=torch.int64, device='cuda'))


def test_bare_graph_replay_draws_consecutive_steps():
    C, H, W, p, B, dtype = 3, 32, 32, 4, 37, torch.bfloat16
    args = (C, H, W, p, 'reflect', True, dtype, B)
    step = torch.zeros((), dtype=torch.int64, device='cuda')
    out = torch.empty((B, C, H, W), dtype=dtype, device='cuda',
                      memory_format=torch.channels_last)
    out_y = torch.empty(B, dtype=torch.int64, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                  # steps 0, 1 outside capture
            _run(*args, step, out=out, out_y=out_y)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run(*args, step, out=out, out_y=out_y)
    torch.cuda.synchronize()
    assert int(step) == 2                   # capture does not advance it
    for k in range(2, 5):
        graph.replay()
        torch.cuda.synchronize()
        _same(out, out_y, *_ref(*args, k))
        assert int(step) == k + 1


@pytest.fixture(scope='module')
def cifar100(tmp_path_factory):
    return write_cifar10(str(tmp_path_factory.mktemp('aug') / 'cifar10_data'),
                         n_train=100)


@pytest.fixture(scope='module')
def cifar64(tmp_path_factory):
    return write_cifar10(str(tmp_path_factory.mktemp('aug') / 'cifar10_data'),
                         n_train=64)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_gpu_loader_equals_cpu_loader(cifar100, dtype):
    from ps_pytorch_amd.data import RealDataset, RealResidentLoader
    cpu = RealResidentLoader(RealDataset('Cifar10', 'train', cifar100,
                                         dtype=dtype),
                             32, seed=11, rng='philox', stream=2)
    gpu = RealResidentLoader(
        RealDataset('Cifar10', 'train', cifar100, dtype=dtype,
                    device=torch.device('cuda', 0)),
        32, seed=11, rng='philox', stream=2)
    assert len(cpu) == 3                    # 10 batches wrap three times
    for _ in range(10):
        xc, yc = cpu.next_batch()
        xg, yg = gpu.next_batch()
        _same(xg, yg, xc, yc)
    assert gpu._epoch == cpu._epoch == 3
    assert int(gpu.step) == cpu.host_step == 10


def _trainer_and_loader(root):
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.data import prepare_data
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='ResNet18', dataset='Cifar10', batch_size=16,
                    lr=0.05, momentum=0.9, enable_gpu=True, seed=3,
                    loader='fused', data_dir=root)
    tr = NNTrainer(cfg, device=torch.device('cuda', 0))
    tr.build_model()
    loader, _ = prepare_data(cfg, device=tr.device, dtype=tr.compute_dtype)
    assert loader.rng == 'philox' and len(loader) == 4
    return tr, loader


def test_graphed_loader_step_matches_eager_bitwise(cifar64):
    # eager: 8 steps, the epoch (4 batches) wraps inside
    tr_e, ld_e = _trainer_and_loader(cifar64)
    for _ in range(8):
        tr_e.train_step(*ld_e.next_batch())
    torch.cuda.synchronize()

    # graph: 3 warmup steps on real batches, then 5 data-free replays
    tr_g, ld_g = _trainer_and_loader(cifar64)
    assert tr_g.enable_graph_loader(ld_g), "hipGraph capture failed"
    loss = None
    for _ in range(5):
        loss = tr_g.graph_loader_step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert torch.isfinite(tr_e.master_w).all()
    assert tr_e.cur_step == tr_g.cur_step == 8
    assert int(ld_e.step) == int(ld_g.step) == 8
    assert ld_e._epoch == ld_g._epoch == 1
    d = (tr_e.master_w - tr_g.master_w).abs().max()
    print(f"max|dW| = {d.item():.3e}, max|W| = "
          f"{tr_e.master_w.abs().max().item():.3e}")
    assert torch.equal(tr_e.master_w.view(torch.int32),
                       tr_g.master_w.view(torch.int32))


def test_only_full_batch_philox_loaders_bind_for_capture(cifar64):
    from ps_pytorch_amd.data import RealDataset, RealResidentLoader
    ds = RealDataset('Cifar10', 'train', cifar64,
                     device=torch.device('cuda', 0))
    with pytest.raises(ValueError):
        RealResidentLoader(ds, 16, seed=3).bind_static()
    with pytest.raises(ValueError):
        RealResidentLoader(ds, 16, seed=3, rng='philox',
                           drop_last=False).bind_static()
    RealResidentLoader(ds, 16, seed=3, rng='philox').bind_static()
