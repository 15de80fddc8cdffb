"""Act-drop kernels (ops/kernels/dropout.hip) bit for bit against the Philox
CPU oracle, the device step counter, and hipGraph replay of the op and of
the reference-head VGG models."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 20240611
SALT, STREAM = 5, 3
SIZES = [1, 7, 8, 9, 515, 512 * 512, 4194304 + 13]


@functools.lru_cache(maxsize=None)
def _keep(n, p, step, seed=SEED, salt=SALT, stream=STREAM):
    from ps_pytorch_amd.ops.functional import dropout_keep_mask
    return dropout_keep_mask(n, p, seed=seed, salt=salt, stream=stream,
                             step=step)


@functools.lru_cache(maxsize=None)
def _input(n, dtype, seed):
    """CPU tensor with exact zeros (+0 and -0) and negative values."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    x[::5] = 0.0
    x[3::11] = -0.0
    return x.to(dtype)


def _run_kernel(x, p, relu, step=0):
    """Raw forward of the autograd function on a fresh counter; returns
    (y, mask bytes, counter tensor, grad_fn-carrying y)."""
    from ps_pytorch_amd.ops.dropout import _ActDropFn
    from ps_pytorch_amd.ops.functional import (dropout_salt_stream,
                                               dropout_scale,
                                               dropout_threshold)
    ctr = torch.full((), step, dtype=torch.int64, device='cuda')
    xg = x.detach().requires_grad_(True)
    y = _ActDropFn.apply(xg, relu, dropout_threshold(p), dropout_scale(p),
                         SEED, dropout_salt_stream(SALT, STREAM), ctr)
    mask = y.grad_fn.saved_tensors[0]
    return xg, y, mask, ctr


def _check(x_cpu, x_gpu, p, relu):
    from ps_pytorch_amd.ops.functional import (act_drop_bwd_ref, act_drop_ref,
                                               dropout_scale, pack_mask_bits)
    n = x_cpu.numel()
    scale = dropout_scale(p)
    y_ref, bits = act_drop_ref(x_cpu, _keep(n, p, 0), scale, relu)
    xg, y, mask, ctr = _run_kernel(x_gpu, p, relu)
    dy_cpu = _input(n, x_cpu.dtype, 99).reshape(x_cpu.shape)
    dy = dy_cpu.cuda()
    y.backward(dy)
    torch.cuda.synchronize()
    assert mask.numel() == (n + 7) // 8
    assert torch.equal(mask.cpu(), pack_mask_bits(bits))
    # compare raw bits: -0.0 == 0.0 under torch.equal
    it = torch.int16 if x_cpu.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(y.detach().cpu().view(it), y_ref.view(it))
    dx_ref = act_drop_bwd_ref(dy_cpu, bits, scale)
    assert torch.equal(xg.grad.cpu().view(it), dx_ref.view(it))
    assert int(ctr) == 1


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('p', [0.5, 0.1])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('n', SIZES)
def test_bitwise_vs_oracle(n, dtype, p, relu):
    x = _input(n, dtype, 1)
    if n == 512 * 512:
        x = x.reshape(512, 512)
    _check(x, x.cuda(), p, relu)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_misaligned_view(dtype):
    x = _input(515, dtype, 1)
    buf = torch.zeros(1024, dtype=dtype, device='cuda')
    view = buf[1:1 + 515]
    view.copy_(x)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    _check(x, view, 0.5, True)
    assert buf[0] == 0 and (buf[516:] == 0).all()


def test_p_edges_on_gpu():
    from ps_pytorch_amd.ops.dropout import PsDropout
    x = _input(1037, torch.float32, 1).cuda()
    assert torch.equal(PsDropout(p=0.0).train()(x), x)
    m = PsDropout(p=1.0).train()
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    y.backward(torch.ones_like(y))
    assert not y.any() and not xg.grad.any()
    assert m.step is None       # neither edge touches the RNG


@pytest.mark.parametrize('shape', [(2, 64, 5, 5), (2, 20, 3, 3)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_psrelu_channels_last(shape, dtype):
    from ps_pytorch_amd.ops.dropout import PsReLU
    g = torch.Generator().manual_seed(4)
    x = torch.randn(shape, generator=g).to(dtype).cuda()
    x = x.contiguous(memory_format=torch.channels_last)
    dy = torch.randn(shape, generator=g).to(dtype).cuda()
    dy = dy.contiguous(memory_format=torch.channels_last)
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    y = PsReLU()(a)
    y_ref = torch.relu(b)
    y.backward(dy)
    y_ref.backward(dy)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, y_ref)
    assert torch.equal(a.grad, b.grad)
    # a contiguous upstream gradient is re-laid-out like y first
    a.grad = None
    PsReLU()(a).backward(dy.contiguous())
    assert torch.equal(a.grad, b.grad)


def _module_mask(y):
    """keep mask of a relu=False forward of positive inputs."""
    return (y != 0).reshape(-1).cpu()


def test_device_counter_steps():
    from ps_pytorch_amd.ops.dropout import PsDropout
    torch.manual_seed(SEED)
    m = PsDropout(p=0.5, salt=SALT).train()
    m.stream = STREAM
    x = torch.ones(64, 512, device='cuda', dtype=torch.bfloat16)
    for step in range(2):
        assert torch.equal(_module_mask(m(x)), _keep(64 * 512, 0.5, step))
    assert m.step.dtype == torch.int64 and m.step.is_cuda
    assert int(m.step) == 2
    assert len(m.state_dict()) == 0 and list(m.named_buffers()) == []


def test_graph_replay_draws_consecutive_steps():
    from ps_pytorch_amd.ops.dropout import PsDropout
    torch.manual_seed(SEED)
    m = PsDropout(p=0.5, salt=SALT).train()
    m.stream = STREAM
    n = 64 * 512
    x = torch.ones(64, 512, device='cuda', dtype=torch.bfloat16,
                   requires_grad=True)
    dy = torch.ones(64, 512, device='cuda', dtype=torch.bfloat16)

    def body():
        y = m(x)
        (dx,) = torch.autograd.grad(y, x, dy)
        return y, dx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):             # steps 0..2, outside capture
            body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gy, gdx = body()
    for step in range(3, 6):
        graph.replay()
        torch.cuda.synchronize()
        keep = _keep(n, 0.5, step)
        assert torch.equal(_module_mask(gy), keep), step
        assert torch.equal(_module_mask(gdx), keep), step
    assert int(m.step) == 6


def _mk(network, seed=17):
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network=network, dataset='Cifar10', batch_size=64,
                    lr=0.05, momentum=0.9, enable_gpu=True, seed=3)
    tr = NNTrainer(cfg, device=torch.device('cuda', 0))
    tr.build_model()
    torch.manual_seed(seed)
    x = torch.randn(64, 3, 32, 32, device='cuda', dtype=tr.compute_dtype)
    y = torch.randint(0, 10, (64,), device='cuda')
    return tr, x, y


@pytest.mark.parametrize('network', ['VGG11_ref', 'VGG11_plain_ref'])
def test_model_graph_step_matches_eager(network):
    tr_e, x, y = _mk(network)
    for _ in range(8):
        tr_e.train_step(x, y)
    torch.cuda.synchronize()

    tr_g, x2, y2 = _mk(network)
    assert tr_g.enable_graph(x2, y2), "hipGraph capture failed"
    loss = None
    for _ in range(5):
        loss = tr_g.graph_step(x2, y2)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert torch.isfinite(tr_e.master_w).all()
    assert torch.isfinite(tr_g.master_w).all()
    d = (tr_e.master_w - tr_g.master_w).abs().max()
    scale = tr_e.master_w.abs().max()
    print(f"{network}: max|dW| / max|W| = {(d / scale).item():.3e}")
    assert d / scale < 1e-2, (d.item(), scale.item())
    from ps_pytorch_amd.ops.dropout import PsDropout
    for tr in (tr_e, tr_g):
        steps = [int(m.step) for m in tr.network.modules()
                 if isinstance(m, PsDropout)]
        assert steps == [8, 8]


def test_eval_forward_is_deterministic():
    tr, x, _ = _mk('VGG11_ref')
    tr.network.eval()
    with torch.no_grad():
        a = tr.network(x.contiguous(memory_format=torch.channels_last))
        b = tr.network(x.contiguous(memory_format=torch.channels_last))
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a, b)
