"""Fused loss + prec@k kernels (ops/kernels/metrics.hip) against the CPU
oracle functional.ce_topk_reference: exact counts, loss tied bitwise to the
training kernel and checked independently against float64, the training
entry, graph capture, and the captured trainer step."""
import pytest
import torch
import torch.nn.functional as F

from ps_pytorch_amd.ops.functional import ce_topk_reference
from ps_pytorch_amd.ops.loss import cross_entropy
from ps_pytorch_amd.ops.metrics import MetricAccumulator, ce_topk

pytestmark = pytest.mark.gpu

REG_LIMIT = 2048      # rows up to this many classes are held in registers
SHAPES = [(1, 1), (3, 2), (5, 10), (64, 16), (7, 100), (33, 257), (6, 520),
          (33, 1000), (1029, 10), (5, REG_LIMIT + 6)]
DTYPES = [torch.bfloat16, torch.float32]
KS = [(1, 5), (1, 2, 3, 10)]
NAN = float('nan')


def _lattice(M, C, seed):
    """Logits on a 16-value integer lattice (exact in bf16): most rows have
    ties at the target."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(0, 16, (M, C), generator=g) - 8).float()
    t = torch.randint(0, C, (M,), generator=g)
    return x, t


def _randn(M, C, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * scale
    t = torch.randint(0, C, (M,), generator=g)
    return x, t


def _assert_counts(xd, td, ks):
    """Kernel counts == oracle counts on the same logit values."""
    loss_sum, hits, rows, invalid = ce_topk(xd, td, ks)
    _, r_hits, r_rows, r_inv = ce_topk_reference(xd.cpu(), td.cpu(), ks)
    got = (hits.tolist(), int(rows), int(invalid))
    want = (r_hits.tolist(), int(r_rows), int(r_inv))
    assert got == want, (got, want)
    return float(loss_sum)


@pytest.mark.parametrize("ks", KS)
@pytest.mark.parametrize("MC", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_counts_equal_oracle(dtype, MC, ks):
    M, C = MC
    x, t = _lattice(M, C, seed=M * 131 + C)
    _assert_counts(x.to('cuda', dtype), t.cuda(), ks)


@pytest.mark.parametrize("C", [16, 10])
@pytest.mark.parametrize("dtype", DTYPES)
def test_counts_on_misaligned_view(dtype, C):
    """Base pointer one element past the allocation: 2-byte aligned for bf16,
    4-byte aligned for f32, for an aligned (16) and a ragged (10) row."""
    M = 37
    x, t = _lattice(M, C, seed=C)
    buf = torch.zeros(M * C + 9, dtype=dtype, device='cuda')
    view = buf[1:1 + M * C].view(M, C)
    view.copy_(x)
    assert view.data_ptr() % 16 == buf.element_size() and view.is_contiguous()
    _assert_counts(view, t.cuda(), (1, 5))
    xr, tr_ = _randn(M, C, seed=C + 1)
    view.copy_(xr)
    ls = _assert_counts(view, tr_.cuda(), (1, 5))
    ref = F.cross_entropy(view.cpu().double(), tr_, reduction='sum')
    assert abs(ls - float(ref)) / M < 2e-3 * max(1.0, abs(float(ref)) / M)


@pytest.mark.parametrize("dtype", DTYPES)
def test_invalid_and_nan_rows_in_a_batch(dtype):
    M, C = 41, 10
    x, t = _lattice(M, C, seed=77)
    t[3], t[17], t[40] = -1, C, 2 ** 40      # never used as an index
    x[5, (int(t[5]) + 1) % C] = NAN          # NaN beside the target
    x[9, int(t[9])] = NAN                    # NaN at the target
    x[11, :] = NAN
    x[3, 0] = NAN                            # NaN in an invalid row
    xd, td = x.to('cuda', dtype), t.cuda()
    _assert_counts(xd, td, (1, 5))
    acc = MetricAccumulator('cuda', ks=(1, 5))
    acc.update(xd, td)
    res = acc.result()
    torch.cuda.synchronize()
    assert (res.rows, res.invalid) == (M - 3, 3)
    # without the NaN rows the loss is finite and excludes the invalid rows
    x2, _ = _lattice(M, C, seed=77)
    keep = torch.tensor([i for i in range(M) if i not in (3, 17, 40)])
    ls = float(ce_topk(x2.to('cuda', dtype), td, (1,))[0])
    ref = F.cross_entropy(x2[keep].double(), t[keep], reduction='sum')
    assert abs(ls - float(ref)) < 2e-3 * abs(float(ref))


LOSS_SHAPES = [(7, 100), (33, 1000), (1029, 10), (6, 520), (5, REG_LIMIT + 6)]


@pytest.mark.parametrize("MC", LOSS_SHAPES)
def test_loss_bitwise_tie_to_training_kernel_bf16(MC):
    M, C = MC
    x, t = _randn(M, C, seed=M + C)
    xd, td = x.to('cuda', torch.bfloat16), t.cuda()
    loss_sum = ce_topk(xd, td)[0].cpu()
    assert loss_sum.dtype == torch.float64
    mean = loss_sum.float() / torch.tensor(float(M), dtype=torch.float32)
    assert float(loss_sum.float()) == float(loss_sum)    # an f32 value
    assert torch.equal(mean, cross_entropy(xd, td).cpu())
    # independent: float64 reference on the same bf16 values
    ref = float(F.cross_entropy(xd.cpu().double(), t, reduction='sum')) / M
    err = abs(float(loss_sum) / M - ref)
    print(f"M={M} C={C}: bf16 mean-loss err vs float64 {err:.3e}")
    assert err < 2e-3 * max(1.0, abs(ref))


@pytest.mark.parametrize("MC", LOSS_SHAPES)
def test_loss_bitwise_tie_to_training_kernel_f32(MC):
    M, C = MC
    x, t = _randn(M, C, seed=M + C)
    xd, td = x.cuda(), t.cuda()
    loss_sum = ce_topk(xd, td)[0].cpu()
    mean = (loss_sum / M).float()
    assert torch.equal(mean, cross_entropy(xd, td).cpu())


def _ce_inputs(M, C, big):
    g = torch.Generator().manual_seed(M * 3 + C)
    x = torch.randn(M, C, generator=g)
    if big:   # logits near +-80: exp overflows f32 without max-subtraction
        x[:, 0::2] += 80.0
        x[:, 1::2] -= 80.0
    t = torch.randint(0, C, (M,), generator=g)
    return x, t


@pytest.mark.parametrize("M,C,big", [(7, 10, False), (1024, 10, False),
                                     (33, 1000, False), (4, 3, False),
                                     (33, 1000, True), (7, 10, True)])
def test_loss_f32_vs_float64(M, C, big):
    """The yardstick of test_softmax_ce_f32_vs_float64: the error against
    float64 may be at most 4x that of torch's own fp32 GPU F.cross_entropy
    (sum reduction) on the same input."""
    x, t = _ce_inputs(M, C, big)
    ref = float(F.cross_entropy(x.double(), t, reduction='sum'))
    lt = float(F.cross_entropy(x.cuda(), t.cuda(), reduction='sum')
               .double().cpu())
    lk = float(ce_topk(x.cuda(), t.cuda())[0])
    e_k, e_t = abs(lk - ref), abs(lt - ref)
    msg = f"M={M} C={C} big={big}: loss-sum err kernel {e_k:.3e} torch {e_t:.3e}"
    print(msg)
    assert e_k <= 4 * e_t, msg


@pytest.mark.parametrize("MC", [(64, 10), (33, 1000), (1029, 10),
                                (5, REG_LIMIT + 6)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_training_entry_bitwise_and_counts(dtype, MC):
    M, C = MC
    x, t = _randn(M, C, seed=M * 7 + C)
    td = t.cuda()
    xa = x.to('cuda', dtype).requires_grad_(True)
    xb = x.to('cuda', dtype).requires_grad_(True)
    acc = MetricAccumulator('cuda', ks=(1, 5))
    la = cross_entropy(xa, td, metrics=acc)
    lb = cross_entropy(xb, td)
    la.backward()
    lb.backward()
    assert torch.equal(la.detach(), lb.detach())
    assert torch.equal(xa.grad, xb.grad)
    res = acc.result()
    r_loss, r_hits, r_rows, _ = ce_topk_reference(xa.detach().cpu(), t, (1, 5))
    assert (res.rows, res.invalid) == (M, 0)
    assert [res.prec[1], res.prec[5]] == [100.0 * h / M
                                          for h in r_hits.tolist()]
    assert abs(res.loss - float(r_loss) / M) < 2e-3 * max(
        1.0, abs(float(r_loss)) / M)
    # the loss the accumulator holds is the returned loss
    lbv = float(lb.detach())
    assert abs(res.loss - lbv) <= 1e-6 * max(1.0, abs(lbv))


def _three_batches(dtype):
    out = []
    for i, (M, C) in enumerate(((64, 10), (33, 10), (7, 10))):
        x, t = _lattice(M, C, seed=900 + i)
        if i == 1:
            t[4] = C                          # an invalid row rides along
        out.append((x.to('cuda', dtype), t.cuda()))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_update_is_capturable_and_syncs_nothing(dtype):
    """Three update() calls in one captured graph (a linear chain): capture
    fails if update synchronises or allocates through HIP."""
    batches = _three_batches(dtype)
    acc = MetricAccumulator('cuda', ks=(1, 5))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for x, t in batches:
            acc.update(x, t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for x, t in batches:
            acc.update(x, t)
    acc.reset()
    graph.replay()
    graph.replay()
    res = acc.result()
    xs = torch.cat([x.cpu() for x, _ in batches] * 2)
    ts = torch.cat([t.cpu() for _, t in batches] * 2)
    r_loss, r_hits, r_rows, r_inv = ce_topk_reference(xs, ts, (1, 5))
    assert (res.rows, res.invalid) == (int(r_rows), int(r_inv)) == (206, 2)
    assert [res.prec[1], res.prec[5]] == [100.0 * h / 206
                                          for h in r_hits.tolist()]
    assert abs(res.loss - float(r_loss) / 206) < 2e-3 * max(
        1.0, float(r_loss) / 206)


@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulation_is_deterministic(dtype):
    batches = _three_batches(dtype) + [
        tuple(v.cuda() if v.dtype == torch.int64 else v.to('cuda', dtype)
              for v in _randn(1029, 10, seed=3))]
    states = []
    for _ in range(2):
        acc = MetricAccumulator('cuda', ks=(1, 2, 5))
        for x, t in batches:
            acc.update(x, t)
        states.append(acc.state.cpu())
    assert torch.equal(states[0], states[1])


def _lenet(train_metrics):
    from ps_pytorch_amd.config import JobConfig
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='LeNet', dataset='MNIST', batch_size=64, lr=0.05,
                    momentum=0.9, enable_gpu=True, seed=3,
                    train_metrics=train_metrics)
    tr = NNTrainer(cfg, device=torch.device('cuda', 0))
    tr.build_model()
    torch.manual_seed(11)
    x = torch.randn(64, 1, 28, 28, device='cuda', dtype=tr.compute_dtype)
    y = torch.randint(0, 10, (64,), device='cuda')
    return tr, x, y


def test_metrics_inside_the_captured_step():
    # eager: the 3 steps enable_graph warms up with, then the step under test
    tr_e, x, y = _lenet(True)
    for _ in range(3):
        tr_e.train_step(x, y)
    tr_e.train_metrics.reset()
    loss_e = tr_e._step_body(x.contiguous(memory_format=torch.channels_last),
                             y).clone()
    res_e = tr_e.read_train_metrics()

    tr_g, x2, y2 = _lenet(True)
    assert tr_g.enable_graph(x2, y2), "hipGraph capture failed"
    loss_g = tr_g.graph_step(x2, y2).clone()
    res_g = tr_g.read_train_metrics()
    assert torch.equal(loss_e, loss_g), (float(loss_e), float(loss_g))
    assert res_e.rows == res_g.rows == 64
    assert res_e.prec == res_g.prec
    assert abs(res_g.loss - float(loss_g)) < 1e-5 * max(1.0, float(loss_g))
    # a second replay adds a second batch; reading reset the buffer
    tr_g.graph_step(x2, y2)
    assert tr_g.read_train_metrics().rows == 64

    # flag off: the unchanged metrics=None path (ps_softmax_ce_fwd) in the
    # captured step gives the same loss bit for bit
    tr_o, x3, y3 = _lenet(False)
    assert tr_o.train_metrics is None
    assert tr_o.enable_graph(x3, y3), "hipGraph capture failed"
    loss_o = tr_o.graph_step(x3, y3).clone()
    assert torch.equal(loss_o, loss_g), (float(loss_o), float(loss_g))
