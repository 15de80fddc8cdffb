"""Fused loss + prec@k metrics, CPU side: the rank / invalid-row rule of
functional.ce_topk_reference (the oracle of the kernel tests), the
accumulator, the evaluation call sites and the --train-metrics flag."""
import logging
import math
import re

import pytest
import torch
import torch.nn.functional as F

from ps_pytorch_amd.config import JobConfig, parse_args
from ps_pytorch_amd.ops.functional import ce_topk_reference
from ps_pytorch_amd.ops.loss import cross_entropy
from ps_pytorch_amd.ops.metrics import MetricAccumulator, ce_topk
from ps_pytorch_amd.utils.metrics import accuracy

NAN = float('nan')


def _perm_rows(M, C, seed):
    """Every row a random permutation of C distinct values: no ties."""
    g = torch.Generator().manual_seed(seed)
    x = torch.stack([torch.randperm(C, generator=g) for _ in range(M)])
    t = torch.randint(0, C, (M,), generator=g)
    return x.float() * 0.25 - 1.0, t


def _hits(x, t, ks):
    return ce_topk_reference(x, t, ks)[1].tolist()


@pytest.mark.parametrize("C", [1, 2, 5, 10, 100])
def test_oracle_equals_accuracy_on_tie_free_logits(C):
    M = 37
    x, t = _perm_rows(M, C, seed=C)
    loss_sum, hits, rows, invalid = ce_topk_reference(x, t, (1, 5))
    p1, p5 = accuracy(x, t, topk=(1, min(5, C)))
    assert hits.tolist() == [round(float(p1) * M / 100),
                             round(float(p5) * M / 100)]
    assert int(rows) == M and int(invalid) == 0
    ref = F.cross_entropy(x.double(), t, reduction='sum')
    assert abs(float(loss_sum) - float(ref)) <= 1e-12 * max(1, abs(float(ref)))
    # the public op takes the same path on the CPU
    l2, h2, r2, i2 = ce_topk(x, t, (1, 5))
    assert float(l2) == float(loss_sum) and h2.tolist() == hits.tolist()
    assert int(r2) == M and int(i2) == 0


def test_tie_rule_all_equal_row():
    C = 6
    x = torch.full((C, C), 0.5)
    t = torch.arange(C)
    for k in (1, 2, 3, 5):
        assert _hits(x, t, (k,)) == [min(k, C)]      # hit iff t < k
        per_row = [_hits(x[i:i + 1], t[i:i + 1], (k,))[0] for i in range(C)]
        assert per_row == [int(i < k) for i in range(C)]


def test_tie_rule_target_between_equal_neighbours():
    # target (index 2) tied with a lower (0) and a higher (4) index, one
    # strictly larger value (3): rank = 1 (larger) + 1 (lower tie) = 2
    x = torch.tensor([[1.0, -2.0, 1.0, 3.0, 1.0]])
    t = torch.tensor([2])
    assert _hits(x, t, (1, 2, 3)) == [0, 0, 1]
    assert _hits(x, torch.tensor([0]), (1, 2, 3)) == [0, 1, 1]   # rank 1
    assert _hits(x, torch.tensor([4]), (1, 2, 3, 4)) == [0, 0, 0, 1]  # rank 3


def test_k_above_class_count():
    x, t = _perm_rows(9, 3, seed=4)
    assert _hits(x, t, (5,)) == [9]              # min(k, C) = C: always a hit
    assert _hits(x, t, (3,)) == [9]
    with pytest.raises(ValueError):
        ce_topk_reference(x, t, (0,))
    with pytest.raises(ValueError):
        MetricAccumulator('cpu', ks=(1, -2))
    with pytest.raises(ValueError):
        MetricAccumulator('cpu', ks=(1, 2, 3, 4, 5))


def test_nan_rules():
    x = torch.tensor([[3.0, 1.0, 2.0, 0.0]])
    t = torch.tensor([0])
    assert _hits(x, t, (1, 2)) == [1, 1]
    xn = x.clone()
    xn[0, 3] = NAN                              # non-target NaN: one rank down
    assert _hits(xn, t, (1, 2)) == [0, 1]
    xt = x.clone()
    xt[0, 0] = NAN                              # NaN at the target: never a hit
    assert _hits(xt, t, (1, 2, 4, 9)) == [0, 0, 0, 0]
    allnan = torch.full((1, 4), NAN)
    assert _hits(allnan, t, (1, 4)) == [0, 0]


def test_invalid_targets_are_counted_and_excluded():
    x, t = _perm_rows(6, 5, seed=9)
    tb = t.clone()
    tb[1], tb[4] = -1, 5
    keep = torch.tensor([0, 2, 3, 5])
    loss_sum, hits, rows, invalid = ce_topk_reference(x, tb, (1, 5))
    l_ok, h_ok, r_ok, _ = ce_topk_reference(x[keep], t[keep], (1, 5))
    assert (int(rows), int(invalid)) == (4, 2) and int(r_ok) == 4
    assert hits.tolist() == h_ok.tolist()
    assert abs(float(loss_sum) - float(l_ok)) < 1e-12

    acc = MetricAccumulator('cpu', ks=(1, 5))
    acc.update(x, tb)
    res = acc.result()
    assert (res.rows, res.invalid) == (4, 2)
    assert res.loss == pytest.approx(float(l_ok) / 4, rel=1e-12)
    assert res.prec[1] == 100.0 * int(h_ok[0]) / 4
    assert res.prec[5] == 100.0


def test_all_invalid_batch(caplog):
    x, _ = _perm_rows(3, 4, seed=2)
    acc = MetricAccumulator('cpu')
    acc.update(x, torch.tensor([-1, 4, 99]))
    with caplog.at_level(logging.WARNING):
        res = acc.result()
    assert (res.rows, res.invalid) == (0, 3)
    assert res.loss == 0.0 and res.prec == {1: 0.0, 5: 0.0}
    assert any('outside the class range' in r.getMessage()
               for r in caplog.records)


def test_accumulator_batches_equal_concatenation():
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-4, 4, (40, 7), generator=g).float()   # many ties
    t = torch.randint(0, 7, (40,), generator=g)
    t[5] = 7
    acc = MetricAccumulator('cpu', ks=(1, 2, 5))
    for lo, hi in ((0, 3), (3, 20), (20, 40)):
        acc.update(x[lo:hi], t[lo:hi])
    res = acc.result()
    loss_sum, hits, rows, invalid = ce_topk_reference(x, t, (1, 2, 5))
    assert (res.rows, res.invalid) == (int(rows), int(invalid)) == (39, 1)
    assert [res.prec[k] for k in (1, 2, 5)] == [100.0 * h / 39
                                                for h in hits.tolist()]
    assert res.loss == pytest.approx(float(loss_sum) / 39, rel=1e-14)
    acc.reset()
    assert acc.result().rows == 0


def test_cross_entropy_with_accumulator_cpu():
    x, t = _perm_rows(12, 10, seed=8)
    acc = MetricAccumulator('cpu')
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    la = cross_entropy(xa, t, metrics=acc)
    lb = cross_entropy(xb, t)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(xa.grad, xb.grad)
    res = acc.result()
    assert res.rows == 12
    assert res.loss == pytest.approx(float(lb.detach()), rel=1e-6)


# ---- call sites ----

def _expected(net, batches):
    """loss / prec@1 / prec@5 the way the loops computed them before the
    accumulator: F.cross_entropy sum + accuracy per batch."""
    tot = loss_sum = p1_sum = p5_sum = 0.0
    with torch.no_grad():
        for data, target in batches:
            out = net(data)
            loss_sum += float(F.cross_entropy(out.float(), target,
                                              reduction='sum'))
            p1, p5 = accuracy(out.float(), target, topk=(1, 5))
            p1_sum += float(p1) * len(target)
            p5_sum += float(p5) * len(target)
            tot += len(target)
    return loss_sum / tot, p1_sum / tot, p5_sum / tot


def _batches(seed=0, sizes=(50, 50, 28)):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(b, 1, 28, 28, generator=g),
             torch.randint(0, 10, (b,), generator=g)) for b in sizes]


def test_validate_prints_the_same_numbers(caplog):
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='LeNet', dataset='MNIST', batch_size=64)
    tr = NNTrainer(cfg, device=torch.device('cpu'))
    tr.build_model()
    batches = _batches()
    tr.network.eval()
    loss, p1, p5 = _expected(tr.network, batches)
    with caplog.at_level(logging.INFO):
        ret = tr.validate(batches)
    assert tr.network.training
    want = 'Validation: loss %.4f, prec@1 %.2f, prec@5 %.2f' % (loss, p1, p5)
    assert want in [r.getMessage() for r in caplog.records]
    assert '%.2f' % ret == '%.2f' % p1


def test_evaluator_returns_the_same_numbers():
    from ps_pytorch_amd.evaluator import DistributedEvaluator
    cfg = JobConfig(network='LeNet', dataset='MNIST')
    ev = DistributedEvaluator(cfg, max_polls=1)
    batches = _batches(seed=5)
    ev.network.eval()
    want = _expected(ev.network, batches)
    got = ev._evaluate_model(batches)
    line = 'Evaluator step %d: loss %.4f prec@1 %.2f prec@5 %.2f'
    assert line % ((50,) + tuple(got)) == line % ((50,) + want)


# ---- --train-metrics ----

def test_train_metrics_flag_parses():
    assert parse_args([]).train_metrics is False
    assert JobConfig.from_args(parse_args([])).train_metrics is False
    assert JobConfig.from_args(parse_args(['--train-metrics'])).train_metrics
    assert JobConfig.from_args(
        parse_args(['--train-metrics', 'false'])).train_metrics is False


STEP_RE = r'Step: \d+, Epoch: 0, Loss: [0-9.]+, Time: [0-9.]+'


def _train_lines(caplog, train_metrics):
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='LeNet', dataset='MNIST', batch_size=16, lr=0.01,
                    epochs=1, max_steps=4, log_interval=2,
                    train_metrics=train_metrics)
    tr = NNTrainer(cfg, device=torch.device('cpu'))
    tr.build_model()
    batches = _batches(seed=1, sizes=(16, 16, 16, 16))
    caplog.clear()
    with caplog.at_level(logging.INFO):
        tr.train_and_validate(batches, [])
    return tr, batches, [r.getMessage() for r in caplog.records
                         if r.getMessage().startswith('Step:')]


def test_train_metrics_off_leaves_the_step_line(caplog):
    tr, _, lines = _train_lines(caplog, False)
    assert tr.train_metrics is None and tr.read_train_metrics() is None
    assert len(lines) == 2
    for ln in lines:
        assert re.fullmatch(STEP_RE, ln), ln


def test_train_metrics_on_appends_prec_fields(caplog):
    tr, batches, lines = _train_lines(caplog, True)
    assert len(lines) == 2
    pat = STEP_RE + r', Prec@1: ([0-9.]+), Prec@5: ([0-9.]+)'
    for ln in lines:
        assert re.fullmatch(pat, ln), ln
    # the fields cover the steps since the last log line: replay the same
    # training with the flag off and count by hand
    from ps_pytorch_amd.trainer import NNTrainer
    cfg = JobConfig(network='LeNet', dataset='MNIST', batch_size=16, lr=0.01)
    ref = NNTrainer(cfg, device=torch.device('cpu'))
    ref.build_model()
    hits = []
    for x, y in batches:
        with torch.no_grad():
            out = ref.network(x)
        hits.append(ce_topk_reference(out, y, (1, 5))[1])
        ref.train_step(x, y)
    for ln, (a, b) in zip(lines, ((0, 1), (2, 3))):
        h = hits[a] + hits[b]
        m = re.fullmatch(pat, ln)
        assert m.group(1) == '%.2f' % (100.0 * int(h[0]) / 32)
        assert m.group(2) == '%.2f' % (100.0 * int(h[1]) / 32)


def _worker_lines(caplog, train_metrics):
    """DistributedWorker.train on the CPU with the transport stubbed out:
    the log lines are what is under test."""
    from ps_pytorch_amd.models import build_model
    from ps_pytorch_amd.parallel.flat import FlatSpace
    from ps_pytorch_amd.parallel.worker import DistributedWorker
    cfg = JobConfig(network='LeNet', dataset='MNIST', batch_size=16,
                    max_steps=2, log_interval=1, eval_freq=1000,
                    overlap=False, train_metrics=train_metrics)
    w = DistributedWorker(cfg, rank=1, world=2, device=torch.device('cpu'))
    torch.manual_seed(0)
    w.network = build_model('LeNet', num_classes=10, in_channels=1)
    w.flat = FlatSpace(w.network, bucket_bytes=1 << 20)
    w.flat.attach_grads(steal=False)
    w.ctrl = None
    w._next_launch = 0
    w.fetch_weights = lambda: None
    w.push_gradients = lambda killed=False: None
    caplog.clear()
    with caplog.at_level(logging.INFO):
        w.train(_batches(seed=2, sizes=(16, 16)))
    return [r.getMessage() for r in caplog.records
            if r.getMessage().startswith('Worker:')]


def test_worker_line_is_unchanged_and_metrics_get_their_own(caplog):
    from ps_pytorch_amd.tuning_parser import WORKER_RE, parse_losses
    from ps_pytorch_amd.utils.logging import WORKER_LINE
    assert WORKER_LINE == (
        'Worker: {}, Step: {}, Epoch: {} [{}/{} ({:.0f}%)], '
        'Loss: {:.4f}, Time Cost: {:.4f}, FetchWeight: {:.4f}, '
        'Forward: {:.4f}, Backward: {:.4f}, Comm Cost: {:.4f}')
    off = _worker_lines(caplog, False)
    assert len(off) == 2 and all(WORKER_RE.fullmatch(ln) for ln in off)
    on = _worker_lines(caplog, True)
    assert len(on) == 4
    strip = lambda ln: re.sub(r'(Cost|Weight|ward): [0-9.]+', r'\1: T', ln)
    assert [strip(ln) for ln in on[0::2]] == [strip(ln) for ln in off]
    for step, ln in zip((1, 2), on[1::2]):
        m = re.fullmatch(r'Worker: 1, Step: (\d+), Prec@1: ([0-9.]+), '
                         r'Prec@5: ([0-9.]+)', ln)
        assert m and int(m.group(1)) == step, ln
        assert 0.0 <= float(m.group(2)) <= float(m.group(3)) <= 100.0
    # the tuning parser sees the same losses with the extra lines present
    assert parse_losses(on) == parse_losses(off)
    assert not math.isnan(parse_losses(on)[1][1])
