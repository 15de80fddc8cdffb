"""Counter-based dropout: the Philox CPU oracle (ops/functional.py) and the
PsDropout / PsReLU modules on CPU. The GPU kernels are checked bit for bit
against this oracle in test_dropout_gpu.py."""
import math

import numpy as np
import pytest
import torch

from ps_pytorch_amd.ops.dropout import PsDropout, PsReLU
from ps_pytorch_amd.ops.functional import (act_drop_bwd_ref, act_drop_ref,
                                           dropout_keep_mask, dropout_scale,
                                           philox4x32_10)

N = 524288
KW = dict(seed=1234, salt=1, stream=0, step=0)


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize('ctr,key,out', [
    ('0 0 0 0', '0 0', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff',
     '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0',
     'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answers(ctr, key, out):
    got = philox4x32_10(_words(ctr), _words(key))
    assert [int(v) for v in got] == _words(out)


def test_philox_batched_matches_single():
    ctr = np.array([_words('0 0 0 0'),
                    _words('243f6a88 85a308d3 13198a2e 03707344')])
    key = np.array([_words('0 0'), _words('a4093822 299f31d0')])
    got = philox4x32_10(ctr, key)
    assert got.shape == (2, 4)
    assert [int(v) for v in got[0]] == _words(
        '6627e8d5 e169c58d bc57ac4c 9b00dbd8')
    assert [int(v) for v in got[1]] == _words(
        'd16cfe09 94fdcceb 5001e420 24126ea1')


@pytest.fixture(scope='module')
def base_mask():
    return dropout_keep_mask(N, 0.5, **KW)


@pytest.mark.parametrize('p', [0.1, 0.5, 0.9])
def test_keep_fraction(p):
    frac = dropout_keep_mask(N, p, **KW).float().mean().item()
    sigma = math.sqrt(p * (1 - p) / N)
    assert abs(frac - (1 - p)) <= 4 * sigma, (p, frac, sigma)


@pytest.mark.parametrize('change', [dict(step=1), dict(salt=2),
                                    dict(stream=1)])
def test_mask_decorrelates(base_mask, change):
    other = dropout_keep_mask(N, 0.5, **{**KW, **change})
    agree = (other == base_mask).float().mean().item()
    assert 0.49 <= agree <= 0.51, (change, agree)


def test_mask_repeats(base_mask):
    assert torch.equal(dropout_keep_mask(N, 0.5, **KW), base_mask)


def test_mask_p_edges():
    assert dropout_keep_mask(1000, 0.0, **KW).all()
    assert not dropout_keep_mask(1000, 1.0, **KW).any()


def test_counter_layout_independent_of_n():
    small = dropout_keep_mask(13, 0.5, **KW)
    big = dropout_keep_mask(4096, 0.5, **KW)
    assert small.dtype == torch.bool and small.shape == (13,)
    assert torch.equal(small, big[:13])


def test_mask_uses_high_seed_word():
    a = dropout_keep_mask(4096, 0.5, seed=7, salt=0, stream=0, step=0)
    b = dropout_keep_mask(4096, 0.5, seed=7 + (1 << 32), salt=0, stream=0,
                          step=0)
    assert not torch.equal(a, b)


# ---- PsDropout on CPU ----

@pytest.mark.parametrize('relu', [False, True])
def test_psdropout_cpu_matches_oracle(relu):
    torch.manual_seed(77)
    m = PsDropout(p=0.1, relu=relu, salt=3)
    m.stream = 2
    m.train()
    x = torch.randn(33, 17)
    x[0, :4] = 0.0
    scale = dropout_scale(0.1)
    for step in range(3):
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        keep = dropout_keep_mask(x.numel(), 0.1, seed=77, salt=3, stream=2,
                                 step=step)
        y_ref, bits = act_drop_ref(x, keep, scale, relu)
        assert torch.equal(y, y_ref), step
        dy = torch.randn_like(x)
        y.backward(dy)
        assert torch.equal(xi.grad, act_drop_bwd_ref(dy, bits, scale)), step
        # the mask the backward used is the forward's
        assert torch.equal(xi.grad != 0, bits & (dy != 0))
    assert m.host_step == 3


def test_psdropout_scale_and_fraction():
    torch.manual_seed(5)
    m = PsDropout(p=0.5).train()
    y = m(torch.ones(4096))
    assert set(y.unique().tolist()) == {0.0, 2.0}


def test_psdropout_eval_is_identity():
    x = torch.randn(8, 5)
    m = PsDropout(p=0.5).eval()
    assert m(x) is x
    mr = PsDropout(p=0.5, relu=True).eval()
    assert torch.equal(mr(x), torch.relu(x))
    assert m.host_step == 0 and mr.host_step == 0


def test_psdropout_has_no_state():
    m = PsDropout(p=0.5).train()
    m(torch.randn(16))
    assert m.stream == 0
    assert len(m.state_dict()) == 0
    assert list(m.named_buffers()) == []
    assert list(m.parameters()) == []


def test_psdropout_reseed_repeats_sequence():
    x = torch.randn(257)

    def run(seed):
        torch.manual_seed(seed)
        m = PsDropout(p=0.5).train()
        return [m(x).clone() for _ in range(3)]

    a, b, c = run(11), run(11), run(12)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a[0], a[1])
    assert not torch.equal(a[0], c[0])


def test_psdropout_p_edges():
    x = torch.randn(100)
    assert torch.equal(PsDropout(p=0.0).train()(x), x)
    assert torch.equal(PsDropout(p=1.0).train()(x), torch.zeros(100))


def test_psrelu_cpu():
    x = torch.randn(4, 6, 3, 3, requires_grad=True)
    y = PsReLU()(x)
    assert torch.equal(y, torch.relu(x))
    y.sum().backward()
    assert torch.equal(x.grad, (x > 0).float())
