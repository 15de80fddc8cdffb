"""Block top-k sparsifying codec (ops/kernels/topk.hip), CPU path: the
contract of ops.functional.pack_topk_ef / unpack_topk (this path is the
bitwise oracle of the kernels and the gloo path), and the config surface."""
import warnings

import pytest
import torch

from ps_pytorch_amd.config import JobConfig, parse_args
from ps_pytorch_amd.ops import functional as F

KS = (4, 8, 16, 32)


def _pack(x, res, k):
    off, tot = F.topk_layout(x.numel(), k)
    payload = torch.full((tot,), 0xAB, dtype=torch.uint8)
    F.pack_topk_ef(payload, x, res, k)
    idx = payload[:off].view(-1, k).to(torch.int64)
    vals = payload[off:].clone().view(torch.bfloat16).view(-1, k)
    return payload, idx, vals


def test_layout_sizes():
    assert F.TOPK_KS == KS
    for k in KS:
        assert F.topk_layout(1, k) == (k, 3 * k)
        assert F.topk_layout(256, k) == (k, 3 * k)
        assert F.topk_layout(257, k) == (2 * k, 6 * k)
        assert F.topk_layout(4101, k) == (17 * k, 51 * k)
    # 3*K bytes per 256 f32 values: 5.33x under the q8 payload at K = 16
    assert F.q8_layout(1 << 20)[1] / F.topk_layout(1 << 20, 16)[1] > 5.0
    for k in (0, 1, 5, 64, 256):
        with pytest.raises(ValueError):
            F.topk_layout(300, k)


def test_argument_errors():
    n, k = 300, 16
    x = torch.randn(n)
    off, tot = F.topk_layout(n, k)
    payload = torch.zeros(tot, dtype=torch.uint8)
    res = torch.zeros(n)
    F.pack_topk_ef(payload, x, res, k)                 # the good call
    with pytest.raises(ValueError):                    # k outside the set
        F.pack_topk_ef(payload, x, res, 5)
    with pytest.raises(ValueError):                    # payload size
        F.pack_topk_ef(payload[:-2], x, res, k)
    with pytest.raises(ValueError):                    # payload dtype
        F.pack_topk_ef(payload.view(torch.int8), x, res, k)
    with pytest.raises(ValueError):                    # payload stride
        F.pack_topk_ef(torch.zeros(2 * tot, dtype=torch.uint8)[::2], x, res, k)
    with pytest.raises(ValueError):                    # payload alignment
        F.pack_topk_ef(torch.zeros(tot + 1, dtype=torch.uint8)[1:], x, res, k)
    with pytest.raises(TypeError):                     # source dtype
        F.pack_topk_ef(payload, x.double(), res, k)
    with pytest.raises(ValueError):                    # source stride
        F.pack_topk_ef(payload, torch.zeros(2 * n)[::2], res, k)
    with pytest.raises(TypeError):                     # residual dtype
        F.pack_topk_ef(payload, x, torch.zeros(n, dtype=torch.bfloat16), k)
    with pytest.raises(ValueError):                    # residual size
        F.pack_topk_ef(payload, x, torch.zeros(n + 1), k)
    with pytest.raises(ValueError):                    # residual stride
        F.pack_topk_ef(payload, x, torch.zeros(2 * n)[::2], k)
    dst = torch.zeros(n)
    F.unpack_topk(dst, payload, k)
    with pytest.raises(ValueError):
        F.unpack_topk(dst, payload, 3)
    with pytest.raises(ValueError):
        F.unpack_topk(dst, payload[:-2], k)
    with pytest.raises(ValueError):
        F.unpack_topk(dst, payload.view(torch.int8), k)
    with pytest.raises(ValueError):
        F.unpack_topk(dst, torch.zeros(tot + 1, dtype=torch.uint8)[1:], k)
    with pytest.raises(TypeError):
        F.unpack_topk(dst.to(torch.bfloat16), payload, k)
    with pytest.raises(ValueError):
        F.unpack_topk(torch.zeros(2 * n)[::2], payload, k)
    # (the device-match checks need two devices: tests/test_topk_gpu.py)


@pytest.mark.parametrize("k", KS)
def test_tie_rule_all_equal_block_selects_lowest_indices(k):
    """Equal magnitudes of either sign: the lower index wins."""
    x = torch.full((512,), 0.5)
    x[1::2] = -0.5
    res = torch.zeros(512)
    _, idx, vals = _pack(x, res, k)
    assert torch.equal(idx, torch.arange(k).repeat(2, 1))
    assert torch.equal(vals.float(), x[:k].repeat(2, 1))
    want = x.clone().view(2, 256)
    want[:, :k] = 0                                     # sent exactly
    assert torch.equal(res, want.view(-1))


def test_selection_is_by_magnitude_then_index_in_ascending_order():
    k = 4
    x = torch.zeros(256)
    x[200], x[7], x[100], x[30], x[31] = -9.0, 3.0, 5.0, -3.0, 3.0
    res = torch.zeros(256)
    _, idx, vals = _pack(x, res, k)
    assert idx.tolist() == [[7, 30, 100, 200]]          # 31 loses the tie
    assert vals.float().tolist() == [[3.0, -3.0, 5.0, -9.0]]
    assert res[31] == 3.0 and res.abs().sum() == 3.0
    # the residual takes part in the selection
    res = torch.zeros(256)
    res[50] = 20.0
    _, idx, _ = _pack(x, res, k)
    assert idx.tolist() == [[7, 50, 100, 200]]
    assert res[30] == -3.0 and res[31] == 3.0 and res[50] == 0.0


def test_value_is_bf16_rne_and_residual_is_the_exact_remainder():
    k = 4
    x = torch.zeros(256)
    x[3] = 1.0 + 2.0 ** -8          # half way between two bf16: to even (1.0)
    x[5] = 1.0 + 3 * 2.0 ** -8      # half way: to even (1 + 2^-6)
    x[9] = -(1.0 + 2.0 ** -9)
    res = torch.zeros(256)
    _, idx, vals = _pack(x, res, k)
    assert idx.tolist() == [[0, 3, 5, 9]]               # +0 at index 0 pads
    assert vals.float().tolist() == [[0.0, 1.0, 1.0 + 2.0 ** -6, -1.0]]
    assert res[3] == 2.0 ** -8 and res[5] == -(2.0 ** -8)
    assert res[9] == -(2.0 ** -9)


def test_tail_block_shorter_than_k():
    n, k = 8, 16
    x = torch.arange(1, n + 1, dtype=torch.float32)
    res = torch.zeros(n)
    payload, idx, vals = _pack(x, res, k)
    assert idx.tolist() == [list(range(16))]
    assert torch.equal(vals.float()[0, :n], x)
    # the pad entries carry +0 (all payload bits zero, sign included)
    assert not vals[0, n:].view(torch.int16).any()
    assert not res.any()
    big = torch.full((n + 32,), 7.0)
    F.unpack_topk(big[:n], payload, k)
    assert torch.equal(big[:n], x) and (big[n:] == 7.0).all()
    F.unpack_topk(big[:n], payload, k, accumulate=True)
    assert torch.equal(big[:n], 2 * x) and (big[n:] == 7.0).all()


@pytest.mark.parametrize("k", KS)
def test_non_finite_values_are_always_sent(k):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(600, generator=g) * 1e30            # large finite values
    x[300], x[511] = float('inf'), float('nan')
    x[17] = float('-inf')
    res = torch.zeros(600)
    _, idx, vals = _pack(x, res, k)
    assert 17 in idx[0].tolist()
    assert {300 - 256, 511 - 256} <= set(idx[1].tolist())
    sent = vals.float()
    assert torch.isinf(sent[1][idx[1] == 44]).all()
    assert torch.isnan(sent[1][idx[1] == 255]).all()
    assert torch.isfinite(sent[2]).all()


def test_all_zero_payload():
    for k in KS:
        n = 700
        _, tot = F.topk_layout(n, k)
        payload = torch.zeros(tot, dtype=torch.uint8)
        dst = torch.full((n,), 3.0)
        F.unpack_topk(dst, payload, k)
        assert not dst.any()
        keep = torch.randn(n)
        dst = keep.clone()
        F.unpack_topk(dst, payload, k, accumulate=True)
        assert torch.equal(dst, keep)


def test_decoder_adds_duplicate_indices_in_payload_order():
    n, k = 300, 4
    off, tot = F.topk_layout(n, k)
    payload = torch.zeros(tot, dtype=torch.uint8)
    payload[:off] = torch.tensor([5, 5, 9, 5, 43, 44, 43, 200],
                                 dtype=torch.uint8)
    vals = torch.tensor([1.0, 2.0, 4.0, 8.0, 1.0, 2.0, 4.0, 8.0],
                        dtype=torch.bfloat16)
    payload[off:] = vals.view(torch.uint8)
    dst = torch.zeros(n)
    F.unpack_topk(dst, payload, k)
    want = torch.zeros(n)
    want[5], want[9] = 11.0, 4.0
    want[256 + 43] = 5.0
    # 256 + 44 and 256 + 200 lie at or past n: skipped
    assert torch.equal(dst, want)


@pytest.mark.parametrize("k", KS)
def test_conservation_is_exact_on_integers(k):
    """Nothing is lost: over a chain of steps, what was decoded plus what
    is still in the residual is the sum of the gradients. Small integers keep
    every value exact in bf16 and f32 (|residual| <= 7 * steps < 256)."""
    n, steps = 4101, 8
    g = torch.Generator().manual_seed(11)
    _, tot = F.topk_layout(n, k)
    res = torch.zeros(n)
    sum_g, sum_dec = torch.zeros(n), torch.zeros(n)
    for _ in range(steps):
        x = torch.randint(-7, 8, (n,), generator=g).float()
        payload = torch.zeros(tot, dtype=torch.uint8)
        F.pack_topk_ef(payload, x, res, k)
        F.unpack_topk(sum_dec, payload, k, accumulate=True)
        sum_g += x
    assert torch.equal(sum_dec + res, sum_g)
    assert res.any() and sum_dec.any()


def test_bf16_source_matches_its_f32_image():
    n, k = 1000, 8
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, generator=g) * 0.01).to(torch.bfloat16)
    res0 = torch.randn(n, generator=g) * 1e-4
    ra, rb = res0.clone(), res0.clone()
    pa, _, _ = _pack(x, ra, k)
    pb, _, _ = _pack(x.float(), rb, k)
    assert torch.equal(pa, pb) and torch.equal(ra, rb)


def test_flags_defaults_and_validation():
    a = parse_args([])
    assert a.compress_codec == 'q8' and a.topk_k == 16
    a = parse_args(['--compress-codec', 'topk', '--topk-k', '8'])
    assert a.compress_codec == 'topk' and a.topk_k == 8
    assert JobConfig().compress_codec == 'q8' and JobConfig().topk_k == 16
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        cfg = JobConfig.from_args(parse_args(
            ['--compress-codec', 'topk', '--topk-k', '32', '--aggregation',
             'gather', '--error-feedback']))
    assert (cfg.compress_codec, cfg.topk_k, cfg.error_feedback) == \
        ('topk', 32, True)
    assert not rec
    with pytest.raises(ValueError):
        JobConfig(compress_codec='snappy')
    for k in (0, 5, 64):
        with pytest.raises(ValueError):
            JobConfig(topk_k=k)


def _cfg_warns(**kw):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        cfg = JobConfig(**kw)
    return cfg, [str(w.message) for w in rec]


def test_normalize_and_warn_rules():
    # collective mode ignores gradient codecs: falls back, naming the codec
    cfg, msgs = _cfg_warns(compress_codec='topk', aggregation='collective',
                           error_feedback=True, wire_dtype='bf16')
    assert cfg.compress_codec == 'q8' and any('topk' in m for m in msgs)
    # ... and so does a run without --compress-grad compress
    cfg, msgs = _cfg_warns(compress_codec='topk', aggregation='gather',
                           compress_grad='None')
    assert cfg.compress_codec == 'q8' and any('topk' in m for m in msgs)
    assert cfg.error_feedback is False
    # feedback off: switched on
    cfg, msgs = _cfg_warns(compress_codec='topk', aggregation='gather')
    assert cfg.compress_codec == 'topk' and cfg.error_feedback is True
    assert any('topk' in m and 'error-feedback' in m for m in msgs)
    # --mode kill moves to gather first, so the codec survives
    cfg, msgs = _cfg_warns(compress_codec='topk', mode='kill',
                           error_feedback=True)
    assert cfg.aggregation == 'gather' and cfg.compress_codec == 'topk'
    # the allreduce engine runs without it
    cfg, msgs = _cfg_warns(compress_codec='topk', aggregation='gather',
                           engine='allreduce')
    assert cfg.compress_codec == 'q8' and cfg.error_feedback is False
    assert any('topk' in m and 'allreduce' in m for m in msgs)


def test_transport_frames_payloads_through_topk_layout():
    from ps_pytorch_amd.models import build_model
    from ps_pytorch_amd.parallel.flat import FlatSpace
    from ps_pytorch_amd.parallel.transport import PSTransport
    fs = FlatSpace(build_model('LeNet', num_classes=10, in_channels=1),
                   bucket_bytes=int(0.25 * 2 ** 20))
    assert len(fs.buckets) > 1
    dev = torch.device('cpu')
    sizes = [F.topk_layout(b.numel, 8)[1] for b in fs.buckets]
    # worker: residual without being asked, payload and zero payload sized
    w = PSTransport(fs, torch.float32, dev, 1, 2, mode='gather',
                    compress=True, codec='topk', topk_k=8)
    assert w.ef_active and not w.residual.any()
    assert [t for _, t in w._pl_off] == sizes
    assert w.payload.numel() == sum(sizes)
    assert w._zero_payload.numel() == max(sizes)
    ps = PSTransport(fs, torch.float32, dev, 0, 2, mode='gather',
                     compress=True, codec='topk', topk_k=8)
    assert not ps.ef_active and ps.stages[0].numel() == sum(sizes)
    # collective mode has no codec at all
    c = PSTransport(fs, torch.float32, dev, 1, 2, mode='collective',
                    compress=True, codec='topk', topk_k=8)
    assert c.codec is None and not c.ef_active
    with pytest.raises(ValueError):
        PSTransport(fs, torch.float32, dev, 1, 2, mode='gather',
                    compress=True, codec='topk', topk_k=5)
    with pytest.raises(ValueError):
        PSTransport(fs, torch.float32, dev, 1, 2, mode='gather',
                    compress=True, codec='lz4')
