"""Error-feedback packs (pack_q8_ef / pack_wire_ef), CPU reference path:
zero-residual equivalence with the plain packs, the telescoping property
that makes error feedback worth having, argument validation and the
--error-feedback flag surface."""
import warnings

import pytest
import torch

from ps_pytorch_amd.config import JobConfig, parse_args
from ps_pytorch_amd.ops import functional as F

U = 2.0 ** -23          # 2x the f32 unit roundoff of the one inexact op, g + e


def _recipe(n, T, dtype):
    """The issue's input recipe: a fixed base gradient plus per-step noise,
    with an outlier at the head of every 256-block."""
    g = torch.Generator().manual_seed(n)
    base = torch.randn(n, generator=g) * 0.01
    for _ in range(T):
        x = (base + 0.001 * torch.randn(n, generator=g)).to(dtype)
        x[::256] *= 50
        yield x


def _scales(payload, n):
    qb, tot = F.q8_layout(n)
    return payload[qb:tot].view(torch.float32)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 4099])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_q8_ef_zero_residual_equals_plain(n, dtype):
    x = next(_recipe(n, 1, dtype))
    _, tot = F.q8_layout(n)
    plain = torch.zeros(tot, dtype=torch.uint8)
    F.pack_q8(plain, x)
    ef = torch.zeros(tot, dtype=torch.uint8)
    res = torch.zeros(n)
    F.pack_q8_ef(ef, x, res)
    assert torch.equal(ef, plain)
    dec = torch.empty(n)
    F.unpack_q8(dec, ef)
    assert torch.equal(res, x.float() - dec)


@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_wire_ef_zero_residual_equals_plain(n):
    x = next(_recipe(n, 1, torch.float32))
    plain = torch.zeros(n, dtype=torch.bfloat16)
    F.pack_wire(plain, x)
    ef = torch.zeros(n, dtype=torch.bfloat16)
    res = torch.zeros(n)
    F.pack_wire_ef(ef, x, res)
    assert torch.equal(ef, plain)
    assert torch.equal(res, x - ef.float())


TELESCOPE_CASES = [(257, 64, torch.float32), (1000, 64, torch.bfloat16),
                   (4099, 200, torch.float32)]


@pytest.mark.parametrize("n,T,dtype", TELESCOPE_CASES)
def test_q8_ef_telescopes(n, T, dtype):
    """sum(decoded) tracks sum(true gradients) to within the residual, for
    any number of steps: |sum dec - sum g + e_T| <= 2^-23 * sum(|g_t| +
    |e_{t-1}|) (the rounding of c = g + e; c - dec is exact), and the
    residual itself stays within (0.5 + 2^-14) quantization steps."""
    _, tot = F.q8_layout(n)
    payload = torch.zeros(tot, dtype=torch.uint8)
    res = torch.zeros(n)
    dec = torch.empty(n)
    sum_dec = torch.zeros(n, dtype=torch.float64)
    sum_g = torch.zeros(n, dtype=torch.float64)
    bound = torch.zeros(n, dtype=torch.float64)
    plain_dec = torch.zeros(n, dtype=torch.float64)
    plain_payload = torch.zeros(tot, dtype=torch.uint8)
    for x in _recipe(n, T, dtype):
        bound += x.double().abs() + res.double().abs()
        F.pack_q8_ef(payload, x, res)
        F.unpack_q8(dec, payload)
        sum_dec += dec.double()
        sum_g += x.double()
        F.pack_q8(plain_payload, x)
        F.unpack_q8(dec, plain_payload)
        plain_dec += dec.double()
    tele = (sum_dec - sum_g + res.double()).abs()
    ratio = (tele / (U * bound)).max().item()
    step = _scales(payload, n).repeat_interleave(F.Q8_BLOCK)[:n].double()
    half = (res.double().abs() / step).max().item()
    print(f"n={n} T={T} {dtype}: telescoping {ratio:.4f} of bound, "
          f"|e_T|/scale {half:.7f}, EF error "
          f"{(sum_dec - sum_g).abs().max().item():.4g}, plain error "
          f"{(plain_dec - sum_g).abs().max().item():.4g}")
    assert (tele <= U * bound).all()
    assert (res.double().abs() <= (0.5 + 2.0 ** -14) * step).all()


@pytest.mark.parametrize("n,T", [(n, T) for n, T, _ in TELESCOPE_CASES])
def test_wire_ef_telescopes(n, T):
    wire = torch.zeros(n, dtype=torch.bfloat16)
    res = torch.zeros(n)
    sum_dec = torch.zeros(n, dtype=torch.float64)
    sum_g = torch.zeros(n, dtype=torch.float64)
    bound = torch.zeros(n, dtype=torch.float64)
    for x in _recipe(n, T, torch.float32):
        bound += x.double().abs() + res.double().abs()
        c = x + res
        F.pack_wire_ef(wire, x, res)
        sum_dec += wire.double()
        sum_g += x.double()
    tele = (sum_dec - sum_g + res.double()).abs()
    print(f"n={n} T={T}: telescoping "
          f"{(tele / (U * bound)).max().item():.4f} of bound")
    assert (tele <= U * bound).all()
    assert (res.double().abs() <= 2.0 ** -8 * c.double().abs()).all()


def test_ef_validation_errors():
    n = 300
    x = torch.randn(n)
    _, tot = F.q8_layout(n)
    payload = torch.zeros(tot, dtype=torch.uint8)
    wire = torch.zeros(n, dtype=torch.bfloat16)
    bad = [torch.zeros(n, dtype=torch.bfloat16),      # dtype
           torch.zeros(n + 1),                         # size
           torch.zeros(2 * n)[::2]]                    # non-contiguous
    for res in bad:
        with pytest.raises((TypeError, ValueError)):
            F.pack_q8_ef(payload, x, res)
        with pytest.raises((TypeError, ValueError)):
            F.pack_wire_ef(wire, x, res)
    with pytest.raises(TypeError):
        F.pack_q8_ef(payload, x, torch.zeros(n, dtype=torch.float64))
    with pytest.raises(ValueError):
        F.pack_q8_ef(payload, x, torch.zeros(n - 1))
    with pytest.raises(ValueError):
        F.pack_q8_ef(payload[:-4], x, torch.zeros(n))
    with pytest.raises(TypeError):     # the EF wire pack is f32 -> bf16 only
        F.pack_wire_ef(torch.zeros(n), x, torch.zeros(n))


def test_error_feedback_flag_and_config():
    assert parse_args([]).error_feedback is False
    assert parse_args(['--error-feedback']).error_feedback is True
    assert parse_args(['--error-feedback', 'false']).error_feedback is False
    assert JobConfig().error_feedback is False
    cfg = JobConfig.from_args(parse_args(['--error-feedback',
                                          '--aggregation', 'gather']))
    assert cfg.error_feedback is True
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        cfg = JobConfig(error_feedback=True, compress_grad='None',
                        wire_dtype='fp32')
    assert cfg.error_feedback is False
    assert any('error-feedback' in str(w.message) for w in rec)
    # a lossy combination stays on, silently
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        cfg = JobConfig(error_feedback=True, compress_grad='compress',
                        aggregation='gather')
    assert cfg.error_feedback is True and not rec


def test_transport_activates_only_where_the_push_is_lossy():
    """Single-process PSTransport: a worker rank with the q8 codec owns a
    zeroed residual; a lossless wire warns and runs without one; the PS
    rank never owns one."""
    from ps_pytorch_amd.models import build_model
    from ps_pytorch_amd.parallel.flat import FlatSpace
    from ps_pytorch_amd.parallel.transport import PSTransport
    fs = FlatSpace(build_model('LeNet', num_classes=10, in_channels=1))
    dev = torch.device('cpu')
    t = PSTransport(fs, torch.float32, dev, 1, 2, mode='gather',
                    compress=True, error_feedback=True)
    assert t.ef_active and t.residual.dtype == torch.float32
    assert t.residual.numel() == fs.padded and not t.residual.any()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        t = PSTransport(fs, torch.float32, dev, 1, 2, mode='collective',
                        compress=True, error_feedback=True)
    assert not t.ef_active and not hasattr(t, 'residual')
    assert any('error-feedback' in str(w.message) for w in rec)
    t = PSTransport(fs, torch.float32, dev, 0, 2, mode='gather',
                    compress=True, error_feedback=True)
    assert not t.ef_active
