"""Error-feedback pack kernels vs the CPU reference: bitwise-identical
payloads AND residuals over chained steps (the kernels keep dec = q*scale and
e' = c - dec as two separately rounded f32 operations, which is what makes
the torch path an exact oracle), tails, bucket-slice views and canaries."""
import pytest
import torch

from ps_pytorch_amd.ops import functional as F

pytestmark = pytest.mark.gpu

# every tail shape of a 4-wide quad and a 256-block, more than one workgroup,
# and one size past the 2048-workgroup launch cap (grid-stride loop)
SIZES = [1, 3, 255, 256, 257, 260, 4101, (1 << 20) + 13, (1 << 21) + 257]
STEPS = 3
CANARY = 0xAB


def _inputs(n, dtype, seed_off=0):
    """(per-step sources, starting residual); whole 256-blocks of zeros
    (source and residual) wherever n has room, the m == 0 case."""
    g = torch.Generator().manual_seed(n + seed_off)
    xs = [(torch.randn(n, generator=g) * 0.01).to(dtype) for _ in range(STEPS)]
    res = torch.randn(n, generator=g) * 1e-4
    for lo in (0, 512):
        if n >= lo + 256:
            res[lo:lo + 256] = 0
            for x in xs:
                x[lo:lo + 256] = 0
    return xs, res


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_q8_ef_bitwise_matches_cpu(n, dtype):
    xs, res = _inputs(n, dtype)
    _, tot = F.q8_layout(n)
    r_cpu, r_gpu = res.clone(), res.cuda()
    for x in xs:
        p_cpu = torch.full((tot,), CANARY, dtype=torch.uint8)
        p_gpu = torch.full((tot,), CANARY, dtype=torch.uint8, device='cuda')
        F.pack_q8_ef(p_cpu, x, r_cpu)
        F.pack_q8_ef(p_gpu, x.cuda(), r_gpu)
        # incl. the up-to-3 pad bytes behind the quants, which nobody writes
        assert torch.equal(p_gpu.cpu(), p_cpu)
        assert torch.equal(r_gpu.cpu(), r_cpu)
    if n >= 256:
        assert not r_cpu[:256].any()          # the all-zero block stays zero


@pytest.mark.parametrize("n", [3, 257, 260, 4101])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_q8_ef_bucket_slice_and_canaries(n, dtype):
    """Views 8 elements into larger buffers (the bucket-slice alignment);
    nothing may be written before the slice, at or past n in the residual,
    in the pad bytes behind the quants, or past the scales."""
    xs, res = _inputs(n, dtype, seed_off=7)
    qb, tot = F.q8_layout(n)
    off, slack = 8, 64
    r_cpu = res.clone()
    r_big = torch.full((off + n + slack,), 777.0, device='cuda')
    r_big[off:off + n] = res.cuda()
    for x in xs:
        x_big = torch.full((off + n + slack,), 3.0, dtype=dtype, device='cuda')
        x_big[off:off + n] = x.cuda()
        p_cpu = torch.full((tot,), CANARY, dtype=torch.uint8)
        p_big = torch.full((16 + tot + slack,), CANARY, dtype=torch.uint8,
                           device='cuda')
        F.pack_q8_ef(p_cpu, x, r_cpu)
        F.pack_q8_ef(p_big[16:16 + tot], x_big[off:off + n],
                     r_big[off:off + n])
        assert torch.equal(p_big[16:16 + tot].cpu(), p_cpu)
        assert (p_big[:16] == CANARY).all() and (p_big[16 + tot:] == CANARY).all()
        assert (p_big[16 + n:16 + qb] == CANARY).all()
        assert torch.equal(r_big[off:off + n].cpu(), r_cpu)
        assert (r_big[:off] == 777.0).all() and (r_big[off + n:] == 777.0).all()


@pytest.mark.parametrize("n", SIZES)
def test_wire_ef_bitwise_matches_cpu(n):
    xs, res = _inputs(n, torch.float32, seed_off=13)
    off, slack = 8, 64
    r_cpu = res.clone()
    r_big = torch.full((off + n + slack,), 777.0, device='cuda')
    r_big[off:off + n] = res.cuda()
    for x in xs:
        x_big = torch.full((off + n + slack,), 3.0, device='cuda')
        x_big[off:off + n] = x.cuda()
        w_cpu = torch.zeros(n, dtype=torch.bfloat16)
        w_big = torch.full((off + n + slack,), 5.0, dtype=torch.bfloat16,
                           device='cuda')
        F.pack_wire_ef(w_cpu, x, r_cpu)
        F.pack_wire_ef(w_big[off:off + n], x_big[off:off + n],
                       r_big[off:off + n])
        assert torch.equal(w_big[off:off + n].cpu(), w_cpu)
        assert (w_big[:off] == 5.0).all() and (w_big[off + n:] == 5.0).all()
        assert torch.equal(r_big[off:off + n].cpu(), r_cpu)
        assert (r_big[:off] == 777.0).all() and (r_big[off + n:] == 777.0).all()


@pytest.mark.parametrize("n", [257, 4101, (1 << 20) + 13])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_q8_ef_zero_residual_equals_plain_pack_on_gpu(n, dtype):
    x = _inputs(n, dtype, seed_off=21)[0][0].cuda()
    _, tot = F.q8_layout(n)
    plain = torch.zeros(tot, dtype=torch.uint8, device='cuda')
    F.pack_q8(plain, x)
    ef = torch.zeros(tot, dtype=torch.uint8, device='cuda')
    res = torch.zeros(n, device='cuda')
    F.pack_q8_ef(ef, x, res)
    assert torch.equal(ef, plain)
    dec = torch.empty(n, device='cuda')
    F.unpack_q8(dec, ef)
    assert torch.equal(res, x.float() - dec)


def test_wire_ef_zero_residual_equals_plain_pack_on_gpu():
    n = 4101
    x = _inputs(n, torch.float32, seed_off=22)[0][0].cuda()
    plain = torch.zeros(n, dtype=torch.bfloat16, device='cuda')
    F.pack_wire(plain, x)
    ef = torch.zeros(n, dtype=torch.bfloat16, device='cuda')
    res = torch.zeros(n, device='cuda')
    F.pack_wire_ef(ef, x, res)
    assert torch.equal(ef, plain)
    assert torch.equal(res, x - ef.float())
