"""Block top-k codec kernels (ops/kernels/topk.hip) vs the CPU path of
ops.functional: bitwise-identical payloads and residuals over chained steps,
tails, ties, non-finite values, bucket-slice views with canaries, the
decoder with repeated and out-of-range indices, and the device round trip."""
import pytest
import torch

from ps_pytorch_amd.ops import functional as F

pytestmark = pytest.mark.gpu

KS = (4, 8, 16, 32)
# every tail shape of a 4-wide quad and a 256-block, a tail block shorter
# than K, more than one workgroup, and one size past the 2048-workgroup
# launch cap (grid-stride loop)
SIZES = [1, 3, 8, 248, 255, 256, 257, 264, 4101, (1 << 21) + 264]
STEPS = 3
CANARY = 0xAB
TIE_VALUES = torch.tensor([0.5, -0.5, 0.25, -0.25, 1.0, -1.0, 0.0])


def _inputs(n, dtype, seed_off=0):
    """(per-step sources, starting residual); whole 256-blocks of zeros
    (source and residual) wherever n has room, and one block of repeated
    magnitudes of both signs on a zero residual: [256, 512) where n reaches
    that far, the head of the only block where n < 256."""
    g = torch.Generator().manual_seed(n + seed_off)
    xs = [(torch.randn(n, generator=g) * 0.01).to(dtype) for _ in range(STEPS)]
    res = torch.randn(n, generator=g) * 1e-4
    for lo in (0, 512):
        if n >= lo + 256:
            res[lo:lo + 256] = 0
            for x in xs:
                x[lo:lo + 256] = 0
    tie = (256, 512) if n >= 512 else (0, n) if n < 256 else None
    if tie is not None:
        lo, hi = tie
        res[lo:hi] = 0
        for x in xs:
            pick = torch.randint(0, len(TIE_VALUES), (hi - lo,), generator=g)
            x[lo:hi] = TIE_VALUES[pick].to(dtype)
    return xs, res


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_topk_ef_bitwise_matches_cpu(n, dtype):
    xs, res = _inputs(n, dtype)
    xs_gpu = [x.cuda() for x in xs]
    for k in KS:
        _, tot = F.topk_layout(n, k)
        r_cpu, r_gpu = res.clone(), res.cuda()
        for x, xg in zip(xs, xs_gpu):
            p_cpu = torch.full((tot,), CANARY, dtype=torch.uint8)
            p_gpu = torch.full((tot,), CANARY, dtype=torch.uint8,
                               device='cuda')
            F.pack_topk_ef(p_cpu, x, r_cpu, k)
            F.pack_topk_ef(p_gpu, xg, r_gpu, k)
            assert torch.equal(p_gpu.cpu(), p_cpu), k
            assert torch.equal(r_gpu.cpu().view(torch.int32),
                               r_cpu.view(torch.int32)), k
        if n >= 256:
            assert not r_cpu[:256].any()      # the all-zero block stays zero


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_topk_ef_non_finite(dtype):
    """+-Inf and NaN are always sent; compared by selected indices and by
    the isfinite pattern (NaN payload bits are nobody's contract). At most 3
    non-finite values per block, so all of them fit every K."""
    n = 4101
    xs, res = _inputs(n, dtype, seed_off=31)
    for x, at in zip(xs, ([5, 300, 301, 1023], [256, 4100], [700, 701, 767])):
        x[at] = torch.tensor([float('inf'), float('-inf'), float('nan'),
                              float('inf')], dtype=dtype)[:len(at)]
    for k in KS:
        off, tot = F.topk_layout(n, k)
        r_cpu, r_gpu = res.clone(), res.cuda()
        for x in xs:
            p_cpu = torch.zeros(tot, dtype=torch.uint8)
            p_gpu = torch.zeros(tot, dtype=torch.uint8, device='cuda')
            F.pack_topk_ef(p_cpu, x, r_cpu, k)
            F.pack_topk_ef(p_gpu, x.cuda(), r_gpu, k)
            assert torch.equal(p_gpu[:off].cpu(), p_cpu[:off])
            v_cpu = p_cpu[off:].clone().view(torch.bfloat16)
            v_gpu = p_gpu[off:].cpu().view(torch.bfloat16)
            fin = torch.isfinite(v_cpu)
            assert not fin.all()
            assert torch.equal(torch.isfinite(v_gpu), fin)
            assert torch.equal(v_gpu[fin].view(torch.int16),
                               v_cpu[fin].view(torch.int16))
            got = r_gpu.cpu()
            fin = torch.isfinite(r_cpu)
            assert torch.equal(torch.isfinite(got), fin)
            assert torch.equal(got[fin], r_cpu[fin])


@pytest.mark.parametrize("n", [3, 8, 257, 264, 4101])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_topk_ef_bucket_slice_and_canaries(n, dtype):
    """Views 8 elements into larger buffers (the bucket-slice alignment);
    nothing may be written before the slice, at or past n in the residual,
    or outside the payload's total_bytes."""
    xs, res = _inputs(n, dtype, seed_off=7)
    off, slack = 8, 64
    for k in (4, 16):
        _, tot = F.topk_layout(n, k)
        r_cpu = res.clone()
        r_big = torch.full((off + n + slack,), 777.0, device='cuda')
        r_big[off:off + n] = res.cuda()
        for x in xs:
            x_big = torch.full((off + n + slack,), 3.0, dtype=dtype,
                               device='cuda')
            x_big[off:off + n] = x.cuda()
            p_cpu = torch.full((tot,), CANARY, dtype=torch.uint8)
            p_big = torch.full((16 + tot + slack,), CANARY, dtype=torch.uint8,
                               device='cuda')
            F.pack_topk_ef(p_cpu, x, r_cpu, k)
            F.pack_topk_ef(p_big[16:16 + tot], x_big[off:off + n],
                           r_big[off:off + n], k)
            assert torch.equal(p_big[16:16 + tot].cpu(), p_cpu)
            assert (p_big[:16] == CANARY).all()
            assert (p_big[16 + tot:] == CANARY).all()
            assert torch.equal(r_big[off:off + n].cpu(), r_cpu)
            assert (r_big[:off] == 777.0).all()
            assert (r_big[off + n:] == 777.0).all()
            assert (x_big[:off] == 3.0).all() and (x_big[off + n:] == 3.0).all()


def _payload(n, k, seed):
    """A real payload from the CPU encoder, and the dst it lands on (with
    negative zeros, which only a targeted add may turn positive)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    _, tot = F.topk_layout(n, k)
    payload = torch.zeros(tot, dtype=torch.uint8)
    F.pack_topk_ef(payload, x, torch.zeros(n), k)
    dst = torch.randn(n, generator=g)
    dst[::3] = -0.0
    return payload, dst


def _same_bits(a_gpu, b_cpu):
    return torch.equal(a_gpu.cpu().view(torch.int32), b_cpu.view(torch.int32))


@pytest.mark.parametrize("n", [1, 8, 255, 257, 4101, (1 << 21) + 264])
def test_unpack_topk_bitwise_matches_cpu(n):
    for k in KS:
        pa, dst = _payload(n, k, seed=n + k)
        pb, _ = _payload(n, k, seed=n + k + 100)
        pa_g, pb_g = pa.cuda(), pb.cuda()
        # plain decode overwrites whatever was there
        d_cpu, d_gpu = dst.clone(), dst.cuda()
        F.unpack_topk(d_cpu, pa, k)
        F.unpack_topk(d_gpu, pa_g, k)
        assert _same_bits(d_gpu, d_cpu), k
        # accumulate, two payloads in both orders
        for first, second in (((pa, pa_g), (pb, pb_g)),
                              ((pb, pb_g), (pa, pa_g))):
            d_cpu, d_gpu = dst.clone(), dst.cuda()
            for p_c, p_g in (first, second):
                F.unpack_topk(d_cpu, p_c, k, accumulate=True)
                F.unpack_topk(d_gpu, p_g, k, accumulate=True)
            assert _same_bits(d_gpu, d_cpu), k
        # the all-zero payload of a killed worker
        zero = torch.zeros_like(pa)
        d_cpu, d_gpu = dst.clone(), dst.cuda()
        F.unpack_topk(d_cpu, zero, k, accumulate=True)
        F.unpack_topk(d_gpu, zero.cuda(), k, accumulate=True)
        assert _same_bits(d_gpu, d_cpu), k
        F.unpack_topk(d_gpu, zero.cuda(), k)
        assert not d_gpu.any()


def test_unpack_topk_duplicates_and_entries_past_n():
    """A hand-built payload: repeated indices add in payload order, entries
    at or past n are skipped, and nothing is written around the slice."""
    n, k = 300, 4
    off, tot = F.topk_layout(n, k)
    payload = torch.zeros(tot, dtype=torch.uint8)
    payload[:off] = torch.tensor([5, 5, 9, 5, 43, 44, 43, 200],
                                 dtype=torch.uint8)
    # 1 + 2^-8 + 2^-16 style sums are order dependent in f32
    vals = torch.tensor([1.0, 2.0 ** -24, 4.0, 2.0 ** -24, 1.0, 2.0, 4.0, 8.0],
                        dtype=torch.bfloat16)
    payload[off:] = vals.view(torch.uint8)
    for acc in (False, True):
        d_cpu = torch.full((n,), 0.5)
        big = torch.full((8 + n + 64,), 0.5, device='cuda')
        F.unpack_topk(d_cpu, payload, k, accumulate=acc)
        F.unpack_topk(big[8:8 + n], payload.cuda(), k, accumulate=acc)
        assert _same_bits(big[8:8 + n], d_cpu)
        assert (big[:8] == 0.5).all() and (big[8 + n:] == 0.5).all()
        base = 0.5 if acc else 0.0
        assert d_cpu[256 + 43] == base + 5.0 and d_cpu[9] == base + 4.0
    # a tail block shorter than K: the pad entries point past n
    n, k = 8, 16
    x = torch.arange(1, n + 1, dtype=torch.float32)
    _, tot = F.topk_layout(n, k)
    payload = torch.zeros(tot, dtype=torch.uint8, device='cuda')
    res = torch.zeros(n, device='cuda')
    F.pack_topk_ef(payload, x.cuda(), res, k)
    assert payload[:k].tolist() == list(range(16)) and not res.any()
    big = torch.full((8 + n + 64,), 7.0, device='cuda')
    F.unpack_topk(big[8:8 + n], payload, k)
    assert torch.equal(big[8:8 + n].cpu(), x)
    assert (big[:8] == 7.0).all() and (big[8 + n:] == 7.0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_round_trip_on_the_device(dtype):
    """residual_after == c - unpack(pack(c)), bit for bit."""
    n = 4101
    xs, res = _inputs(n, dtype, seed_off=21)
    for k in KS:
        _, tot = F.topk_layout(n, k)
        r = res.cuda()
        for x in xs:
            x = x.cuda()
            c = x.float() + r
            payload = torch.zeros(tot, dtype=torch.uint8, device='cuda')
            F.pack_topk_ef(payload, x, r, k)
            dec = torch.empty(n, device='cuda')
            F.unpack_topk(dec, payload, k)
            assert torch.equal(r, c - dec)
            assert int((dec != 0).sum()) <= k * ((n + 255) // 256)


@pytest.mark.parametrize("k", KS)
def test_conservation_is_exact_on_integers_on_the_device(k):
    n, steps = 4101, 4
    g = torch.Generator().manual_seed(11)
    _, tot = F.topk_layout(n, k)
    res = torch.zeros(n, device='cuda')
    sum_dec = torch.zeros(n, device='cuda')
    sum_g = torch.zeros(n)
    for _ in range(steps):
        x = torch.randint(-7, 8, (n,), generator=g).float()
        payload = torch.zeros(tot, dtype=torch.uint8, device='cuda')
        F.pack_topk_ef(payload, x.cuda(), res, k)
        F.unpack_topk(sum_dec, payload, k, accumulate=True)
        sum_g += x
    assert torch.equal((sum_dec + res).cpu(), sum_g)
    assert res.any() and sum_dec.any()


def test_device_mismatch_is_an_error():
    n, k = 300, 16
    _, tot = F.topk_layout(n, k)
    x, res = torch.randn(n), torch.zeros(n)
    payload = torch.zeros(tot, dtype=torch.uint8)
    with pytest.raises(ValueError):
        F.pack_topk_ef(payload, x.cuda(), res, k)
    with pytest.raises(ValueError):
        F.pack_topk_ef(payload.cuda(), x, res, k)
    with pytest.raises(ValueError):
        F.pack_topk_ef(payload, x.cuda(), res.cuda(), k)
    with pytest.raises(ValueError):
        F.unpack_topk(res.cuda(), payload, k)
