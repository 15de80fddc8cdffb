"""GPU tests of the fused BatchNorm kernels (ops/kernels/batchnorm.hip)
against the float64 oracle and the derived bounds of tests/bn_utils.py,
through the raw entry points ps_bn_fwd / ps_bn_bwd as ops/modules.py calls
them. Every output is a slice of a NaN-filled buffer with guard bands
(0xA5 for the mask bytes); the inputs are compared with their originals
after the calls. On the lattice the kernel's sums are exact, so save_mean,
running_mean and dbeta are compared for equality with the float64 value
rounded once, everything else with its elementwise bound.

Coverage (R = 2048 / C rows per block pass; the reduce kernels take chunks
of 8 R rows on at most 1024 blocks, the row kernels chunks of 4 R rows on at
most 1024 blocks; "both reduce kernels" because every case runs forward and
backward):
- main loop of both reduce kernels, no tail: fold (2048, 2048);
- tail only: tail_lt_R (8, 5), (64, 1), (64, 31); tail of one row after
  full chunks: (64, 257), (2048, 9); tail of chunk - 1 rows: (64, 255),
  (2048, 7); main loop + tail with M no multiple of R: ragged, envelope;
- M < R (most row lanes idle): tail_lt_R; M = 1: (64, 1), also in
  test_momentum_and_running_stats (the M - 1 guard, var = 0);
- every C of the envelope 8 ... 2048: envelope;
- strided loop `b += 256` of both fold kernels: nb = 255, 256, 256, 258 in
  fold, nb = 1024 in capped;
- second grid pass of the two reduce kernels and of the two row kernels
  (normalize, dx), with exactly one partial grid position: capped
  (2048, 8203): 1026 chunks of 8 rows and 2051 of 4 on 1024 blocks;
  (512, 32803): 1026 chunks of 32 rows and 2051 of 16;
- template instantiations <T, RELU, RES / DRES>: each group holds the four
  (relu, res) combinations and runs in bf16 and f32
  (bn_utils.CASES, tests/test_bn_oracle.py checks the table);
- eval: test_eval_mode; ext_stats: test_ext_stats;
- "deterministic, no atomics": test_bit_identical_across_runs;
- the modules.py call and its channels_last handling:
  test_module_equals_raw_entry_points.
"""
import functools

import numpy as np
import pytest
import torch

import bn_utils as bu
import conv_lattice as cl
from ps_pytorch_amd.ops import current_stream_ptr, dtype_tag, require_lib
from ps_pytorch_amd.ops.modules import PsBatchNorm2d

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
NAN = float('nan')
MASK_FILL = 0xA5
PARTIAL_ROWS = 1024


def _tname(dtype):
    return 'bf16' if dtype == BF else 'f32'


def _dev(t, dtype):
    """float64 CPU lattice values -> the storage type on the GPU (exact)."""
    d = t.to(dtype)
    assert torch.equal(d.to(F64), t)
    return d.cuda()


def _bits(t):
    """Bit pattern, so that NaN == NaN in comparisons."""
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(
        torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(_bits(a), _bits(b)), f"{what}: bits differ"


class _Bufs:
    """Outputs carved from sentinel-filled buffers with guard bands."""

    def __init__(self):
        self.all = {}

    def new(self, name, n, dtype, init=None):
        fill = MASK_FILL if dtype == torch.uint8 else NAN
        whole = torch.full((n + 2 * cl.GUARD,), fill, dtype=dtype,
                           device='cuda')
        view = whole[cl.GUARD:cl.GUARD + n]
        if init is not None:
            view.copy_(init)
        self.all[name] = (whole, view)
        return view

    def collect(self):
        """Guard bands intact; the views as CPU tensors."""
        torch.cuda.synchronize()
        out = {}
        for name, (whole, view) in self.all.items():
            n = view.numel()
            for band in (whole[:cl.GUARD], whole[cl.GUARD + n:]):
                ok = ((band == MASK_FILL).all() if whole.dtype == torch.uint8
                      else torch.isnan(band).all())
                assert bool(ok), f"{name}: guard band written"
            out[name] = view.cpu()
        return out


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _run(x, res, dy, gam, beta, dtype, relu, rm0, rv0, momentum=bu.MOMENTUM,
         training=True, ext=None, backward=True):
    """One ps_bn_fwd (and ps_bn_bwd) on guarded buffers. Returns the CPU
    copies of every buffer; checks guard bands and that the inputs are
    unchanged. ext: [nblk, 2C] f32 partials handed in as ext_stats."""
    M, C = x.shape
    lib, tag, strm = require_lib(), dtype_tag(dtype), current_stream_ptr()
    ins = {'x': _dev(x, dtype), 'gamma': _dev(gam, dtype),
           'beta': _dev(beta, dtype)}
    if res is not None:
        ins['res'] = _dev(res, dtype)
    if backward:
        ins['dy'] = _dev(dy, dtype)
    if ext is not None:
        ins['ext'] = ext.to(F32).cuda()
    keep = {k: v.cpu() for k, v in ins.items()}
    b = _Bufs()
    y = b.new('y', M * C, dtype)
    ws = b.new('ws', 5 * C, F32)
    rm = b.new('running_mean', C, F32, rm0)
    rv = b.new('running_var', C, F32, rv0)
    mask = smean = sinv = partial = None
    if training:
        smean, sinv = b.new('save_mean', C, F32), b.new('save_invstd', C, F32)
        partial = b.new('partial', PARTIAL_ROWS * 2 * C, F32)
        if relu:
            mask = b.new('mask', M * C // 8, torch.uint8)
    lib.ps_bn_fwd(
        ins['x'].data_ptr(), y.data_ptr(), ins['gamma'].data_ptr(),
        ins['beta'].data_ptr(), rm.data_ptr(), rv.data_ptr(), _ptr(smean),
        _ptr(sinv), ws.data_ptr(), _ptr(partial), _ptr(ins.get('res')),
        _ptr(mask), _ptr(ins.get('ext')),
        ext.shape[0] if ext is not None else 0, M, C, float(momentum),
        bu.EPS, int(training), int(relu), tag, strm)
    if backward:
        # fresh ws / partial, as _FusedBNFn.backward allocates them
        ws2 = b.new('ws_bwd', 5 * C, F32)
        partial2 = b.new('partial_bwd', PARTIAL_ROWS * 2 * C, F32)
        dx = b.new('dx', M * C, dtype)
        dres = b.new('dres', M * C, dtype) if res is not None else None
        dgamma, dbeta = b.new('dgamma', C, dtype), b.new('dbeta', C, dtype)
        lib.ps_bn_bwd(
            ins['x'].data_ptr(), _ptr(mask), ins['dy'].data_ptr(),
            ins['gamma'].data_ptr(), smean.data_ptr(), sinv.data_ptr(),
            dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), _ptr(dres),
            ws2.data_ptr(), partial2.data_ptr(), M, C, int(relu), tag, strm)
    out = b.collect()
    for k, v in ins.items():
        _same_bits(v.cpu(), keep[k], f"input {k} changed")
    return out


def _ws_written_only(ws, C, lo, hi, what):
    w = ws.view(5, C)
    assert bool(torch.isnan(w[:lo]).all()) and bool(torch.isnan(w[hi:]).all()), \
        f"{what}: written outside [{lo}C, {hi}C)"
    assert not torch.isnan(w[lo:hi]).any(), f"{what}: [{lo}C, {hi}C) not written"
    return w.to(F64)


def _partial_rows(p, C, nb, what):
    p = p.view(PARTIAL_ROWS, 2 * C)
    assert bool(torch.isnan(p[nb:]).all()), f"{what}: rows >= {nb} written"
    assert not torch.isnan(p[:nb]).any(), f"{what}: rows < {nb} not written"
    return p[:nb].to(F64).sum(0)


def _check_fwd(got, x, gam, beta, res, o, fb, dtype, relu, rm0, rv0,
               momentum, tag, own_stats=True):
    """Training forward against the oracle. Returns the kernel's mask as
    [M, C] bool (None without relu)."""
    M, C = x.shape
    t, bf = _tname(dtype), dtype == BF
    bu.check_exact(got['save_mean'], bu.once(o['mean'], F32), f"{tag} save_mean")
    bu.check_within(got['save_invstd'], o['invstd'], fb['invstd'],
                    f"{tag} save_invstd", ('save_invstd', t))
    bu.check_within(got['y'], o['y'], bu.io_bound(fb['v'], o['y'], bf), f"{tag} y",
                    ('y', t))
    if bool((rm0 == 0).all()) and np.log2(momentum) % 1 == 0:
        bu.check_exact(got['running_mean'], bu.once(o['running_mean'], F32),
                       f"{tag} running_mean")
    bu.check_within(got['running_mean'], o['running_mean'],
                    fb['running_mean'], f"{tag} running_mean",
                    ('running_mean', t))
    bu.check_within(got['running_var'], o['running_var'], fb['running_var'],
                    f"{tag} running_var", ('running_var', t))
    w = _ws_written_only(got['ws'], C, 2, 4, f"{tag} ws")
    bu.check_within(w[2], o['scale'], fb['scale'], f"{tag} ws scale",
                    ('ws_scale', t))
    bu.check_within(w[3], o['shift'], fb['shift'], f"{tag} ws shift",
                    ('ws_shift', t))
    if own_stats:
        s = _partial_rows(got['partial'], C, bu.stats_blocks(M, C),
                          f"{tag} partial")
        bu.check_exact(s[:C], o['s1'], f"{tag} sum of partial sums")
        bu.check_exact(s[C:], o['s2'], f"{tag} sum of partial sums of squares")
    else:
        assert bool(torch.isnan(got['partial']).all()), \
            f"{tag}: partial written although ext_stats was given"
    if not relu:
        assert 'mask' not in got
        return None
    kmask = bu.unpack_mask(got['mask'], M, C)
    und = bu.undecided(o, fb)
    assert float(und.double().mean()) <= 1e-3
    bad = (kmask != o['mask']) & ~und
    assert not bad.any(), f"{tag} mask: {int(bad.sum())} decided bits wrong"
    return kmask


def _check_bwd(got, x, dy, gam, o, fb, kmask, dtype, has_res, tag):
    M, C = x.shape
    t, bf = _tname(dtype), dtype == BF
    r = bu.ref_bwd(x, dy, gam, o['mean'], o['invstd'], kmask)
    bb = bu.bwd_bounds(gam, o, fb, r, bf)
    bu.check_exact(got['dbeta'], bu.once(r['dbeta'], dtype), f"{tag} dbeta")
    bu.check_within(got['dgamma'], r['dgamma'], bb['dgamma'], f"{tag} dgamma",
                    ('dgamma', t))
    bu.check_within(got['dx'], r['dx'], bb['dx'], f"{tag} dx", ('dx', t))
    if has_res:
        bu.check_exact(got['dres'], r['dres'], f"{tag} dres")
    else:
        assert 'dres' not in got
    s = _partial_rows(got['partial_bwd'], C, bu.stats_blocks(M, C),
                      f"{tag} partial_bwd")
    bu.check_exact(s[:C], r['dbeta'], f"{tag} sum of partial sum(dy_eff)")
    bu.check_within(s[C:], r['dgamma'], bb['dgamma_f32'],
                    f"{tag} sum of partial sum(dy_eff xhat)")
    w = _ws_written_only(got['ws_bwd'], C, 2, 5, f"{tag} ws_bwd")
    bu.check_within(w[2], o['scale'], fb['scale'], f"{tag} ws a", ('ws_a', t))
    bu.check_within(w[3], -o['scale'] * o['invstd'] * r['dgamma'] / M,
                    bb['b'], f"{tag} ws b", ('ws_b', t))
    bu.check_within(w[4], -o['scale'] * r['dbeta'] / M, bb['c'],
                    f"{tag} ws c", ('ws_c', t))


@functools.lru_cache(maxsize=1)
def _table_ref(case):
    """Forward reference and f32 bounds of one table row, shared by the two
    types (gamma and beta are the same numbers in both)."""
    _, C, M, relu, _ = case
    x, res, dy, gam, beta = bu.bn_case(case)
    rm0, rv0 = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    o = bu.ref_fwd(x, gam, beta, res, bool(relu), rm0, rv0)
    return o, bu.fwd_bounds(x, gam, beta, res, o, rm0, rv0), rm0, rv0


@DTYPES
@pytest.mark.parametrize("case", bu.CASES, ids=bu.CASE_IDS)
def test_case_table(case, dtype):
    _, C, M, relu, _ = case
    x, res, dy, gam, beta = bu.bn_case(case)
    o, fb, rm0, rv0 = _table_ref(case)
    got = _run(x, res, dy, gam, beta, dtype, relu, rm0, rv0)
    tag = f"{case} {_tname(dtype)}"
    kmask = _check_fwd(got, x, gam, beta, res, o, fb, dtype, relu, rm0, rv0,
                       bu.MOMENTUM, tag)
    _check_bwd(got, x, dy, gam, o, fb, kmask, dtype, res is not None, tag)


def _stats(C, tag):
    """Running statistics that are neither 0 nor 1 (f32 values)."""
    gen = bu._gen('bn_running', C, tag)
    rm = (torch.rand(C, generator=gen) * 2 - 1).to(F64)
    rv = (torch.rand(C, generator=gen) * 1.5 + 0.25).to(F64)
    return rm, rv


@DTYPES
@pytest.mark.parametrize("relu,with_res", bu.RR)
@pytest.mark.parametrize("case", [bu.TAIL_CASE, bu.RAGGED_CASE],
                         ids=["tail", "blocks"])
def test_eval_mode(case, relu, with_res, dtype):
    """Null smean / sinvstd / partial / mask as _bn_eval_fused passes them:
    nothing can be written through them, and nothing but y and ws[2C, 4C)
    is written at all."""
    _, C, M, _, _ = case
    gen = bu._gen('bn_eval', case)
    x, res = bu.lattice((M, C), gen), bu.lattice((M, C), gen)
    res = res if with_res else None
    gam, beta = bu.params(C, gen)
    rm, rv = _stats(C, 'eval')
    o = bu.ref_fwd(x, gam, beta, res, bool(relu), rm, rv, training=False)
    fb = bu.fwd_bounds(x, gam, beta, res, o, training=False)
    got = _run(x, res, None, gam, beta, dtype, relu, rm, rv, training=False,
               backward=False)
    t, tag = _tname(dtype), f"eval {case} {_tname(dtype)}"
    assert set(got) == {'y', 'ws', 'running_mean', 'running_var'}
    bu.check_within(got['y'], o['y'], bu.io_bound(fb['v'], o['y'], dtype == BF),
                    f"{tag} y", ('eval_y', t))
    _same_bits(got['running_mean'], rm.float(), f"{tag} running_mean")
    _same_bits(got['running_var'], rv.float(), f"{tag} running_var")
    w = _ws_written_only(got['ws'], C, 2, 4, f"{tag} ws")
    bu.check_within(w[2], o['scale'], fb['scale'], f"{tag} ws scale")
    bu.check_within(w[3], o['shift'], fb['shift'], f"{tag} ws shift")


@DTYPES
@pytest.mark.parametrize("nblk", [1, 255, 300])
def test_ext_stats(nblk, dtype):
    """Partials handed in by a producer: [nblk][2C] slice sums of ANOTHER
    tensor xs. Mean, invstd and y follow xs; the kernel's own partial
    buffer is not touched. C = 64, M = 600: 2.3 chunks of 256 rows."""
    C, M = 64, 600
    gen = bu._gen('bn_ext', nblk)
    x, xs, res, dy = (bu.lattice((M, C), gen) for _ in range(4))
    xs = xs * 0.5 + 1.0                      # other mean, other variance
    bu.assert_lattice_exact(xs, 0.125, 'ext xs')
    gam, beta = bu.params(C, gen)
    ext = torch.stack([torch.cat([s.sum(0), (s * s).sum(0)])
                       for s in torch.tensor_split(xs, nblk)])
    assert ext.shape == (nblk, 2 * C)
    assert torch.equal(ext.float().to(F64), ext)
    rm0, rv0 = _stats(C, 'ext')
    o = bu.ref_fwd(x, gam, beta, res, True, rm0, rv0, stats_x=xs)
    fb = bu.fwd_bounds(x, gam, beta, res, o, rm0, rv0)
    assert float((o['mean'] - x.mean(0)).abs().min()) > 0.5
    got = _run(x, res, dy, gam, beta, dtype, 1, rm0, rv0, ext=ext)
    tag = f"ext_stats {nblk} {_tname(dtype)}"
    kmask = _check_fwd(got, x, gam, beta, res, o, fb, dtype, 1, rm0, rv0,
                       bu.MOMENTUM, tag, own_stats=False)
    # the backward normalizes x with the saved statistics, whatever they are
    _check_bwd(got, x, dy, gam, o, fb, kmask, dtype, True, tag)


@DTYPES
@pytest.mark.parametrize("C,M", [(64, 31), (64, 1), (128, 1000)])
def test_momentum_and_running_stats(C, M, dtype):
    """Two successive forwards, momentum 0.1 then 1.0, from running
    statistics that are not the initial ones. The second step starts from
    what the kernel left after the first. At M = 1 the unbiased factor is
    M / max(M - 1, 1) = 1 and var = 0."""
    gen = bu._gen('bn_momentum', C, M)
    x, res = bu.lattice((M, C), gen), bu.lattice((M, C), gen)
    gam, beta = bu.params(C, gen)
    rm, rv = _stats(C, 'momentum')
    t = _tname(dtype)
    for step, mom in enumerate((float(np.float32(0.1)), 1.0)):
        o = bu.ref_fwd(x, gam, beta, res, True, rm, rv, momentum=mom)
        fb = bu.fwd_bounds(x, gam, beta, res, o, rm, rv, momentum=mom)
        got = _run(x, res, None, gam, beta, dtype, 1, rm, rv, momentum=mom,
                   backward=False)
        tag = f"momentum {mom:g} C{C} M{M} {t}"
        _check_fwd(got, x, gam, beta, res, o, fb, dtype, 1, rm, rv, mom, tag)
        if mom == 1.0:
            bu.check_exact(got['running_mean'], bu.once(o['mean'], F32),
                           f"{tag} running_mean")
        if M == 1:
            # x^2, mean = x and mean * mean are exact on the lattice, so the
            # kernel's var is 0 as well: one invstd for all channels, and
            # momentum 1 leaves running_var = 0
            assert float(o['var'].abs().max()) == 0.0
            assert bool((got['save_invstd'] == got['save_invstd'][0]).all())
            if mom == 1.0:
                bu.check_exact(got['running_var'], o['running_var'],
                               f"{tag} running_var")
        rm, rv = got['running_mean'].to(F64), got['running_var'].to(F64)


@DTYPES
def test_offset_mean(dtype):
    """|mean| >> std: what var = E[x^2] - mean^2 and x * scale + shift cost.
    The bounds carry the cancellation terms (bn_utils); the figures printed
    here are recorded in profiles/r15_bn_oracle.md."""
    bf = dtype == BF
    x, res, dy, gam, beta = bu.offset_case(bf)
    M, C = x.shape
    rm0, rv0 = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    o = bu.ref_fwd(x, gam, beta, res, True, rm0, rv0)
    fb = bu.fwd_bounds(x, gam, beta, res, o, rm0, rv0)
    got = _run(x, res, dy, gam, beta, dtype, 1, rm0, rv0)
    t, tag = _tname(dtype), f"offset {_tname(dtype)}"
    y, inv = got['y'].to(F64).view(M, C), got['save_invstd'].to(F64)
    uio = bu.UB if bf else bu.U
    for name, cols in (('offset64', slice(0, 4)), ('const', slice(4, 5)),
                       ('mean2_std1', slice(5, 6)), ('plain', slice(6, 8))):
        e_inv = (inv - o['invstd'])[cols].abs()
        e_y = (y - o['y'])[:, cols].abs()
        nz = o['y'][:, cols].abs() > 0
        rel = (e_y[nz] / (uio * o['y'][:, cols].abs()[nz])).max() if nz.any() else 0
        fig = {
            'invstd_err_over_bound': float((e_inv / fb['invstd'][cols]).max()),
            'invstd_rel_err_over_u': float((e_inv / o['invstd'][cols]).max() / bu.U),
            'y_err_over_bound': float((e_y / bu.io_bound(fb['v'], o['y'], bf)[:, cols]).max()),
            'y_err_over_u_y': float(rel),
            'y_bound_over_u_y': float((bu.io_bound(fb['v'], o['y'], bf)[:, cols][nz]
                                       / (uio * o['y'][:, cols].abs()[nz])).max()),
        }
        for k, v in fig.items():
            bu.RATIOS[(f"{name}.{k}", t)] = v
        print(tag, name, fig)
    kmask = _check_fwd(got, x, gam, beta, res, o, fb, dtype, 1, rm0, rv0,
                       bu.MOMENTUM, tag)
    _check_bwd(got, x, dy, gam, o, fb, kmask, dtype, True, tag)


@DTYPES
@pytest.mark.parametrize("case", [('tail_edge', 64, 257, 1, 1),
                                  bu.CAPPED_CASE], ids=["tail", "capped"])
def test_bit_identical_across_runs(case, dtype):
    _, C, M, relu, _ = case
    x, res, dy, gam, beta = bu.bn_case(case)
    rm0, rv0 = _stats(C, 'det')
    a = _run(x, res, dy, gam, beta, dtype, relu, rm0, rv0)
    b = _run(x, res, dy, gam, beta, dtype, relu, rm0, rv0)
    assert set(a) == set(b)
    for k in a:
        _same_bits(a[k], b[k], f"{case} {k}")


def _factor(M):
    """M = N * H * W with H * W > 1 where M allows it."""
    for hw in (49, 25, 13, 10, 7, 5, 3, 2):
        if M % hw == 0:
            return M // hw, hw, 1
    return 1, M, 1


@DTYPES
@pytest.mark.parametrize("case", [bu.TAIL_CASE, bu.RAGGED_CASE,
                                  bu.CAPPED_CASE],
                         ids=["tail", "ragged", "capped"])
def test_module_equals_raw_entry_points(case, dtype):
    """PsBatchNorm2d forward + backward on NCHW inputs that are contiguous
    in no layout: bit for bit what the raw entry points give on the same
    rows, so the oracle's verdict on test_case_table covers the module."""
    _, C, M, relu, _ = case
    x, res, dy, gam, beta = bu.bn_case(case)
    rm0, rv0 = _stats(C, 'module')
    raw = _run(x, res, dy, gam, beta, dtype, relu, rm0, rv0,
               momentum=float(np.float32(0.1)))
    N, H, W = _factor(M)

    def nchw(t):
        """[M, C] rows as an N, C, H, W slice of a wider NCHW buffer."""
        wide = torch.zeros(N, C, H, W + 1, dtype=dtype, device='cuda')
        v = wide[..., :W]
        v.copy_(t.to(dtype).view(N, H, W, C).permute(0, 3, 1, 2))
        assert not v.is_contiguous()
        assert not v.is_contiguous(memory_format=torch.channels_last)
        return v

    def rows(t):
        return t.permute(0, 2, 3, 1).reshape(M, C).contiguous().cpu().view(-1)

    m = PsBatchNorm2d(C, eps=bu.EPS, momentum=float(np.float32(0.1)),
                      relu=bool(relu)).to('cuda', dtype)
    m._ensure_f32_stats()
    with torch.no_grad():
        m.weight.copy_(gam)
        m.bias.copy_(beta)
        m.running_mean.copy_(rm0)
        m.running_var.copy_(rv0)
    xm = nchw(x).requires_grad_(True)
    rmod = nchw(res).requires_grad_(True) if res is not None else None
    y = m(xm, residual=rmod)
    y.backward(nchw(dy))
    torch.cuda.synchronize()
    tag = f"module {case} {_tname(dtype)}"
    _same_bits(rows(y.detach()), raw['y'], f"{tag} y")
    _same_bits(rows(xm.grad), raw['dx'], f"{tag} dx")
    if res is not None:
        _same_bits(rows(rmod.grad), raw['dres'], f"{tag} dres")
    _same_bits(m.weight.grad.cpu(), raw['dgamma'], f"{tag} dgamma")
    _same_bits(m.bias.grad.cpu(), raw['dbeta'], f"{tag} dbeta")
    _same_bits(m.running_mean.cpu(), raw['running_mean'], f"{tag} running_mean")
    _same_bits(m.running_var.cpu(), raw['running_var'], f"{tag} running_var")
