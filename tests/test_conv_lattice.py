"""CPU half of the exact-integer oracle (tests/conv_lattice.py): the case
tables reach every dispatch branch of conv.hip the mirrors can name, every
reference stays in the range where bf16 is exact, and the float64 torch
reference agrees with plain int64 loops. The GPU half is
test_conv_lattice_gpu.py."""
import pytest
import torch

import conv_lattice as cl


def _names(fn, cases):
    return {fn(*c) for c in cases}


def test_tables_cover_every_fwd_branch():
    uni = cl.branch_universe()[0]
    hit = _names(cl.fwd_branch, cl.FWD_CASES + cl.FWD_RAW_ONLY)
    print(f"fwd: {len(hit)} of {len(uni)} branch names")
    assert uni - hit == set(), sorted(uni - hit)
    assert hit <= uni, sorted(hit - uni)    # the sweep is wide enough
    # c4_nb1/c4_nb2/c8: TN x stride; small_nb1/nb2: stride; 1x1: stride x
    # aligned; gen: TN x stride x aligned; two halo widths
    assert len(uni) == 4 + 4 + 4 + 2 + 2 + 4 + 12 + 2


def test_tables_cover_every_dgrad_branch():
    uni = cl.branch_universe()[1]
    hit = _names(cl.dgrad_branch, cl.DGRAD_CASES + cl.DGRAD_RAW_ONLY)
    print(f"dgrad: {len(hit)} of {len(uni)} branch names")
    assert uni - hit == set(), sorted(uni - hit)
    assert hit <= uni, sorted(hit - uni)
    # s1: 3 TN x aligned x carry; s2: 2 TN x aligned x carry x seed/full;
    # halo: 2 widths x carry
    assert len(uni) == 12 + 16 + 4


def test_tables_cover_every_wgrad_branch():
    uni = cl.branch_universe()[2]
    hit = _names(cl.wgrad_branch, cl.WGRAD_CASES + cl.WGRAD_RAW_ONLY)
    print(f"wgrad: {len(hit)} of {len(uni)} branch names")
    assert uni - hit == set(), sorted(uni - hit)
    assert hit <= uni, sorted(hit - uni)
    # small: 3 CPM x stride x pw/magic; two row kernels; gen: 2 TK x stride
    # x pw/magic x aligned
    assert len(uni) == 12 + 2 + 16


def test_raw_only_rows_are_not_reachable_from_the_modules():
    """The separate tables hold what PsConv2d / _ConvFn.backward pad away:
    C <= 3 or ragged C < 64 with R > 1, or K % 8 != 0 in a backward."""
    for c in cl.FWD_RAW_ONLY:
        assert c[5] > 1 and c[1] < 64 and (c[1] <= 3 or c[1] % 8), c
    for c in cl.DGRAD_RAW_ONLY + cl.WGRAD_RAW_ONLY:
        ragged_c = c[5] > 1 and c[1] < 64 and (c[1] <= 3 or c[1] % 8)
        assert ragged_c or c[4] % 8, c


def test_tables_have_no_duplicates_and_are_supported():
    for tab in (cl.FWD_CASES + cl.FWD_RAW_ONLY,
                cl.DGRAD_CASES + cl.DGRAD_RAW_ONLY,
                cl.WGRAD_CASES + cl.WGRAD_RAW_ONLY):
        assert len(set(tab)) == len(tab)
        for c in tab:
            assert cl.supported(*c[:8]), c


def test_wgrad_split_within_kernel_contract():
    """Every slab of the split-K wgrad holds at least one 64-pixel chunk."""
    for c in cl.WGRAD_CASES + cl.WGRAD_RAW_ONLY:
        assert 1 <= c[8] <= max(1, cl.wgrad_len(c) // 64), c


def _worst(refs):
    return max(float(r.abs().max()) for r in refs)


def test_fwd_range_condition():
    worst = 0.0
    for c in cl.FWD_CASES + cl.FWD_RAW_ONLY:
        m = float(cl.fwd_case(c)[3].abs().max())
        assert m <= cl.RANGE, (c, m)
        worst = max(worst, m)
    print(f"fwd worst max|ref| = {worst:g}")


def test_dgrad_range_condition():
    worst = 0.0
    for c in cl.DGRAD_CASES + cl.DGRAD_RAW_ONLY:
        m = float(cl.dgrad_case(c)[3].abs().max())
        assert m <= cl.RANGE, (c, m)
        worst = max(worst, m)
    print(f"dgrad worst max|ref| = {worst:g}")


def test_wgrad_range_condition():
    worst = 0.0
    for c in cl.WGRAD_CASES + cl.WGRAD_RAW_ONLY:
        m = float(cl.wgrad_case(c)[2].abs().max())
        assert m <= cl.RANGE, (c, m)
        worst = max(worst, m)
    print(f"wgrad worst max|ref| = {worst:g}")


def test_bias_grad_range_condition():
    worst = 0.0
    for c in cl.BIAS_CASES:
        m = float(cl.bias_case(c)[1].abs().max())
        print(f"bias-grad {c} max|ref| = {m:g}")
        assert m <= cl.RANGE, (c, m)
        worst = max(worst, m)
    print(f"bias-grad worst max|ref| = {worst:g}")


def test_e2e_range_condition():
    for c in cl.E2E_CONV:
        for name, t in zip(('out', 'dx', 'dw', 'db'), cl.e2e_conv_case(c)[4:]):
            m = float(t.abs().max())
            print(f"{c[0]} {name} max|ref| = {m:g}")
            assert m <= cl.RANGE, (c, name, m)
    for c in cl.E2E_LINEAR:
        for name, t in zip(('out', 'dx', 'dw', 'db'),
                           cl.e2e_linear_case(c)[4:]):
            m = float(t.abs().max())
            print(f"linear {c} {name} max|ref| = {m:g}")
            assert m <= cl.RANGE, (c, name, m)


def test_references_are_integers():
    """float64 holds every sum exactly, so each reference is integral."""
    for c in cl.FWD_CASES[:4] + cl.FWD_RAW_ONLY[:2]:
        r = cl.fwd_case(c)[3]
        assert torch.equal(r, r.round())
    for c in cl.DGRAD_CASES[:4]:
        r = cl.dgrad_case(c)[3]
        assert torch.equal(r, r.round())
    for c in cl.WGRAD_CASES[:4]:
        r = cl.wgrad_case(c)[2]
        assert torch.equal(r, r.round())


# (Nb, C, H, W, K, R, stride, pad): tiny, one of them stride 2 with padding
NAIVE_CASES = [(2, 3, 5, 4, 2, 3, 1, 0), (1, 2, 6, 5, 3, 3, 2, 1)]


@pytest.mark.parametrize("case", NAIVE_CASES)
def test_reference_equals_naive_int64_loops(case):
    """The float64 torch routines the oracle uses against nested int64
    loops, so the oracle does not rest on one torch routine."""
    Nb, C, H, W, K, R, stride, pad = case
    x, w, b, out = cl.fwd_case(case)
    dy, w2, cy, dx = cl.dgrad_case(case + (1,))
    x3, dy3, dw = cl.wgrad_case(case + (1,))
    n_out, _, _ = cl.naive_conv_int64(x, w, b, dy, stride, pad)
    assert torch.equal(out, n_out.double())
    _, n_dx, _ = cl.naive_conv_int64(x, w2, b, dy, stride, pad)
    assert torch.equal(dx, n_dx.double() + cy)
    _, _, n_dw = cl.naive_conv_int64(x3, w, b, dy3, stride, pad)
    assert torch.equal(dw, n_dw.double())


def test_amps_rule():
    assert cl.amps(36) == (3, 3)
    assert cl.amps(87) == (3, 3)        # 6 * sqrt(16 * 87) = 223.9
    assert cl.amps(88) == (2, 2)
    assert cl.amps(348) == (2, 2)
    assert cl.amps(349) == (2, 1)
    assert cl.amps(1045) == (2, 1)
    assert cl.amps(1046) == (1, 1)
    assert cl.amps(3000) == (1, 1)


def test_seed_is_stable_across_processes():
    """crc32 of the case's repr, not hash(): the same draw everywhere."""
    import zlib
    c = cl.FWD_CASES[0]
    assert cl.gen('fwd', c).initial_seed() == \
        zlib.crc32(repr(('fwd',) + c).encode())
