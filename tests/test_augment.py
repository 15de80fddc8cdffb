"""Fused Philox augmentation loader on the CPU: the draw oracle's statistics
and purity, augment_ref against a per-sample F.pad construction, the
rng='philox' loader mode, and the --loader flag / ValueError guards."""
import pytest
import torch

from augment_utils import (SEED, SHAPES, STREAM, bits, fake_dataset,
                           fake_indices, norm_consts, per_sample_ref,
                           write_cifar10)
from ps_pytorch_amd.config import JobConfig, parse_args
from ps_pytorch_amd.data import (RealDataset, RealResidentLoader,
                                 prepare_data)
from ps_pytorch_amd.ops.augment import augment_batch
from ps_pytorch_amd.ops.functional import augment_draws, augment_ref


# ---- draws ----

def test_draw_statistics():
    """9000 samples: each of the 9 offsets 1000 +- 149 times per axis (5
    sigma, sigma = sqrt(9000 * 8/81)), 4500 +- 237 flips (5 sigma, sigma =
    sqrt(9000/4)), all 162 (oy, ox, flip) combinations."""
    oy, ox, fl = (torch.cat(t) for t in zip(*[
        augment_draws(1000, 4, True, SEED, STREAM, step)
        for step in range(9)]))
    cy = torch.bincount(oy, minlength=9)
    cx = torch.bincount(ox, minlength=9)
    print("oy counts", cy.tolist(), "ox counts", cx.tolist(),
          "flips", int(fl.sum()))
    assert cy.numel() == 9 and cx.numel() == 9
    assert int(oy.min()) >= 0 and int(ox.min()) >= 0
    for c in cy.tolist() + cx.tolist():
        assert abs(c - 1000) <= 149, (cy.tolist(), cx.tolist())
    assert abs(int(fl.sum()) - 4500) <= 237
    combos = set(zip(oy.tolist(), ox.tolist(), fl.tolist()))
    assert len(combos) == 162


def test_draws_are_a_pure_function():
    base = augment_draws(64, 4, True, SEED, STREAM, 5)
    again = augment_draws(64, 4, True, SEED, STREAM, 5)
    assert all(torch.equal(a, b) for a, b in zip(base, again))
    for other in (augment_draws(64, 4, True, SEED, STREAM, 6),
                  augment_draws(64, 4, True, SEED, STREAM + 1, 5),
                  augment_draws(64, 4, True, SEED + 1, STREAM, 5)):
        assert not all(torch.equal(a, b) for a, b in zip(base, other))
    # a prefix of a larger batch: slot b does not depend on B
    big = augment_draws(100, 4, True, SEED, STREAM, 5)
    assert all(torch.equal(a, b[:64]) for a, b in zip(base, big))
    # no hflip: never flipped; pad 0: offsets 0
    oy, ox, fl = augment_draws(64, 0, False, SEED, STREAM, 5)
    assert not oy.any() and not ox.any() and not fl.any()


def test_batch_of_37_covers_offsets_and_flips():
    oy, ox, fl = augment_draws(37, 4, True, SEED, STREAM, 0)
    assert sorted(set(oy.tolist())) == list(range(9))
    assert sorted(set(ox.tolist())) == list(range(9))
    assert int(fl.sum()) == 20


# ---- augment_ref against the per-sample construction ----

def _cases():
    for C, H, W, p in SHAPES:
        if p:
            for mode in ('reflect', 'constant'):
                for hflip in (True, False):
                    yield C, H, W, p, mode, hflip
        else:
            yield C, H, W, 0, None, True
            yield C, H, W, 0, None, False


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('C,H,W,p,mode,hflip', list(_cases()))
def test_augment_ref_matches_per_sample(C, H, W, p, mode, hflip, dtype):
    x, y = fake_dataset(C, H, W)
    idx = fake_indices(37)
    mean, inv = norm_consts(C)
    draws = (augment_draws(37, p, hflip, SEED, STREAM, 0)
             if p or hflip else None)
    got, got_y = augment_ref(x, y, idx, mean, inv, p, mode, hflip, draws,
                             dtype)
    want, want_y = per_sample_ref(x, y, idx, mean, inv, p, mode, draws,
                                  dtype)
    assert got.shape == (37, C, H, W) and got.dtype == dtype
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(got_y, want_y)
    # the CPU wrapper is the oracle
    via, via_y = augment_batch(x, y, idx, mean, inv, pad=p, pad_mode=mode,
                               hflip=hflip, seed=SEED, stream=STREAM, step=0,
                               dtype=dtype)
    assert torch.equal(bits(via), bits(want)) and torch.equal(via_y, want_y)


def test_normalize_formula_all_bytes():
    """The kernel's formula on ds.mean / ds.inv_std values reproduces the
    torch loader's normalize for every byte value."""
    for C in (1, 3):
        mean, inv = norm_consts(C)
        x = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16)
        x = x.expand(1, C, 16, 16).contiguous()
        y = torch.zeros(1, dtype=torch.int64)
        m = torch.tensor(mean).view(1, C, 1, 1)
        s = torch.tensor(inv).view(1, C, 1, 1)
        for dtype in (torch.float32, torch.bfloat16):
            got, _ = augment_ref(x, y, torch.zeros(1, dtype=torch.int64),
                                 mean, inv, dtype=dtype)
            want = ((x.float() - m) * s).to(dtype)
            assert torch.equal(bits(got), bits(want))


# ---- loader ----

@pytest.fixture(scope='module')
def cifar_root(tmp_path_factory):
    return write_cifar10(str(tmp_path_factory.mktemp('aug') / 'cifar10_data'),
                         n_train=100, n_test=20)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_philox_loader_without_augment_equals_torch_loader(cifar_root, dtype):
    for split, shuffle in (('train', True), ('test', False)):
        ds = RealDataset('Cifar10', split, cifar_root, dtype=dtype)
        kw = dict(batch_size=16, shuffle=shuffle, seed=5, drop_last=False,
                  augment=False)
        a = RealResidentLoader(ds, rng='torch', **kw)
        b = RealResidentLoader(ds, rng='philox', **kw)
        n = 0
        for (xa, ya), (xb, yb) in zip(a, b):
            assert xb.dtype == dtype and xa.shape == xb.shape
            assert torch.equal(bits(xa), bits(xb))
            assert torch.equal(ya, yb)
            n += 1
        assert n == len(a) == len(b)
        assert b.host_step == 0 and b.step is None     # no RNG used


def test_philox_loader_augmented(cifar_root):
    ds = RealDataset('Cifar10', 'train', cifar_root)
    mk = lambda **kw: RealResidentLoader(ds, batch_size=32, seed=9,
                                         rng='philox', **kw)
    a, b, c = mk(), mk(), mk(stream=1)
    first_perm = a._perm.clone()
    seen = []
    for k in range(4):                       # 3 batches per epoch: wraps
        pos = k % 3
        xa, ya = a.next_batch()
        xb, yb = b.next_batch()
        xc, _ = c.next_batch()
        idx = a._perm[pos * 32:(pos + 1) * 32]
        assert xa.shape == (32, 3, 32, 32)
        assert xa.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(bits(xa), bits(xb)) and torch.equal(ya, yb)
        assert not torch.equal(xa, xc)
        assert torch.equal(ya, ds.y[idx])
        want, _ = augment_ref(ds.x_u8, ds.y, idx, a._mean255, a._inv_std255,
                              ds.pad, ds.pad_mode, ds.hflip,
                              augment_draws(32, ds.pad, ds.hflip, 9, 0, k),
                              torch.float32)
        assert torch.equal(bits(xa), bits(want))
        seen.append(xa)
    assert a.host_step == 4
    assert a._epoch == 1 and not torch.equal(a._perm, first_perm)
    assert not torch.equal(seen[0], seen[3])
    # both modes visit the same indices in the same order
    t = RealResidentLoader(ds, batch_size=32, seed=9)
    assert torch.equal(t._perm, first_perm)


def test_loader_rejects_unknown_rng(cifar_root):
    ds = RealDataset('Cifar10', 'train', cifar_root)
    with pytest.raises(ValueError):
        RealResidentLoader(ds, batch_size=8, rng='mt19937')


# ---- flag and validation ----

def test_loader_flag():
    assert JobConfig().loader == 'torch'
    assert parse_args([]).loader == 'torch'
    args = parse_args(['--loader', 'fused'])
    assert JobConfig.from_args(args).loader == 'fused'
    with pytest.raises(ValueError):
        JobConfig(loader='bogus')


def test_prepare_data_fused(cifar_root):
    cfg = JobConfig(dataset='Cifar10', batch_size=8, data_dir=cifar_root,
                    loader='fused', seed=4)
    tr, te = prepare_data(cfg, rank=2)
    assert isinstance(tr, RealResidentLoader) and tr.rng == 'philox'
    assert tr.stream == 2 and tr.seed == 4 and te.rng == 'philox'
    x, y = tr.next_batch()
    assert x.shape == (8, 3, 32, 32) and y.shape == (8,)
    xt, _ = te.next_batch()
    assert xt.shape == (20, 3, 32, 32) and te.host_step == 0
    # default stays the torch loader
    tr0, _ = prepare_data(JobConfig(dataset='Cifar10', batch_size=8,
                                    data_dir=cifar_root))
    assert tr0.rng == 'torch'


def test_value_error_guards():
    x, y = fake_dataset(3, 5, 7)
    idx = fake_indices(4)
    mean, inv = norm_consts(3)
    ok = dict(pad=4, pad_mode='reflect', hflip=True, seed=1, step=0)
    augment_batch(x, y, idx, mean, inv, **ok)
    bad = [
        (torch.zeros(2, 5, 4, 4, dtype=torch.uint8), torch.zeros(
            2, dtype=torch.int64), idx[:1] * 0, [0.] * 5, [1.] * 5, {}),
        (x.float(), y, idx, mean, inv, ok),                     # x dtype
        (x, y.int(), idx, mean, inv, ok),                       # y dtype
        (x, y, idx.int(), mean, inv, ok),                       # idx dtype
        (x, y, idx, mean, inv, dict(ok, dtype=torch.float16)),  # out dtype
        (x, y, idx, mean, inv, dict(ok, pad=5)),                # p > H-1
        (x, y, idx, mean, inv, dict(ok, pad_mode='edge')),
        (x, y, idx, mean[:2], inv, ok),
        (x.permute(0, 1, 3, 2), y, idx, mean, inv, ok),         # not NCHW
    ]
    for xx, yy, ii, mm, ss, kw in bad:
        with pytest.raises(ValueError):
            augment_batch(xx, yy, ii, mm, ss, **kw)
    # constant padding has no such limit on the pad
    augment_batch(x, y, idx, mean, inv, **dict(ok, pad=6,
                                               pad_mode='constant'))
    # H, W < 65536 (checked before anything is read)
    wide = torch.zeros(1, 1, 1, 65536, dtype=torch.uint8)
    with pytest.raises(ValueError):
        augment_batch(wide, torch.zeros(1, dtype=torch.int64),
                      torch.zeros(1, dtype=torch.int64), [0.], [1.])
