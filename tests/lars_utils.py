"""Shared helpers of the LARS tests: a synthetic segment list independent of
any model, laid out by FlatSpace's ALIGN=8 rule, and input draws."""
import numpy as np
import torch

from ps_pytorch_amd.ops.functional import LARS_CHUNK

ALIGN = 8
# (numel, ndim): one element, the three sizes around the alignment, the
# three around a chunk, two chunks and a tail, and one of 2^17; 1-D and
# >= 2-D mixed so both kinds sit on both sides of gaps and chunk boundaries
SEG_SPEC = [(1, 2), (7, 1), (8, 4), (9, 2), (LARS_CHUNK - 1, 1),
            (LARS_CHUNK, 2), (LARS_CHUNK + 1, 4), (2 * LARS_CHUNK + 3, 2),
            (1 << 17, 2), (5, 1)]


def synthetic_segments(spec=SEG_SPEC):
    """([(offset, numel, ndim)], padded total) by FlatSpace's layout rule."""
    segs, total = [], 0
    for n, d in spec:
        total = (total + ALIGN - 1) & ~(ALIGN - 1)
        segs.append((total, n, d))
        total += n
    return segs, (total + ALIGN - 1) & ~(ALIGN - 1)


def synthetic_buckets(segs, total, per_bucket=3):
    """Regions of `per_bucket` whole segments each, covering [0, total)."""
    starts = [segs[i][0] for i in range(0, len(segs), per_bucket)]
    return list(zip(starts, starts[1:] + [total]))


def own_mask(segs, total) -> torch.Tensor:
    """True on the parameters' own elements, False in the alignment gaps."""
    mask = torch.zeros(total, dtype=torch.bool)
    for off, n, _ in segs:
        mask[off:off + n] = True
    return mask


def lattice(n: int, seed: int) -> torch.Tensor:
    """f32 draws from {k/8 : |k| <= 8}: exact in bf16, squares multiples of
    2^-6, so a 2^17-element sum of squares is exact in any order."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (n,), generator=g).to(torch.float32) / 8.0


def f32_bits(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def f64_bits(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, dtype=np.float64).view(np.int64)
