"""Shared pieces of the fused-loader tests (test_augment.py,
test_augment_gpu.py): seeds, shapes, a fake dataset, a fake CIFAR-10 tree of
any size, and the per-sample F.pad construction the oracle is checked
against."""
import functools
import os
import pickle

import numpy as np
import torch
import torch.nn.functional as F

SEED = 20240611
STREAM = 3

# (C, H, W, pad): the largest legal reflect pad on the smallest image, the
# MNIST shape without padding, the CIFAR shape
SHAPES = [(3, 5, 7, 4), (1, 28, 28, 0), (3, 32, 32, 4)]
N_IMAGES = 50

MEAN255 = {1: [0.1307 * 255.0], 3: [125.3, 123.0, 113.9]}
STD255 = {1: [0.3081 * 255.0], 3: [63.0, 62.1, 66.7]}


def norm_consts(C):
    """(mean255, inv_std255) as lists of f32-representable Python floats,
    computed the way RealDataset computes ds.mean / ds.inv_std."""
    mean = torch.tensor(MEAN255[C], dtype=torch.float32)
    inv = 1.0 / torch.tensor(STD255[C], dtype=torch.float32)
    return mean.tolist(), inv.tolist()


@functools.lru_cache(maxsize=None)
def fake_dataset(C, H, W):
    """CPU (x_u8 [N,C,H,W], y [N]) with every byte value present."""
    g = torch.Generator().manual_seed(C * 10007 + H * 101 + W)
    x = torch.randint(0, 256, (N_IMAGES, C, H, W), generator=g,
                      dtype=torch.uint8)
    x.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    y = torch.randint(0, 10, (N_IMAGES,), generator=g)
    return x, y


@functools.lru_cache(maxsize=None)
def fake_indices(B):
    """In-range int64 [B]: descending, with repeats (for B > 2), the last
    image included."""
    m = min(N_IMAGES, B // 2 + 1)
    idx = N_IMAGES - 1 - (torch.arange(B) * 7) % m
    idx, _ = torch.sort(idx, descending=True)
    return idx.contiguous()


def per_sample_ref(x_u8, y, idx, mean255, inv_std255, pad, pad_mode, draws,
                   dtype):
    """Per sample: F.pad on the float image, slice at (oy, ox), optional
    flip, then the loader's normalize formula. NCHW result + labels."""
    C, H, W = x_u8.shape[1:]
    mean = torch.tensor(mean255, dtype=torch.float32).view(C, 1, 1)
    inv = torch.tensor(inv_std255, dtype=torch.float32).view(C, 1, 1)
    out = []
    for b, n in enumerate(idx.tolist()):
        img = x_u8[n].float()
        if draws is not None:
            oy, ox, flip = (int(draws[0][b]), int(draws[1][b]),
                            bool(draws[2][b]))
            if pad:
                img = F.pad(img[None], (pad,) * 4, mode=pad_mode)[0]
            img = img[:, oy:oy + H, ox:ox + W]
            if flip:
                img = img.flip(-1)
        out.append(((img - mean) * inv).to(dtype))
    return torch.stack(out), y[idx]


def bits(t):
    """Raw bits, so that -0.0 != 0.0 and NaNs compare."""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16
                               else torch.int32)


def write_cifar10(root, n_train, n_test=16):
    """Fake CIFAR-10 pickle batches: n_train images over the 5 train files."""
    d = os.path.join(root, 'cifar-10-batches-py')
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(1)
    sizes = [len(a) for a in np.array_split(np.arange(n_train), 5)]
    names = [f'data_batch_{i}' for i in range(1, 6)] + ['test_batch']
    for name, n in zip(names, sizes + [n_test]):
        data = rng.integers(0, 256, (n, 3072), dtype=np.uint8)
        labels = rng.integers(0, 10, n).tolist()
        with open(os.path.join(d, name), 'wb') as f:
            pickle.dump({'data': data, 'labels': labels}, f)
    return root
