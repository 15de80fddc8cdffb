"""Shared helpers of the fan-in tests: payload builders on the existing CPU
packers, hand-made edge-case payloads, and an independent numpy-float32 left
fold of the sum contract (docs/KERNELS.md, fanin.hip)."""
import numpy as np
import torch

from ps_pytorch_amd.ops import functional as F

# (name, codec, k, raw dtype)
CODECS = [
    ('raw_f32', 'raw', None, torch.float32),
    ('raw_bf16', 'raw', None, torch.bfloat16),
    ('q8', 'q8', None, None),
    ('topk4', 'topk', 4, None),
    ('topk8', 'topk', 8, None),
    ('topk16', 'topk', 16, None),
    ('topk32', 'topk', 32, None),
]
CODEC_IDS = [c[0] for c in CODECS]


def encode(x: torch.Tensor, codec: str, k, dtype) -> torch.Tensor:
    """One worker's wire contribution for the f32 gradient `x`, built with
    the existing CPU packers."""
    n = x.numel()
    if codec == 'raw':
        return x.to(dtype).contiguous()
    if codec == 'q8':
        p = torch.zeros(F.q8_layout(n)[1], dtype=torch.uint8)
        F.pack_q8(p, x)
        return p
    p = torch.zeros(F.topk_layout(n, k)[1], dtype=torch.uint8)
    F.pack_topk_ef(p, x, torch.zeros(n), k)
    return p


def make_sources(codec: str, k, dtype, W: int, n: int, seed: int = 0):
    g = torch.Generator().manual_seed(seed * 7919 + n)
    return [encode(torch.randn(n, generator=g) * (0.5 + j), codec, k, dtype)
            for j in range(W)]


def order_triple(codec: str, k, dtype, n: int):
    """Sources worth 1e8, -1e8 and 1 (up to the codec's rounding) at every
    sent position: (a + b) + c != (a + c) + b in f32."""
    return [encode(torch.full((n,), v), codec, k, dtype)
            for v in (1e8, -1e8, 1.0)]


def zero_payload(codec: str, k, dtype, n: int) -> torch.Tensor:
    """What a killed worker sends: all-zero bytes."""
    if codec == 'raw':
        return torch.zeros(n, dtype=dtype)
    tot = F.q8_layout(n)[1] if codec == 'q8' else F.topk_layout(n, k)[1]
    return torch.zeros(tot, dtype=torch.uint8)


def topk_edge_payload(n: int, k: int, seed: int) -> torch.Tensor:
    """A hand-made top-k payload no packer would emit: indices drawn with
    replacement (repeats inside a block) over the whole 0..255 range (so in
    a tail block most point at or past n), entry 0 and 1 of every block
    forced equal, values of both signs."""
    off, tot = F.topk_layout(n, k)
    g = torch.Generator().manual_seed(seed)
    nblk = off // k
    idx = torch.randint(0, 256, (nblk, k), generator=g)
    idx[:, 1] = idx[:, 0]
    # the tail block: make sure some entries do land below n, repeated
    idx[-1, :2] = 0
    vals = (torch.randn(nblk, k, generator=g) * 3).to(torch.bfloat16)
    p = torch.zeros(tot, dtype=torch.uint8)
    p[:off] = idx.to(torch.uint8).view(-1)
    p[off:] = vals.contiguous().view(-1).view(torch.uint8)
    return p


def _bf16_bytes_to_f32(b: np.ndarray) -> np.ndarray:
    u = b.view(np.uint16).astype(np.uint32) << np.uint32(16)
    return u.view(np.float32)


def numpy_fold(srcs, codec: str, k, n: int) -> np.ndarray:
    """The sum contract written out in numpy float32, independent of the
    torch paths: s = +0; for each source in order s = s + dec (q8: dec is a
    float32 product, then the add; top-k: entries in payload order)."""
    s = np.zeros(n, dtype=np.float32)
    for p in srcs:
        if codec == 'raw':
            if p.dtype == torch.bfloat16:
                dec = _bf16_bytes_to_f32(
                    p.view(torch.int16).numpy().view(np.uint8).copy())
            else:
                dec = p.numpy().astype(np.float32)
            s = (s + dec).astype(np.float32)
        elif codec == 'q8':
            b = p.numpy().copy()
            qb = (n + 3) & ~3
            nblk = (n + 255) // 256
            q = b[:n].view(np.int8).astype(np.float32)
            sc = b[qb:qb + 4 * nblk].view(np.float32)
            dec = (q * np.repeat(sc, 256)[:n]).astype(np.float32)
            s = (s + dec).astype(np.float32)
        else:
            b = p.numpy().copy()
            nblk = (n + 255) // 256
            idx = b[:nblk * k].reshape(nblk, k).astype(np.int64)
            vals = _bf16_bytes_to_f32(b[nblk * k:]).reshape(nblk, k)
            for blk in range(nblk):
                for t in range(k):
                    pos = blk * 256 + idx[blk, t]
                    if pos < n:
                        s[pos] = np.float32(s[pos] + vals[blk, t])
    return s


def bits(t) -> np.ndarray:
    """int32 view for bitwise comparison (tensor or ndarray, f32)."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)
