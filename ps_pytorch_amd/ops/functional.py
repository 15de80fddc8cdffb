"""Python-facing ops: HIP kernels on GPU, torch reference path on CPU.

Every GPU entry point calls require_lib() — a GPU host without the in-tree
libps_hip.so fails loudly (no silent eager fallback). The CPU paths double
as the numerics references for the kernel tests (tests/test_ops_*.py).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import require_lib, dtype_tag, current_stream_ptr


def _check_flat(t: torch.Tensor, name: str, n: int) -> None:
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.numel() != n:
        raise ValueError(f"{name} numel {t.numel()} != {n}")


def fused_sgd_step(
    w: torch.Tensor,            # f32 master weights (flat)
    grad_sum: torch.Tensor,     # f32 or bf16 summed grads (flat)
    momentum_buf: torch.Tensor, # f32 (flat)
    lr: float,
    momentum: float = 0.0,
    weight_decay: float = 0.0,
    grad_scale: float = 1.0,    # usually 1/num_aggregate
    nesterov: bool = False,
    wire_out: Optional[torch.Tensor] = None,  # optional f32/bf16 broadcast payload
) -> None:
    """w/m update + optional wire re-pack, semantics of ref src/optim/sgd.py:59-92
    (momentum buffer m = mu*m + g; w -= lr*m; nesterov variant as torch)."""
    n = w.numel()
    _check_flat(w, "w", n)
    _check_flat(grad_sum, "grad_sum", n)
    _check_flat(momentum_buf, "momentum_buf", n)
    if wire_out is not None:
        _check_flat(wire_out, "wire_out", n)

    if w.is_cuda:
        if n % 4:
            raise ValueError("flat buffers must be padded to a multiple of 4")
        lib = require_lib()
        lib.ps_fused_sgd(
            w.data_ptr(), grad_sum.data_ptr(), momentum_buf.data_ptr(),
            0 if wire_out is None else wire_out.data_ptr(), n,
            float(lr), float(momentum), float(weight_decay), float(grad_scale),
            int(nesterov), dtype_tag(grad_sum.dtype),
            dtype_tag(wire_out.dtype) if wire_out is not None else 0,
            current_stream_ptr())
        return

    # CPU reference path (also the golden model for the kernel test)
    g = grad_sum.to(torch.float32) * grad_scale
    if weight_decay:
        g = g.add(w, alpha=weight_decay)
    momentum_buf.mul_(momentum).add_(g)
    upd = g.add(momentum_buf, alpha=momentum) if nesterov else momentum_buf
    w.add_(upd, alpha=-lr)
    if wire_out is not None:
        wire_out.copy_(w.to(wire_out.dtype))



def fused_adam_step(
    w: torch.Tensor, grad_sum: torch.Tensor, exp_avg: torch.Tensor,
    exp_avg_sq: torch.Tensor, t: int, lr: float, beta1: float, beta2: float,
    eps: float, weight_decay: float = 0.0, grad_scale: float = 1.0,
    max_exp_avg_sq: Optional[torch.Tensor] = None,
    wire_out: Optional[torch.Tensor] = None,
) -> None:
    """Fused flat Adam (ref src/optim/adam.py:48-95 semantics, incl.
    amsgrad); one kernel pass on GPU, torch ops on CPU."""
    n = w.numel()
    _check_flat(w, "w", n)
    _check_flat(grad_sum, "grad_sum", n)
    bc1 = 1.0 - beta1 ** t
    bc2 = 1.0 - beta2 ** t
    if w.is_cuda:
        if n % 4:
            raise ValueError("flat buffers must be padded to a multiple of 4")
        lib = require_lib()
        lib.ps_fused_adam(
            w.data_ptr(), grad_sum.data_ptr(), exp_avg.data_ptr(),
            exp_avg_sq.data_ptr(),
            0 if max_exp_avg_sq is None else max_exp_avg_sq.data_ptr(),
            0 if wire_out is None else wire_out.data_ptr(), n,
            float(lr / bc1), float(beta1), float(beta2), float(1.0 / bc2),
            float(eps), float(weight_decay), float(grad_scale),
            dtype_tag(grad_sum.dtype),
            dtype_tag(wire_out.dtype) if wire_out is not None else 0,
            current_stream_ptr())
        return
    g = grad_sum.to(torch.float32)
    if grad_scale != 1.0:
        g = g * grad_scale
    if weight_decay:
        g = g.add(w, alpha=weight_decay)
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    if max_exp_avg_sq is not None:
        torch.maximum(max_exp_avg_sq, exp_avg_sq, out=max_exp_avg_sq)
        denom = (max_exp_avg_sq / bc2).sqrt_().add_(eps)
    else:
        denom = (exp_avg_sq / bc2).sqrt_().add_(eps)
    w.addcdiv_(exp_avg, denom, value=-lr / bc1)
    if wire_out is not None:
        wire_out.copy_(w.to(wire_out.dtype))


# ---- fused LARS (ops/kernels/lars.hip) ----
# Per parameter tensor ("segment") of the flat layout: Sw = sum w^2 over the
# f32 master weights and Sg = sum g^2 over the raw gradient sum, both in
# float64; then in float64 wn = sqrt(Sw), gn = grad_scale * sqrt(Sg),
#   ratio = eta*wn / (gn + wd*wn + eps)  if adapt and wn > 0 and gn > 0 else 1
#   local_lr = f32(lr * ratio),  wd_seg = wd if adapt else 0
# with adapt = ndim > 1 and lr = lr_table[min(step_ctr, T-1)], latched into
# lr_cur (and step_ctr incremented) only by a call with advance=True. The
# update is, per element in f32: g = s*scale (+ wd_seg*w, one fma);
# m = fma(mu, m, local_lr*g); w = w - m; wire = cast(w). The CPU paths are
# the numerics oracle: torch float64 sums, the scalar formula in Python
# floats, the elementwise chain in f32 with fma taken through float64.

LARS_CHUNK = 4096      # elements per chunk (LARS_CHUNK in lars.hip)
LARS_ALIGN = 8         # segment starts: FlatSpace's ALIGN


class LarsLayout:
    """Chunk and segment tables of one flat layout plus the per-layout
    workspaces, built once and kept on `device`.

    segments: (offset, numel, ndim) per parameter in flat order, offsets
    multiples of 8 and ascending (FlatSpace.segments()); total: numel of the
    flat buffers (a multiple of 8). A chunk is a LARS_CHUNK piece of a
    segment counted from the segment's start; its update extent runs to the
    next chunk's start, so alignment gaps travel with the tensor in front of
    them. A region (start, end) must begin at a segment start and end at one
    (or at `total`): it then is a contiguous chunk and segment range."""

    def __init__(self, segments, total: int, device=None):
        segs = [(int(o), int(n), int(d)) for o, n, d in segments]
        if not segs:
            raise ValueError("LARS needs at least one segment")
        total = int(total)
        if total % LARS_ALIGN:
            raise ValueError(f"flat numel {total} is no multiple of "
                             f"{LARS_ALIGN}")
        prev_end = 0
        for o, n, d in segs:
            if o % LARS_ALIGN or o < prev_end or n < 0:
                raise ValueError(f"segment ({o}, {n}) is unaligned, "
                                 "overlapping or out of order")
            prev_end = o + n
        if prev_end > total or segs[0][0] != 0:
            raise ValueError("segments must start at 0 and fit the buffer")
        self.segments = segs
        self.total = total
        self.device = torch.device(device) if device is not None \
            else torch.device('cpu')
        self.seg_offsets = [o for o, _, _ in segs]
        starts, lens, cseg, seg_c0 = [], [], [], []
        for s, (o, n, _) in enumerate(segs):
            seg_c0.append(len(starts))
            for c in range(0, n, LARS_CHUNK):
                starts.append(o + c)
                lens.append(min(LARS_CHUNK, n - c))
                cseg.append(s)
        seg_c0.append(len(starts))
        starts.append(total)
        if len(starts) - 1 >= 2 ** 31:
            raise ValueError("too many chunks")
        self.nseg, self.nchunk = len(segs), len(starts) - 1
        self.seg_chunk0_host = seg_c0
        dev = self.device
        self.chunk_start = torch.tensor(starts, dtype=torch.int64, device=dev)
        self.chunk_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        self.chunk_seg = torch.tensor(cseg, dtype=torch.int32, device=dev)
        self.seg_chunk0 = torch.tensor(seg_c0, dtype=torch.int32, device=dev)
        self.seg_adapt = torch.tensor([int(d > 1) for _, _, d in segs],
                                      dtype=torch.int32, device=dev)
        # workspaces: per-chunk (Sw, Sg) partials, per-segment sums and the
        # per-segment step size / decay the update reads
        self.partial = torch.zeros(max(self.nchunk, 1), 2,
                                   dtype=torch.float64, device=dev)
        self.seg_sums = torch.zeros(self.nseg, 2, dtype=torch.float64,
                                    device=dev)
        self.local_lr = torch.zeros(self.nseg, dtype=torch.float32, device=dev)
        self.wd_seg = torch.zeros(self.nseg, dtype=torch.float32, device=dev)

    def ranges(self, region=None):
        """(seg0, seg1, chunk0, chunk1, start, end) of a region."""
        import bisect
        if region is None:
            return 0, self.nseg, 0, self.nchunk, 0, self.total
        st, en = int(region[0]), int(region[1])
        s0 = bisect.bisect_left(self.seg_offsets, st)
        s1 = (self.nseg if en == self.total
              else bisect.bisect_left(self.seg_offsets, en))
        if (s0 >= self.nseg or self.seg_offsets[s0] != st or st > en
                or (en != self.total and (s1 >= self.nseg or
                                          self.seg_offsets[s1] != en))):
            raise ValueError(f"region {(st, en)} does not run from one "
                             "parameter start to another")
        return (s0, s1, self.seg_chunk0_host[s0], self.seg_chunk0_host[s1],
                st, en)


def _lars_check(layout: LarsLayout, w, g, m=None, wire_out=None) -> None:
    if w.dtype != torch.float32:
        raise TypeError("master weights must be f32")
    if g.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("the gradient sum must be f32 or bf16")
    if m is not None and m.dtype != torch.float32:
        raise TypeError("momentum must be f32")
    for name, t in (("w", w), ("grad_sum", g), ("momentum_buf", m),
                    ("wire_out", wire_out)):
        if t is None:
            continue
        _check_flat(t, name, layout.total)
        if t.device != layout.device:
            raise ValueError(f"{name} is on {t.device}, the LARS layout on "
                             f"{layout.device}")
        if t.is_cuda and t.data_ptr() % 16:
            raise ValueError(f"{name} must be 16-byte aligned")


def lars_norms(layout: LarsLayout, w: torch.Tensor, grad_sum: torch.Tensor,
               lr_table: torch.Tensor, step_ctr: torch.Tensor,
               lr_cur: torch.Tensor, grad_scale: float = 1.0,
               eta: float = 1e-3, weight_decay: float = 0.0,
               eps: float = 0.0, region=None, advance: bool = True) -> None:
    """Per-segment norms and step sizes of the region's segments into
    layout.seg_sums / local_lr / wd_seg. w, grad_sum: the WHOLE flat buffers.
    lr_table f32 [T], step_ctr i64 [1], lr_cur f32 [1] live on the layout's
    device; advance latches lr_cur from the table and bumps step_ctr before
    the step sizes are formed. No host sync on the GPU."""
    _lars_check(layout, w, grad_sum)
    if (lr_table.dtype != torch.float32 or step_ctr.dtype != torch.int64
            or lr_cur.dtype != torch.float32 or lr_table.numel() < 1):
        raise TypeError("lr_table/lr_cur must be f32 and step_ctr i64")
    s0, s1, c0, c1, _, _ = layout.ranges(region)
    if w.is_cuda:
        if advance and c1 == c0:
            raise ValueError("an advancing LARS step needs a non-empty region")
        rc = require_lib().ps_lars_norms(
            w.data_ptr(), grad_sum.data_ptr(), dtype_tag(grad_sum.dtype),
            layout.chunk_start.data_ptr(), layout.chunk_len.data_ptr(),
            c0, c1 - c0, layout.seg_chunk0.data_ptr(),
            layout.seg_adapt.data_ptr(), s0, s1 - s0,
            layout.partial.data_ptr(), layout.seg_sums.data_ptr(),
            layout.local_lr.data_ptr(), layout.wd_seg.data_ptr(),
            lr_table.data_ptr(), lr_table.numel(), step_ctr.data_ptr(),
            lr_cur.data_ptr(), int(bool(advance)), float(grad_scale),
            float(eta), float(weight_decay), float(eps),
            current_stream_ptr())
        if rc:
            raise RuntimeError(f"ps_lars_norms launched nothing (code {rc})")
        return
    import math
    import numpy as np
    if advance:
        i = min(max(int(step_ctr), 0), lr_table.numel() - 1)
        lr_cur.copy_(lr_table[i:i + 1])
        step_ctr += 1
    lr = float(lr_cur)
    gs, eta, wd, eps = (float(grad_scale), float(eta), float(weight_decay),
                        float(eps))
    for s in range(s0, s1):
        off, n, ndim = layout.segments[s]
        sw = float(w[off:off + n].to(torch.float64).square().sum())
        sg = float(grad_sum[off:off + n].to(torch.float64).square().sum())
        adapt = ndim > 1
        wn, gn = math.sqrt(sw), gs * math.sqrt(sg)
        ratio = 1.0
        if adapt and wn > 0.0 and gn > 0.0:
            ratio = eta * wn / (gn + wd * wn + eps)
        layout.seg_sums[s, 0] = sw
        layout.seg_sums[s, 1] = sg
        layout.local_lr[s] = float(np.float32(lr * ratio))
        layout.wd_seg[s] = float(np.float32(wd)) if adapt else 0.0


def _fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """f32 fma through float64: the product is exact there, the sum rounds to
    f64 and then to f32 (at most one double-rounding ulp from fmaf)."""
    return (a.to(torch.float64) * b.to(torch.float64)
            + c.to(torch.float64)).to(torch.float32)


def lars_step(layout: LarsLayout, w: torch.Tensor, grad_sum: torch.Tensor,
              momentum_buf: torch.Tensor, momentum: float = 0.0,
              grad_scale: float = 1.0,
              wire_out: Optional[torch.Tensor] = None, region=None) -> None:
    """The LARS update of the region (alignment gaps included) with the step
    sizes lars_norms left in layout.local_lr / wd_seg. All tensors are the
    WHOLE flat buffers."""
    _lars_check(layout, w, grad_sum, momentum_buf, wire_out)
    s0, s1, c0, c1, st, en = layout.ranges(region)
    if w.is_cuda:
        rc = require_lib().ps_lars_update(
            w.data_ptr(), grad_sum.data_ptr(), momentum_buf.data_ptr(),
            0 if wire_out is None else wire_out.data_ptr(),
            dtype_tag(grad_sum.dtype),
            dtype_tag(wire_out.dtype) if wire_out is not None else 0,
            layout.chunk_start.data_ptr(), layout.chunk_seg.data_ptr(),
            c0, c1 - c0, layout.local_lr.data_ptr(),
            layout.wd_seg.data_ptr(), float(momentum), float(grad_scale),
            current_stream_ptr())
        if rc:
            raise RuntimeError(f"ps_lars_update launched nothing (code {rc})")
        return
    scale = torch.tensor(float(grad_scale), dtype=torch.float32)
    mu = torch.tensor(float(momentum), dtype=torch.float32)
    for s in range(s0, s1):
        a = layout.seg_offsets[s]
        if not layout.segments[s][1]:
            continue                     # an empty tensor owns no chunk
        b = en
        for o, n, _ in layout.segments[s + 1:s1]:
            if n:
                b = o
                break
        llr, wds = layout.local_lr[s], layout.wd_seg[s]
        ws, ms = w[a:b], momentum_buf[a:b]
        gk = grad_sum[a:b].to(torch.float32) * scale
        if float(wds) != 0.0:
            gk = _fma32(wds, ws, gk)
        mk = _fma32(mu, ms, llr * gk)
        ms.copy_(mk)
        ws.copy_(ws - mk)
    if wire_out is not None:
        wire_out[st:en].copy_(w[st:en].to(wire_out.dtype))


def pack_wire(dst: torch.Tensor, src: torch.Tensor) -> None:
    """Wire pack: f32 -> bf16 (the GPU 'compression' path, ref compression.py
    g_compress role) or plain copy when dtypes match."""
    n = src.numel()
    _check_flat(dst, "dst", n)
    if dst.dtype == src.dtype:
        dst.copy_(src)
        return
    if src.is_cuda:
        lib = require_lib()
        if src.dtype == torch.float32 and dst.dtype == torch.bfloat16:
            lib.ps_pack_bf16(dst.data_ptr(), src.data_ptr(), n, current_stream_ptr())
        elif src.dtype == torch.bfloat16 and dst.dtype == torch.float32:
            lib.ps_unpack_bf16(dst.data_ptr(), src.data_ptr(), n, current_stream_ptr())
        else:
            raise TypeError(f"unsupported pack {src.dtype} -> {dst.dtype}")
        return
    dst.copy_(src.to(dst.dtype))


unpack_wire = pack_wire  # symmetric: direction decided by dtypes


# ---- block-scaled int8 codec (the blosc-role GPU compressor) ----
# Scheme/layout documented in ops/kernels/quant.hip: 256-elem blocks,
# per-block f32 scale = max|x|/127, payload = [int8 x align4(n)][f32 x nblk].
# The CPU path below is the numerics REFERENCE for the HIP kernels and the
# gloo test path; both round identically (rint == torch.round, half-to-even).

Q8_BLOCK = 256


def q8_layout(n: int):
    """(scales_byte_offset, total_payload_bytes) for n f32 values."""
    qb = (n + 3) & ~3
    nblk = (n + Q8_BLOCK - 1) // Q8_BLOCK
    return qb, qb + 4 * nblk


def pack_q8(payload: torch.Tensor, src: torch.Tensor) -> None:
    """Compress flat f32 `src` into the uint8 `payload` buffer (4x vs f32)."""
    n = src.numel()
    qb, tot = q8_layout(n)
    if payload.dtype != torch.uint8 or payload.numel() != tot:
        raise ValueError(f"payload must be uint8[{tot}], got "
                         f"{payload.dtype}[{payload.numel()}]")
    if src.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("q8 source must be f32 or bf16")
    _check_flat(src, "src", n)
    if src.is_cuda:
        require_lib().ps_pack_q8(payload.data_ptr(), src.data_ptr(), n,
                                 dtype_tag(src.dtype), current_stream_ptr())
        return
    q, scale = _q8_encode_cpu(src.to(torch.float32))
    payload[:n] = q.view(-1)[:n].to(torch.int8).view(torch.uint8)
    payload[qb:qb + 4 * scale.numel()].view(torch.float32).copy_(scale)


def _q8_encode_cpu(x: torch.Tensor):
    """CPU block encode of flat f32 `x`: (f32 quants [nblk, 256] holding the
    clamped integers, zero in the pad; f32 scales [nblk])."""
    n = x.numel()
    nblk = (n + Q8_BLOCK - 1) // Q8_BLOCK
    xp = torch.zeros(nblk * Q8_BLOCK, dtype=torch.float32)
    xp[:n] = x
    xb = xp.view(nblk, Q8_BLOCK)
    m = xb.abs().amax(dim=1)
    # NB: divide f32-tensor by f32-tensor — torch computes python-scalar /
    # tensor in f64 and casts, which is 1 ulp off strict f32 division and
    # breaks bitwise parity with the GPU kernel's IEEE f32 divide.
    c127 = torch.full_like(m, 127.0)
    inv = torch.where(m > 0, c127 / m, torch.zeros_like(m))
    q = torch.clamp(torch.round(xb * inv[:, None]), -127, 127)
    return q, m / c127


def _check_residual(residual: torch.Tensor, src: torch.Tensor) -> None:
    if residual.dtype != torch.float32:
        raise TypeError("error-feedback residual must be f32")
    _check_flat(residual, "residual", src.numel())
    if residual.device != src.device:
        raise ValueError("residual and src must live on the same device")


def pack_q8_ef(payload: torch.Tensor, src: torch.Tensor,
               residual: torch.Tensor) -> None:
    """pack_q8 with error feedback: encode c = src + residual and leave
    c - decode(payload) in `residual` (f32, same numel as src, in place) —
    what this step's code could not carry is added to the next step's
    gradient. With residual == 0 the payload equals pack_q8's.

    Per element, each operation rounded to f32 once: c = g + e; per block
    m = max|c|, inv = 127/m (0 when m == 0), scale = m/127;
    q = clamp(rint(c*inv), +-127); dec = q*scale; e' = c - dec. dec is what
    unpack_q8 (no accumulate) yields. The CPU path below is the bitwise
    reference of ps_pack_q8_ef."""
    n = src.numel()
    qb, tot = q8_layout(n)
    if payload.dtype != torch.uint8 or payload.numel() != tot:
        raise ValueError(f"payload must be uint8[{tot}], got "
                         f"{payload.dtype}[{payload.numel()}]")
    if src.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("q8 source must be f32 or bf16")
    _check_flat(src, "src", n)
    _check_residual(residual, src)
    if src.is_cuda:
        require_lib().ps_pack_q8_ef(payload.data_ptr(), src.data_ptr(),
                                    residual.data_ptr(), n,
                                    dtype_tag(src.dtype), current_stream_ptr())
        return
    c = src.to(torch.float32) + residual
    q, scale = _q8_encode_cpu(c)
    payload[:n] = q.view(-1)[:n].to(torch.int8).view(torch.uint8)
    payload[qb:qb + 4 * scale.numel()].view(torch.float32).copy_(scale)
    dec = q * scale[:, None]
    residual.copy_(c - dec.view(-1)[:n])


def pack_wire_ef(dst: torch.Tensor, src: torch.Tensor,
                 residual: torch.Tensor) -> None:
    """f32 -> bf16 wire pack with error feedback: dst = bf16(src + residual)
    (round to nearest even) and residual = (src + residual) - f32(dst), in
    place; the subtraction is exact in f32."""
    n = src.numel()
    if src.dtype != torch.float32 or dst.dtype != torch.bfloat16:
        raise TypeError(f"error-feedback wire pack is f32 -> bf16, got "
                        f"{src.dtype} -> {dst.dtype}")
    _check_flat(src, "src", n)
    _check_flat(dst, "dst", n)
    _check_residual(residual, src)
    if src.is_cuda:
        require_lib().ps_pack_bf16_ef(dst.data_ptr(), src.data_ptr(),
                                      residual.data_ptr(), n,
                                      current_stream_ptr())
        return
    c = src + residual
    dst.copy_(c.to(torch.bfloat16))
    residual.copy_(c - dst.to(torch.float32))


def unpack_q8(dst: torch.Tensor, payload: torch.Tensor,
              accumulate: bool = False) -> None:
    """Decompress `payload` into f32 `dst` (dst += values if accumulate)."""
    n = dst.numel()
    qb, tot = q8_layout(n)
    if payload.numel() != tot:
        raise ValueError(f"payload size {payload.numel()} != {tot}")
    if dst.dtype != torch.float32:
        raise TypeError("q8 destination must be f32")
    _check_flat(dst, "dst", n)
    if dst.is_cuda:
        require_lib().ps_unpack_q8(dst.data_ptr(), payload.data_ptr(), n,
                                   int(accumulate), current_stream_ptr())
        return
    nblk = (n + Q8_BLOCK - 1) // Q8_BLOCK
    q = payload[:n].view(torch.int8).to(torch.float32)
    scales = payload[qb:qb + 4 * nblk].view(torch.float32)
    vals = q * scales.repeat_interleave(Q8_BLOCK)[:n]
    if accumulate:
        dst.add_(vals)
    else:
        dst.copy_(vals)


# ---- block top-k sparsifying codec (error-feedback path only) ----
# Contract documented in ops/kernels/topk.hip and docs/KERNELS.md: of every
# 256-element block of c = src + residual the K elements with the largest
# keys (bits(|c|) << 8) | (255 - index) go on the wire as
# [u8 idx x nblk*K][bf16 val x nblk*K]; the rest stays in the residual. The
# CPU paths below are the gloo path and the bitwise reference of the kernels.

TOPK_BLOCK = 256
TOPK_KS = (4, 8, 16, 32)


def _check_topk_k(k: int) -> None:
    if k not in TOPK_KS:
        raise ValueError(f"top-k codec keeps k in {TOPK_KS} per "
                         f"{TOPK_BLOCK}-block, got {k!r}")


def topk_layout(n: int, k: int):
    """(vals_byte_offset, total_payload_bytes) for n values at k per block."""
    _check_topk_k(k)
    nblk = (n + TOPK_BLOCK - 1) // TOPK_BLOCK
    return nblk * k, 3 * nblk * k


def _check_topk_payload(payload: torch.Tensor, tot: int) -> None:
    if payload.dtype != torch.uint8 or payload.numel() != tot:
        raise ValueError(f"payload must be uint8[{tot}], got "
                         f"{payload.dtype}[{payload.numel()}]")
    if not payload.is_contiguous():
        raise ValueError("payload must be contiguous")
    if payload.data_ptr() % 2:
        raise ValueError("payload must be 2-byte aligned (bf16 values)")


def pack_topk_ef(payload: torch.Tensor, src: torch.Tensor,
                 residual: torch.Tensor, k: int) -> None:
    """Top-k encode c = src + residual (one f32 add) into `payload` and
    leave what was not sent in `residual` (f32, same numel, in place).

    Per 256-block the k largest keys (bits(|c_i|) << 8) | (255 - i) are sent
    — larger magnitude first, ties to the lower index, +-Inf and NaN above
    every finite value; positions past n in the tail block count as +0 —
    in ascending index order, val = bf16(c_i) rounded to nearest even. The
    residual becomes c - f32(val) where sent (exact for finite c) and c
    elsewhere. The CPU path below is the bitwise reference of
    ps_pack_topk_ef."""
    n = src.numel()
    off, tot = topk_layout(n, k)
    _check_topk_payload(payload, tot)
    if src.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("top-k source must be f32 or bf16")
    _check_flat(src, "src", n)
    _check_residual(residual, src)
    if payload.device != src.device:
        raise ValueError("payload and src must live on the same device")
    if src.is_cuda:
        if require_lib().ps_pack_topk_ef(payload.data_ptr(), src.data_ptr(),
                                         residual.data_ptr(), n, k,
                                         dtype_tag(src.dtype),
                                         current_stream_ptr()):
            raise RuntimeError(f"ps_pack_topk_ef has no kernel for k={k}")
        return
    nblk = off // k
    cb = torch.zeros(nblk * TOPK_BLOCK, dtype=torch.float32)
    cb[:n] = src.to(torch.float32) + residual
    cb = cb.view(nblk, TOPK_BLOCK)
    # integer keys are unique, so topk's choice is fully determined (a float
    # topk would leave the order of ties open)
    mag = (cb.view(torch.int32) & 0x7fffffff).to(torch.int64)
    key = (mag << 8) | (255 - torch.arange(TOPK_BLOCK, dtype=torch.int64))
    idx = torch.topk(key, k, dim=1).indices.sort(dim=1).values
    sent = cb.gather(1, idx)
    vals = sent.to(torch.bfloat16)
    payload[:off] = idx.to(torch.uint8).view(-1)
    payload[off:] = vals.contiguous().view(-1).view(torch.uint8)
    cb.scatter_(1, idx, sent - vals.to(torch.float32))
    residual.copy_(cb.view(-1)[:n])


def unpack_topk(dst: torch.Tensor, payload: torch.Tensor, k: int,
                accumulate: bool = False) -> None:
    """Decode a top-k `payload` into f32 `dst`: zero-fill unless
    `accumulate`, then for every block and j = 0..k-1 in payload order
    dst[blk*256 + idx_j] += f32(val_j) where that position is < n. Indices
    may repeat (a killed worker's all-zero payload adds +0 to element 0 of
    each block k times); the add order is fixed, no atomics."""
    n = dst.numel()
    off, tot = topk_layout(n, k)
    _check_topk_payload(payload, tot)
    if dst.dtype != torch.float32:
        raise TypeError("top-k destination must be f32")
    _check_flat(dst, "dst", n)
    if payload.device != dst.device:
        raise ValueError("payload and dst must live on the same device")
    if dst.is_cuda:
        if require_lib().ps_unpack_topk(dst.data_ptr(), payload.data_ptr(),
                                        n, k, int(accumulate),
                                        current_stream_ptr()):
            raise RuntimeError(f"ps_unpack_topk has no kernel for k={k}")
        return
    nblk = off // k
    idx = payload[:off].view(nblk, k).to(torch.int64)
    vals = payload[off:].clone().view(torch.bfloat16).view(nblk, k).to(
        torch.float32)
    base = torch.arange(nblk, dtype=torch.int64) * TOPK_BLOCK
    if not accumulate:
        dst.zero_()
    for j in range(k):
        # one entry per block: positions within a pass are distinct
        pos = base + idx[:, j]
        live = pos < n
        dst[pos[live]] += vals[:, j][live]


def acc_into(acc: torch.Tensor, src: torch.Tensor) -> None:
    """acc += src (f32 acc; f32/bf16 src) — PS fan-in accumulate for
    uncompressed gather mode (the reference's Waitany += loop,
    sync_replicas_master_nn.py:157-186, on-device)."""
    n = acc.numel()
    _check_flat(acc, "acc", n)
    _check_flat(src, "src", n)
    if acc.dtype != torch.float32:
        raise TypeError("accumulator must be f32")
    if acc.is_cuda:
        require_lib().ps_acc(acc.data_ptr(), src.data_ptr(), n,
                             dtype_tag(src.dtype), current_stream_ptr())
        return
    acc.add_(src.to(torch.float32))


# ---- rank-ordered fan-in (ops/kernels/fanin.hip) ----
# One launch decodes up to 16 staged payloads of one bucket and sums them in
# the order given: s = +0; s = s + dec_j, one f32 add per source. raw: dec is
# the (widened) value; q8: dec = f32(q) * scale, a rounded multiply and then
# the add (no fma); topk: a source's entries are added in payload order. The
# CPU paths below are the gloo path and the bitwise reference of the kernels.

FANIN_MAX_SRCS = 16
FANIN_CODECS = ('raw', 'q8', 'topk')
_FANIN_F32, _FANIN_BF16, _FANIN_Q8, _FANIN_TOPK = 0, 1, 2, 3


def _fanin_check(n: int, device, srcs, codec: str, k) -> int:
    """Validate the sources of one fan-in over n elements; returns the codec
    tag of the native entry points."""
    if codec not in FANIN_CODECS:
        raise ValueError(f"unknown fan-in codec {codec!r}, one of "
                         f"{FANIN_CODECS}")
    if len(srcs) > FANIN_MAX_SRCS:
        raise ValueError(f"fan-in takes at most {FANIN_MAX_SRCS} sources, "
                         f"got {len(srcs)}")
    if codec == 'topk':
        _, tot = topk_layout(n, k)          # raises for a bad k
        for s in srcs:
            _check_topk_payload(s, tot)
        tag = _FANIN_TOPK
    elif codec == 'q8':
        _, tot = q8_layout(n)
        for s in srcs:
            if s.dtype != torch.uint8 or s.numel() != tot:
                raise ValueError(f"payload must be uint8[{tot}], got "
                                 f"{s.dtype}[{s.numel()}]")
        tag = _FANIN_Q8
    else:
        dt = srcs[0].dtype if srcs else torch.float32
        if dt not in (torch.float32, torch.bfloat16):
            raise TypeError("raw fan-in sources must be f32 or bf16")
        for s in srcs:
            if s.dtype != dt:
                raise TypeError("raw fan-in sources must share one dtype")
            _check_flat(s, "src", n)
        tag = _FANIN_BF16 if dt == torch.bfloat16 else _FANIN_F32
    for s in srcs:
        if not s.is_contiguous():
            raise ValueError("fan-in sources must be contiguous")
        if s.device != device:
            raise ValueError("fan-in sources and outputs must live on the "
                             "same device")
    return tag


def _fanin_device_args(n: int, srcs, tag: int, outs):
    """Alignment checks of the vector kernels and the host pointer array."""
    import ctypes
    if n % 4:
        raise ValueError("flat buffers must be padded to a multiple of 4")
    # payload byte buffers: q8 4 B (char4 quants, f32 scales), top-k 2 B
    # (bf16 values); raw sources are read as whole quads
    align = {_FANIN_F32: 16, _FANIN_BF16: 8, _FANIN_Q8: 4, _FANIN_TOPK: 2}[tag]
    for s in srcs:
        if s.data_ptr() % align:
            raise ValueError(f"fan-in source must be {align}-byte aligned")
    for name, t in outs:
        if t is not None and t.data_ptr() % (4 * t.element_size()):
            raise ValueError(f"{name} must be aligned to 4 elements")
    return (ctypes.c_void_p * FANIN_MAX_SRCS)(*[s.data_ptr() for s in srcs])


def _fanin_raise(entry: str, rc: int, nsrc: int, codec: str, k, n: int):
    raise RuntimeError(f"{entry} launched nothing (code {rc}): nsrc={nsrc}, "
                       f"codec={codec!r}, k={k!r}, n={n}")


def fanin_reduce(dst: torch.Tensor, srcs, codec: str, k=None) -> None:
    """dst (f32) = the sum of the decoded `srcs` taken strictly in list
    order, starting from +0 (an empty list zero-fills). codec: 'raw' (f32 or
    bf16 tensors of dst's numel), 'q8' (pack_q8 payloads) or 'topk'
    (pack_topk_ef payloads at `k` per block)."""
    n = dst.numel()
    srcs = list(srcs)
    if dst.dtype != torch.float32:
        raise TypeError("fan-in destination must be f32")
    _check_flat(dst, "dst", n)
    tag = _fanin_check(n, dst.device, srcs, codec, k)
    if dst.is_cuda:
        ptrs = _fanin_device_args(n, srcs, tag, [("dst", dst)])
        rc = require_lib().ps_fanin_reduce(
            dst.data_ptr(), ptrs, len(srcs), tag,
            int(k) if codec == 'topk' else 0, n, current_stream_ptr())
        if rc:
            _fanin_raise('ps_fanin_reduce', rc, len(srcs), codec, k, n)
        return
    s = torch.zeros(n, dtype=torch.float32)
    if codec == 'topk':
        off, _ = topk_layout(n, k)
        nblk = off // k
        base = torch.arange(nblk, dtype=torch.int64) * TOPK_BLOCK
    elif codec == 'q8':
        qb, _ = q8_layout(n)
        nblk = (n + Q8_BLOCK - 1) // Q8_BLOCK
    for p in srcs:
        if codec == 'topk':
            idx = p[:off].view(nblk, k).to(torch.int64)
            vals = p[off:].clone().view(torch.bfloat16).view(nblk, k).to(
                torch.float32)
            for j in range(k):
                # one entry per block: positions within a pass are distinct
                pos = base + idx[:, j]
                live = pos < n
                s[pos[live]] += vals[:, j][live]
        elif codec == 'q8':
            q = p[:n].view(torch.int8).to(torch.float32)
            scales = p[qb:qb + 4 * nblk].clone().view(torch.float32)
            dec = q * scales.repeat_interleave(Q8_BLOCK)[:n]   # rounded once
            s = s + dec                                        # then the add
        else:
            s = s + p.to(torch.float32)
    dst.copy_(s)


def fanin_sgd(w: torch.Tensor, m: torch.Tensor, srcs, codec: str, k,
              lr: float, momentum: float = 0.0, weight_decay: float = 0.0,
              grad_scale: float = 1.0, nesterov: bool = False,
              wire_out: Optional[torch.Tensor] = None) -> None:
    """fanin_reduce followed by fused_sgd_step on the sum; on the GPU one
    launch in which the sum never reaches memory. Bitwise equal to the
    two-step form."""
    n = w.numel()
    srcs = list(srcs)
    if w.dtype != torch.float32 or m.dtype != torch.float32:
        raise TypeError("master weights and momentum must be f32")
    _check_flat(w, "w", n)
    _check_flat(m, "momentum_buf", n)
    if wire_out is not None:
        _check_flat(wire_out, "wire_out", n)
    tag = _fanin_check(n, w.device, srcs, codec, k)
    if w.is_cuda:
        ptrs = _fanin_device_args(n, srcs, tag, [("w", w), ("m", m),
                                                 ("wire_out", wire_out)])
        rc = require_lib().ps_fanin_sgd(
            w.data_ptr(), m.data_ptr(),
            0 if wire_out is None else wire_out.data_ptr(),
            dtype_tag(wire_out.dtype) if wire_out is not None else 0,
            ptrs, len(srcs), tag, int(k) if codec == 'topk' else 0, n,
            float(lr), float(momentum), float(weight_decay),
            float(grad_scale), int(nesterov), current_stream_ptr())
        if rc:
            _fanin_raise('ps_fanin_sgd', rc, len(srcs), codec, k, n)
        return
    g = torch.empty(n, dtype=torch.float32)
    fanin_reduce(g, srcs, codec, k)
    fused_sgd_step(w, g, m, lr, momentum, weight_decay, grad_scale, nesterov,
                   wire_out)


# ---- counter-based dropout (CPU oracle for ops/kernels/dropout.hip) ----
# Philox4x32-10; element e takes word (e & 3) of the block whose counter is
# (lo32(e>>2), hi32(e>>2), step, (stream << 16) | salt) under key
# (lo32(seed), hi32(seed)); keep iff word >= round(p * 2^32). Everything is
# integer arithmetic, so the masks equal the kernel's bit for bit.

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 on uint32 words: counter [..., 4], key [..., 2] (numpy
    broadcastable) -> uint32 [..., 4]."""
    import numpy as np
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(_U32)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(_U32)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = k[..., 0], k[..., 1]
    m32 = np.uint64(_U32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(_PHILOX_M0) * c0     # 32x32 -> 64: exact in uint64
        p1 = np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0, p1 & m32,
                          (p0 >> s32) ^ c3 ^ k1, p0 & m32)
        k0 = (k0 + np.uint64(_PHILOX_W0)) & m32
        k1 = (k1 + np.uint64(_PHILOX_W1)) & m32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3),
                    axis=-1).astype(np.uint32)


def dropout_threshold(p: float) -> int:
    """thr = round(p * 2^32) as a uint32: keep iff word >= thr. 0 keeps
    everything; p >= 1 is not representable and is handled by the callers."""
    return min(max(int(round(float(p) * 4294967296.0)), 0), _U32)


def dropout_salt_stream(salt: int, stream: int) -> int:
    return ((int(stream) & 0xFFFF) << 16) | (int(salt) & 0xFFFF)


def dropout_keep_mask(n: int, p: float, seed: int, salt: int = 0,
                      stream: int = 0, step: int = 0) -> torch.Tensor:
    """bool [n]: True where the dropout kernel keeps element e."""
    import numpy as np
    if p >= 1.0:
        return torch.zeros(n, dtype=torch.bool)
    thr = dropout_threshold(p)
    if thr == 0:
        return torch.ones(n, dtype=torch.bool)
    blk = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.empty((blk.size, 4), dtype=np.uint64)
    ctr[:, 0] = blk & np.uint64(_U32)
    ctr[:, 1] = blk >> np.uint64(32)
    ctr[:, 2] = int(step) & _U32
    ctr[:, 3] = dropout_salt_stream(salt, stream)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10(ctr, [seed & _U32, seed >> 32]).reshape(-1)[:n]
    return torch.from_numpy(words >= np.uint32(thr))


def dropout_scale(p: float) -> float:
    """float32(1/(1-p)); 0.0 encodes p >= 1 (everything dropped)."""
    if p >= 1.0:
        return 0.0
    return float(torch.tensor(1.0 / (1.0 - float(p)), dtype=torch.float32))


def act_drop_ref(x: torch.Tensor, keep: torch.Tensor, scale: float,
                 relu: bool):
    """Reference forward of the act-drop kernel: returns (y, bits) with
    y = bits ? T(float(x) * scale) : 0 and bits = keep & (!relu | x > 0),
    in the kernel's order (float32 multiply, then round to x.dtype)."""
    xf = x.detach().to(torch.float32)
    bits = keep.reshape(x.shape).to(x.device)
    if relu:
        bits = bits & (xf > 0)
    s = torch.tensor(scale, dtype=torch.float32, device=x.device)
    y = torch.where(bits, (xf * s).to(x.dtype), torch.zeros((), dtype=x.dtype,
                                                           device=x.device))
    return y, bits


def act_drop_bwd_ref(dy: torch.Tensor, bits: torch.Tensor,
                     scale: float) -> torch.Tensor:
    """dx = bits ? T(float(dy) * scale) : 0."""
    s = torch.tensor(scale, dtype=torch.float32, device=dy.device)
    dx = (dy.to(torch.float32) * s).to(dy.dtype)
    return torch.where(bits.reshape(dy.shape), dx,
                       torch.zeros((), dtype=dy.dtype, device=dy.device))


def pack_mask_bits(bits: torch.Tensor) -> torch.Tensor:
    """bool [n] -> uint8 [(n+7)//8] in the kernels' layout (bit k of byte i
    is element 8*i+k)."""
    import numpy as np
    b = bits.reshape(-1).cpu().numpy()
    return torch.from_numpy(np.packbits(b, bitorder='little'))


# ---- fused augmentation loader (CPU oracle for ops/kernels/augment.hip) ----
# Per batch slot b one Philox block: counter (b, 0, lo32(step),
# (stream << 16) | 0xDA7A), key (lo32(seed), hi32(seed));
# oy = (w0 * (2p+1)) >> 32, ox = (w1 * (2p+1)) >> 32, flip = hflip & (w2 >> 31).

AUGMENT_SALT = 0xDA7A


def augment_draws(B: int, pad: int, hflip: bool, seed: int, stream: int = 0,
                  step: int = 0):
    """(oy, ox, flip) of the B batch slots: int64 [B], int64 [B], bool [B];
    offsets are uniform on 0..2*pad, flip is a fair coin (False without
    hflip)."""
    import numpy as np
    ctr = np.zeros((B, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(B, dtype=np.uint64)
    ctr[:, 2] = int(step) & _U32
    ctr[:, 3] = dropout_salt_stream(AUGMENT_SALT, stream)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(ctr, [seed & _U32, seed >> 32]).astype(np.uint64)
    span = np.uint64(2 * int(pad) + 1)
    oy = ((w[:, 0] * span) >> np.uint64(32)).astype(np.int64)
    ox = ((w[:, 1] * span) >> np.uint64(32)).astype(np.int64)
    flip = (w[:, 2] >> np.uint64(31)).astype(bool) & bool(hflip)
    return torch.from_numpy(oy), torch.from_numpy(ox), torch.from_numpy(flip)


def _augment_src(o, flip, L: int, pad: int, reflect: bool):
    """Source coordinate [B, L] along one axis and its in-range mask."""
    ar = torch.arange(L, device=o.device).view(1, L)
    if flip is not None:
        ar = torch.where(flip.view(-1, 1), L - 1 - ar, ar)
    s = o.view(-1, 1) + ar - pad
    if reflect:
        s = torch.where(s < 0, -s, s)
        s = torch.where(s >= L, 2 * (L - 1) - s, s)
        return s, torch.ones_like(s, dtype=torch.bool)
    ok = (s >= 0) & (s < L)
    return s.clamp(0, L - 1), ok


def augment_ref(x_u8: torch.Tensor, y: torch.Tensor, idx: torch.Tensor,
                mean255, inv_std255, pad: int = 0, pad_mode=None,
                hflip: bool = False, draws=None,
                dtype: torch.dtype = torch.float32):
    """Reference of the augment kernel in index arithmetic: output pixel
    (b, h, w) reads source (oy + h - pad, ox + w' - pad), w' = W-1-w where
    flipped, reflected back into the image (pad_mode 'reflect') or replaced
    by uint8 0 ('constant'), then T((float(u8) - mean255[c]) * inv_std255[c])
    with both operations rounded to f32. `draws` = (oy, ox, flip) from
    augment_draws, or None for a plain gather + normalize. Returns the
    [B,C,H,W] batch in channels-last memory and the labels."""
    dev = x_u8.device
    B = idx.numel()
    _, C, H, W = x_u8.shape
    if draws is None:
        pad = 0
        oy = ox = torch.zeros(B, dtype=torch.int64, device=dev)
        flip = None
    else:
        oy, ox, flip = (t.to(dev) for t in draws)
    sy, oky = _augment_src(oy, None, H, pad, pad_mode == 'reflect')
    sx, okx = _augment_src(ox, flip, W, pad, pad_mode == 'reflect')
    idx = idx.to(dev)
    # advanced indices split by the channel slice -> [B, H, W, C]
    u = x_u8[idx.view(B, 1, 1), :, sy.view(B, H, 1), sx.view(B, 1, W)].float()
    ok = oky.view(B, H, 1, 1) & okx.view(B, 1, W, 1)
    u = torch.where(ok, u, torch.zeros((), device=dev))
    mean = torch.as_tensor(mean255, dtype=torch.float32, device=dev).view(C)
    inv = torch.as_tensor(inv_std255, dtype=torch.float32, device=dev).view(C)
    out = ((u - mean) * inv).to(dtype)
    return out.permute(0, 3, 1, 2), y.index_select(0, idx)


# ---- fused loss + prec@k (CPU oracle for ops/kernels/metrics.hip) ----
# rank(m) = #{c != t : x[c] > x[t] or isnan(x[c])} + #{c < t : x[c] == x[t]}:
# ties go to the lower class index, so the count never depends on a sort's
# tie order. Row m is a hit at k iff rank(m) < min(k, C); a NaN at the target
# misses at every k; a row whose target is outside [0, C) is invalid — never
# used as an index, worth 0 in the loss sum and in every hit count, and
# counted on its own.

METRIC_MAX_KS = 4


def check_ks(ks) -> tuple:
    ks = tuple(int(k) for k in ks)
    if not 1 <= len(ks) <= METRIC_MAX_KS:
        raise ValueError(f"between 1 and {METRIC_MAX_KS} values of k, "
                         f"got {len(ks)}")
    if any(k < 1 for k in ks):
        raise ValueError(f"every k must be >= 1, got {ks}")
    return ks


def ce_topk_reference(logits: torch.Tensor, target: torch.Tensor,
                      ks=(1, 5)):
    """(loss_sum f64 [], hits i64 [len(ks)], rows i64 [], invalid i64 []) of
    one [M, C] batch by the rule above, in plain torch on the logits' device
    and without a host sync; the row loss is float64 log-sum-exp minus the
    target logit. `rows` counts the valid rows."""
    ks = check_ks(ks)
    if logits.dim() != 2:
        raise ValueError(f"logits must be [M, C], got {tuple(logits.shape)}")
    x = logits.detach()
    M, C = x.shape
    t = target.detach().to(device=x.device, dtype=torch.int64).reshape(M)
    valid = (t >= 0) & (t < C)
    tc = t.clamp(0, max(C - 1, 0)).view(M, 1)
    xt = x.gather(1, tc)
    idx = torch.arange(C, device=x.device).view(1, C)
    above = ((x > xt) | torch.isnan(x)) & (idx != tc)
    tie = (x == xt) & (idx < tc)
    rank = above.sum(1) + tie.sum(1)
    rank = torch.where(torch.isnan(xt.view(M)), torch.full_like(rank, C), rank)
    hits = torch.stack([((rank < min(k, C)) & valid).sum() for k in ks])
    x64 = x.to(torch.float64)
    row = torch.logsumexp(x64, dim=1) - xt.view(M).to(torch.float64)
    loss_sum = torch.where(valid, row, torch.zeros_like(row)).sum()
    rows = valid.sum()
    return loss_sum, hits, rows, M - rows
