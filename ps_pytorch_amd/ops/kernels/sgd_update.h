// Per-element arithmetic of the PS-side SGD/momentum update, shared by
// fused_sgd.hip (update of a materialised gradient sum) and fanin.hip
// (update fused behind the rank-ordered fan-in), so both round alike:
//
//   g   = s * scale            (+ wd * w, one fma, only where has_wd)
//   m   = fma(mu, m, g)
//   upd = nesterov ? fma(mu, m, g) : m
//   w   = fma(-lr, upd, w)
//
// has_wd / nesterov are compile-time constants in fused_sgd.hip and
// wave-uniform runtime flags in fanin.hip; the operations are the same.
#pragma once
#include "common.h"

__device__ __forceinline__ void sgd_update_elem(
    float& w, float& m, float s, float scale, float lr, float mu, float wd,
    bool has_wd, bool nesterov)
{
    float gk = s * scale;
    if (has_wd) gk = fmaf(wd, w, gk);
    float mk = fmaf(mu, m, gk);
    m = mk;
    float upd = nesterov ? fmaf(mu, mk, gk) : mk;
    w = fmaf(-lr, upd, w);
}

// Per-element arithmetic of the LARS update (lars.hip). The step size llr
// (= lr * trust ratio) and the decay wds are per tensor, so the learning
// rate is folded into the momentum buffer, as usual for LARS:
//
//   g = s * scale              (+ wds * w, one fma, only where wds != 0)
//   m = fma(mu, m, llr * g)
//   w = w - m
__device__ __forceinline__ void lars_update_elem(
    float& w, float& m, float s, float scale, float llr, float mu, float wds)
{
    float gk = s * scale;
    if (wds != 0.0f) gk = fmaf(wds, w, gk);
    float mk = fmaf(mu, m, llr * gk);
    m = mk;
    w = w - mk;
}
