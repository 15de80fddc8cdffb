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
