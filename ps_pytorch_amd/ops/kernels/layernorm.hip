// Channel LayerNorm, exact-erf GELU and layer-scale + residual for NHWC
// activations: the three steps of a ConvNeXt block between its convolutions.
//
// Layout: x is [M][C], M = N*H*W pixels, C innermost, bf16 or f32; gamma,
// beta, lambda and their gradients in the type of x. All arithmetic is f32,
// bf16 is storage only, every output is rounded once. Envelope of the row
// kernels: C % 8 == 0, 8 <= C <= 2048, M >= 1; of GELU: n % 8 == 0.
//
// Lane-group map (LayerNorm forward / backward, layer scale): a row is
// C/VEC 16-B granules (VEC = 8 bf16 or 4 f32). A lane group of LG lanes, the
// smallest of 8 / 16 / 32 / 64 that is >= the granule count (64 above), owns
// one row; lane l holds granules l, l + LG, ... (NG <= 4 at bf16, <= 8 at
// f32) IN REGISTERS. A wave holds 64/LG rows, a 256-thread block 256/LG rows
// per pass. Lanes whose granule index is >= C/VEC are idle: they load
// nothing, contribute +0 and store nothing. A row sum is the lane's own
// granules in ascending order (elements 0..VEC-1 in order), then an xor
// butterfly over the group with offsets 1, 2, ..., LG/2; a + b == b + a bit
// for bit, so every lane of the group ends with the same sum and there is no
// broadcast, no LDS and no barrier in the forward.
//
// A block owns ONE contiguous chunk of rows_per_block rows (never a
// grid-strided set: the DRAM-page reason recorded under bn_stats_kernel).
// The host picks (rows_per_block, blocks) in ops/modules.py:_ln_plan, the
// only place that rule lives; the launch functions take it as given and
// reject a plan that breaks the kernels' invariants.
//
// LayerNorm, per row (two-pass: the row is in registers):
//   m0 = (sum x)/C, d = x - m0, dm = (sum d)/C, xc = d - dm   (mean refined
//   once: m0's rounding error scales with |x|; sum d is a compensated sum)
//   mean = m0 + dm, var = (sum xc^2)/C, invstd = rsqrtf(var + eps)
//   y = xc*invstd*gamma + beta
//   (one f32 mean cannot hold the refined centre: the saved mean and invstd
//   alone do not reproduce the forward's x-hat bit for bit, the backward
//   repeats the remainder step)
//   backward  d = x - mean (saved), xc = d - (sum d)/C, xh = xc*invstd,
//             g = gamma*dy
//             c1 = (sum g)/C, c2 = (sum g*xh)/C
//             dx = invstd*(g - c1 - xh*c2)
//             dbeta_c = sum_rows dy, dgamma_c = sum_rows dy*xh
// Layer scale: out = res + lambda_c*y (one fma); dy = lambda_c*dout,
//             dlambda_c = sum_rows dout*y; dres is dout itself.
// Column sums: per-lane f32 accumulators over the block's rows, folded over
// the block's row slots through LDS in ascending order -> partial[block][.][C]
// -> ln_param_fold_kernel adds the blocks 0, 1, ... in order. No atomics;
// two runs are bit-identical.
#include "common.h"

template <typename T> struct LnGran;
template <> struct LnGran<unsigned short> {
    static constexpr int VEC = 8;
    static __device__ __forceinline__ void unpack(uint4 r, float* v) {
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(w[i] << 16);
            v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ uint4 pack(const float* v) {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = (unsigned)f32_to_bf16(v[2 * i]) |
                   ((unsigned)f32_to_bf16(v[2 * i + 1]) << 16);
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
    static __device__ __forceinline__ unsigned short round(float v) { return f32_to_bf16(v); }
};
template <> struct LnGran<float> {
    static constexpr int VEC = 4;
    static __device__ __forceinline__ void unpack(uint4 r, float* v) {
        v[0] = __uint_as_float(r.x); v[1] = __uint_as_float(r.y);
        v[2] = __uint_as_float(r.z); v[3] = __uint_as_float(r.w);
    }
    static __device__ __forceinline__ uint4 pack(const float* v) {
        return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]),
                          __float_as_uint(v[2]), __float_as_uint(v[3]));
    }
    static __device__ __forceinline__ float round(float v) { return v; }
};

// the granules l, l + LG, ... of one row (or of a parameter vector); idle
// lanes and inactive rows get +0 bits and touch no memory
template <typename T, int LG, int NG>
__device__ __forceinline__ void ln_load_row(const T* __restrict__ row, int l,
                                            int G, bool active, uint4 (&raw)[NG])
{
    constexpr int VEC = LnGran<T>::VEC;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int g = l + k * LG;
        raw[k] = (active && g < G) ? *(const uint4*)(row + g * VEC)
                                   : make_uint4(0u, 0u, 0u, 0u);
    }
}

// xor butterfly over the lane group; offsets < LG never leave the group
template <int LG>
__device__ __forceinline__ float ln_group_sum(float s)
{
#pragma unroll
    for (int o = 1; o < LG; o <<= 1) s += __shfl_xor(s, o);
    return s;
}

// The remainder sum of the centred row, sum (x - m0), is the one sum whose
// ABSOLUTE error reaches y: where x is at the mean and beta near 0 nothing
// else is left of y. It is carried as (sum, error term) by Knuth's two-sum,
// in the lane and through the butterfly; the error of an add is computed
// exactly, so both lanes of a pair still end with the same bits.
__device__ __forceinline__ void ln_two_sum(float& s, float& c, float b)
{
    const float t = s + b;
    const float bb = t - s;
    c += (s - (t - bb)) + (b - bb);
    s = t;
}

template <int LG>
__device__ __forceinline__ float ln_group_sum_comp(float s, float c)
{
#pragma unroll
    for (int o = 1; o < LG; o <<= 1) {
        const float so = __shfl_xor(s, o), co = __shfl_xor(c, o);
        const float t = s + so;
        const float bb = t - s;
        c = (c + co) + ((s - (t - bb)) + (so - bb));
        s = t;
    }
    return s + c;
}

// ---------------- LayerNorm forward ----------------
// U rows per lane group are loaded before the first is reduced, so a lane
// has about four 16-B loads in flight whatever NG is.
template <typename T, int LG, int NG>
__global__ __launch_bounds__(256) void ln_fwd_kernel(
    const T* __restrict__ x, T* __restrict__ y, const T* __restrict__ gamma,
    const T* __restrict__ beta, float* __restrict__ save_mean,
    float* __restrict__ save_invstd, long M, int C, int rpb, float eps)
{
    constexpr int VEC = LnGran<T>::VEC, RP = 256 / LG;
    constexpr int U = NG == 1 ? 4 : NG == 2 ? 2 : 1;
    const int G = C / VEC;
    const int l = threadIdx.x % LG, rg = threadIdx.x / LG;
    const long r0 = (long)blockIdx.x * rpb;
    const long r1 = r0 + rpb < M ? r0 + rpb : M;
    const float fc = (float)C;
    uint4 gr[NG], br[NG];
    ln_load_row<T, LG, NG>(gamma, l, G, true, gr);
    ln_load_row<T, LG, NG>(beta, l, G, true, br);

    for (long base = r0; base < r1; base += U * RP) {
        uint4 raw[U][NG];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = base + u * RP + rg;
            ln_load_row<T, LG, NG>(x + row * C, l, G, row < r1, raw[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = base + u * RP + rg;
            const bool active = row < r1;
            float v[NG][VEC];
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                LnGran<T>::unpack(raw[u][k], v[k]);
#pragma unroll
                for (int i = 0; i < VEC; ++i) s += v[k][i];
            }
            const float m0 = ln_group_sum<LG>(s) / fc;
            float e = 0.f, ec = 0.f;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                if (l + k * LG < G) {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        v[k][i] -= m0;
                        ln_two_sum(e, ec, v[k][i]);
                    }
                }
            }
            // the rounding error of m0 scales with |x|: take the remainder
            // off the centred values
            const float dm = ln_group_sum_comp<LG>(e, ec) / fc;
            const float mean = m0 + dm;
            float q = 0.f;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                if (l + k * LG < G) {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        v[k][i] -= dm;
                        q += v[k][i] * v[k][i];
                    }
                }
            }
            const float invstd = rsqrtf(ln_group_sum<LG>(q) / fc + eps);
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                const int g = l + k * LG;
                if (active && g < G) {
                    float ga[VEC], be[VEC];
                    LnGran<T>::unpack(gr[k], ga);
                    LnGran<T>::unpack(br[k], be);
#pragma unroll
                    for (int i = 0; i < VEC; ++i)
                        v[k][i] = v[k][i] * invstd * ga[i] + be[i];
                    *(uint4*)(y + row * C + g * VEC) = LnGran<T>::pack(v[k]);
                }
            }
            if (save_mean && active && l == 0) {
                save_mean[row] = mean;
                save_invstd[row] = invstd;
            }
        }
    }
}

// ---------------- column-sum core ----------------
// Fold the per-lane channel accumulators acc[NG][VEC] of the block's 256/LG
// row slots (thread t = rg*LG + l) in ascending rg, i.e. the lane groups of
// wave 0, then wave 1, ..., and write the totals of channels < C to dst[C].
// red is [256][VEC+1] floats. Bank argument: thread t writes dword
// t*(VEC+1) + i; for one i the 64 lanes of a wave are consecutive t, so
// their addresses step by VEC+1 = 9 (or 5) dwords: odd, hence coprime with
// the power-of-two bank count, and every lane lands on its own bank. The
// readers are the lanes of row slot 0 (t = l < LG, consecutive again), lane
// l reading dword (s*LG + l)*(VEC+1) + i for slot s: the same odd step.
// Without the padded column the step would be 8 (4) dwords and a pass would
// pile 8-way (4-way) onto an eighth (a quarter) of the banks.
template <int VEC, int LG, int NG>
__device__ __forceinline__ void ln_col_fold(float* red, const float (&acc)[NG][VEC],
                                            float* __restrict__ dst, int l,
                                            int rg, int G)
{
    constexpr int RS = VEC + 1, RP = 256 / LG;
    float* mine = red + threadIdx.x * RS;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) mine[i] = acc[k][i];
        __syncthreads();
        const int g = l + k * LG;
        if (rg == 0 && g < G) {
            float t[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) t[i] = mine[i];
            for (int s = 1; s < RP; ++s) {
                const float* o = mine + s * LG * RS;
#pragma unroll
                for (int i = 0; i < VEC; ++i) t[i] += o[i];
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) dst[g * VEC + i] = t[i];
        }
        __syncthreads();
    }
}

// partial is [nblk][ncols]; columns < C go to out0, the rest to out1 (ncols
// is C or 2C). A block owns 64 columns and adds the rows 0, 1, ... in order:
// 64 rows at a time are staged in LDS by all 256 threads (coalesced 256-B row
// segments), then thread j < 64 walks its column top to bottom (lane-linear
// LDS reads). One rounding to the parameter type at the end.
template <typename PT>
__global__ __launch_bounds__(256) void ln_param_fold_kernel(
    const float* __restrict__ partial, PT* __restrict__ out0,
    PT* __restrict__ out1, int nblk, int C, int ncols)
{
    __shared__ float stage[64 * 64];
    const int j = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + j;
    const bool live = col < ncols;
    float acc = 0.f;
    for (int b0 = 0; b0 < nblk; b0 += 64) {
        const int rows = nblk - b0 < 64 ? nblk - b0 : 64;
        for (int r = w; r < rows; r += 4)
            stage[r * 64 + j] = live ? partial[(long)(b0 + r) * ncols + col] : 0.f;
        __syncthreads();
        if (w == 0)
            for (int r = 0; r < rows; ++r) acc += stage[r * 64 + j];
        __syncthreads();
    }
    if (w == 0 && live) {
        if (col < C) out0[col] = LnGran<PT>::round(acc);
        else out1[col - C] = LnGran<PT>::round(acc);
    }
}

// ---------------- LayerNorm backward ----------------
template <typename T, int LG, int NG>
__global__ __launch_bounds__(256) void ln_bwd_kernel(
    const T* __restrict__ x, const T* __restrict__ dy,
    const T* __restrict__ gamma, const float* __restrict__ save_mean,
    const float* __restrict__ save_invstd, T* __restrict__ dx,
    float* __restrict__ partial, long M, int C, int rpb)
{
    constexpr int VEC = LnGran<T>::VEC, RP = 256 / LG;
    constexpr int U = NG == 1 ? 2 : 1;
    __shared__ float red[256 * (VEC + 1)];
    const int G = C / VEC;
    const int l = threadIdx.x % LG, rg = threadIdx.x / LG;
    const long r0 = (long)blockIdx.x * rpb;
    const long r1 = r0 + rpb < M ? r0 + rpb : M;
    const float fc = (float)C;
    uint4 gr[NG];
    ln_load_row<T, LG, NG>(gamma, l, G, true, gr);
    float ab[NG][VEC], ag[NG][VEC];       // dbeta, dgamma of my channels
#pragma unroll
    for (int k = 0; k < NG; ++k)
#pragma unroll
        for (int i = 0; i < VEC; ++i) { ab[k][i] = 0.f; ag[k][i] = 0.f; }

    for (long base = r0; base < r1; base += U * RP) {
        uint4 rx[U][NG], rd[U][NG];
        float mu[U], iv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = base + u * RP + rg;
            const bool active = row < r1;
            ln_load_row<T, LG, NG>(x + row * C, l, G, active, rx[u]);
            ln_load_row<T, LG, NG>(dy + row * C, l, G, active, rd[u]);
            mu[u] = active ? save_mean[row] : 0.f;
            iv[u] = active ? save_invstd[row] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = base + u * RP + rg;
            const bool active = row < r1;
            float xh[NG][VEC], gg[NG][VEC];
            // the saved mean is one f32: the remainder of the centred row
            // is taken off as in the forward
            float e = 0.f, ec = 0.f;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                LnGran<T>::unpack(rx[u][k], xh[k]);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    xh[k][i] = (active && l + k * LG < G) ? xh[k][i] - mu[u] : 0.f;
                    ln_two_sum(e, ec, xh[k][i]);
                }
            }
            const float dm = ln_group_sum_comp<LG>(e, ec) / fc;
            float s1 = 0.f, s2 = 0.f;
            // idle lanes and inactive rows: dy and gamma are +0, so every
            // product below is a zero and adds nothing
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                float dv[VEC], ga[VEC];
                LnGran<T>::unpack(rd[u][k], dv);
                LnGran<T>::unpack(gr[k], ga);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    xh[k][i] = (xh[k][i] - dm) * iv[u];
                    ab[k][i] += dv[i];
                    ag[k][i] += dv[i] * xh[k][i];
                    gg[k][i] = ga[i] * dv[i];
                    s1 += gg[k][i];
                    s2 += gg[k][i] * xh[k][i];
                }
            }
            const float c1 = ln_group_sum<LG>(s1) / fc;
            const float c2 = ln_group_sum<LG>(s2) / fc;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                const int g = l + k * LG;
                if (active && g < G) {
#pragma unroll
                    for (int i = 0; i < VEC; ++i)
                        gg[k][i] = iv[u] * (gg[k][i] - c1 - xh[k][i] * c2);
                    *(uint4*)(dx + row * C + g * VEC) = LnGran<T>::pack(gg[k]);
                }
            }
        }
    }
    float* prow = partial + (long)blockIdx.x * 2 * C;
    ln_col_fold<VEC, LG, NG>(red, ab, prow, l, rg, G);
    ln_col_fold<VEC, LG, NG>(red, ag, prow + C, l, rg, G);
}

// ---------------- layer scale + residual ----------------
template <typename T, int LG, int NG>
__global__ __launch_bounds__(256) void lscale_fwd_kernel(
    const T* __restrict__ y, const T* __restrict__ res,
    const T* __restrict__ lam, T* __restrict__ out, long M, int C, int rpb)
{
    constexpr int VEC = LnGran<T>::VEC, RP = 256 / LG;
    constexpr int U = NG == 1 ? 2 : 1;
    const int G = C / VEC;
    const int l = threadIdx.x % LG, rg = threadIdx.x / LG;
    const long r0 = (long)blockIdx.x * rpb;
    const long r1 = r0 + rpb < M ? r0 + rpb : M;
    uint4 lr[NG];
    ln_load_row<T, LG, NG>(lam, l, G, true, lr);
    for (long base = r0; base < r1; base += U * RP) {
        uint4 ry[U][NG], rr[U][NG];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = base + u * RP + rg;
            ln_load_row<T, LG, NG>(y + row * C, l, G, row < r1, ry[u]);
            ln_load_row<T, LG, NG>(res + row * C, l, G, row < r1, rr[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = base + u * RP + rg;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                const int g = l + k * LG;
                if (row < r1 && g < G) {
                    float yv[VEC], rv[VEC], lv[VEC];
                    LnGran<T>::unpack(ry[u][k], yv);
                    LnGran<T>::unpack(rr[u][k], rv);
                    LnGran<T>::unpack(lr[k], lv);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) yv[i] = fmaf(lv[i], yv[i], rv[i]);
                    *(uint4*)(out + row * C + g * VEC) = LnGran<T>::pack(yv);
                }
            }
        }
    }
}

template <typename T, int LG, int NG>
__global__ __launch_bounds__(256) void lscale_bwd_kernel(
    const T* __restrict__ y, const T* __restrict__ dout,
    const T* __restrict__ lam, T* __restrict__ dy,
    float* __restrict__ partial, long M, int C, int rpb)
{
    constexpr int VEC = LnGran<T>::VEC, RP = 256 / LG;
    constexpr int U = NG == 1 ? 2 : 1;
    __shared__ float red[256 * (VEC + 1)];
    const int G = C / VEC;
    const int l = threadIdx.x % LG, rg = threadIdx.x / LG;
    const long r0 = (long)blockIdx.x * rpb;
    const long r1 = r0 + rpb < M ? r0 + rpb : M;
    uint4 lr[NG];
    ln_load_row<T, LG, NG>(lam, l, G, true, lr);
    float al[NG][VEC];
#pragma unroll
    for (int k = 0; k < NG; ++k)
#pragma unroll
        for (int i = 0; i < VEC; ++i) al[k][i] = 0.f;
    for (long base = r0; base < r1; base += U * RP) {
        uint4 ry[U][NG], rd[U][NG];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = base + u * RP + rg;
            ln_load_row<T, LG, NG>(y + row * C, l, G, row < r1, ry[u]);
            ln_load_row<T, LG, NG>(dout + row * C, l, G, row < r1, rd[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = base + u * RP + rg;
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                const int g = l + k * LG;
                float yv[VEC], dv[VEC], lv[VEC];
                LnGran<T>::unpack(ry[u][k], yv);
                LnGran<T>::unpack(rd[u][k], dv);
                LnGran<T>::unpack(lr[k], lv);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    al[k][i] += dv[i] * yv[i];      // +0 where nothing was loaded
                    dv[i] *= lv[i];
                }
                if (row < r1 && g < G)
                    *(uint4*)(dy + row * C + g * VEC) = LnGran<T>::pack(dv);
            }
        }
    }
    ln_col_fold<VEC, LG, NG>(red, al, partial + (long)blockIdx.x * C, l, rg, G);
}

// ---------------- GELU (exact erf form) ----------------
// One 16-B granule per lane per trip. The kernels are bound by the erff /
// expf arithmetic, not by loads in flight: several granules per trip were
// measured and bought nothing (profiles/r19_layernorm.md).
template <typename T>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(
    const T* __restrict__ x, T* __restrict__ y, long nvec)
{
    constexpr int VEC = LnGran<T>::VEC;
    EW_IDX
    for (long i = gid; i < nvec; i += stride) {
        float v[VEC];
        LnGran<T>::unpack(*(const uint4*)(x + i * VEC), v);
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            v[k] = 0.5f * v[k] * (1.f + erff(v[k] * 0.70710678f));
        *(uint4*)(y + i * VEC) = LnGran<T>::pack(v);
    }
}

// dx = dy * (Phi(x) + x*phi(x)), recomputed from the saved x
template <typename T>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(
    const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
    long nvec)
{
    constexpr int VEC = LnGran<T>::VEC;
    EW_IDX
    for (long i = gid; i < nvec; i += stride) {
        float v[VEC], d[VEC];
        LnGran<T>::unpack(*(const uint4*)(x + i * VEC), v);
        LnGran<T>::unpack(*(const uint4*)(dy + i * VEC), d);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float cdf = 0.5f * (1.f + erff(v[k] * 0.70710678f));
            const float pdf = expf(-0.5f * v[k] * v[k]) * 0.3989422804f;
            d[k] = d[k] * (cdf + v[k] * pdf);
        }
        *(uint4*)(dx + i * VEC) = LnGran<T>::pack(d);
    }
}

// ---------------- C API ----------------
#define LN_MAX_GRID (1L << 20)

static bool ln_envelope(long M, long C, int dtype) {
    if (dtype != PS_F32 && dtype != PS_BF16) return false;
    return M >= 1 && C >= 8 && C <= 2048 && C % 8 == 0;
}

static int ln_lane_group(long C, int elt) {
    const long G = C / (16 / elt);
    return G <= 8 ? 8 : G <= 16 ? 16 : G <= 32 ? 32 : 64;
}

// The invariants of a plan (not the choice among plans). Every row is guarded
// by row < r1, so blocks*rpb >= M is the one the kernels need for coverage;
// rpb a multiple of the rows a block handles at once keeps whole passes.
// blocks is bounded by the grid limit only: the CALLER sizes `partial` for
// the blocks it passes (blocks*2*C floats for ps_ln_bwd, blocks*C for
// ps_lscale_bwd); _ln_plan caps blocks at 512.
static bool ln_plan_ok(long M, long C, int elt, long rpb, long blocks) {
    const long unit = 256 / ln_lane_group(C, elt);
    return rpb >= unit && rpb % unit == 0 && rpb <= (1L << 30) &&
           blocks >= 1 && blocks <= LN_MAX_GRID && blocks * rpb >= M;
}

template <int V> struct LnInt { static constexpr int value = V; };

// f(LG, NG) for the lane-group map of C channels of type T
template <typename T, typename F>
static int ln_dispatch(int C, F&& f)
{
    const int G = C / LnGran<T>::VEC;
    if (G <= 8) return f(LnInt<8>{}, LnInt<1>{});
    if (G <= 16) return f(LnInt<16>{}, LnInt<1>{});
    if (G <= 32) return f(LnInt<32>{}, LnInt<1>{});
    switch ((G + 63) / 64) {
    case 1: return f(LnInt<64>{}, LnInt<1>{});
    case 2: return f(LnInt<64>{}, LnInt<2>{});
    case 3: return f(LnInt<64>{}, LnInt<3>{});
    case 4: return f(LnInt<64>{}, LnInt<4>{});
    }
    if constexpr (LnGran<T>::VEC == 4) {
        switch ((G + 63) / 64) {
        case 5: return f(LnInt<64>{}, LnInt<5>{});
        case 6: return f(LnInt<64>{}, LnInt<6>{});
        case 7: return f(LnInt<64>{}, LnInt<7>{});
        case 8: return f(LnInt<64>{}, LnInt<8>{});
        }
    }
    return 1;
}

template <typename T>
static int ln_fwd_t(const void* x, void* y, const void* gamma, const void* beta,
                    void* mean, void* invstd, long M, int C, float eps,
                    int rpb, int blocks, hipStream_t s)
{
    return ln_dispatch<T>(C, [&](auto lg, auto ng) {
        hipLaunchKernelGGL((ln_fwd_kernel<T, decltype(lg)::value, decltype(ng)::value>),
                           dim3((unsigned)blocks), dim3(256), 0, s,
                           (const T*)x, (T*)y, (const T*)gamma, (const T*)beta,
                           (float*)mean, (float*)invstd, M, C, rpb, eps);
        return 0;
    });
}

// y = layer_norm(x) over the C channels of each of the M rows. mean, invstd
// (f32 [M]) are written when both are given; null = no backward follows.
// (rows_per_block, blocks) from _ln_plan. Nonzero = rejected, nothing launched.
extern "C" int ps_ln_fwd(const void* x, void* y, const void* gamma,
                         const void* beta, void* mean, void* invstd,
                         long M, long C, float eps, long rows_per_block,
                         long blocks, int dtype, void* stream)
{
    if (!ln_envelope(M, C, dtype) || !x || !y || !gamma || !beta) return 1;
    if ((mean == nullptr) != (invstd == nullptr)) return 1;
    const int elt = dtype == PS_BF16 ? 2 : 4;
    if (!ln_plan_ok(M, C, elt, rows_per_block, blocks)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PS_BF16)
        return ln_fwd_t<unsigned short>(x, y, gamma, beta, mean, invstd, M, (int)C,
                                        eps, (int)rows_per_block, (int)blocks, s);
    return ln_fwd_t<float>(x, y, gamma, beta, mean, invstd, M, (int)C, eps,
                           (int)rows_per_block, (int)blocks, s);
}

template <typename T>
static int ln_bwd_t(const void* x, const void* dy, const void* gamma,
                    const void* mean, const void* invstd, void* dx,
                    void* dgamma, void* dbeta, void* partial, long M, int C,
                    int rpb, int blocks, hipStream_t s)
{
    const int rc = ln_dispatch<T>(C, [&](auto lg, auto ng) {
        hipLaunchKernelGGL((ln_bwd_kernel<T, decltype(lg)::value, decltype(ng)::value>),
                           dim3((unsigned)blocks), dim3(256), 0, s,
                           (const T*)x, (const T*)dy, (const T*)gamma,
                           (const float*)mean, (const float*)invstd, (T*)dx,
                           (float*)partial, M, C, rpb);
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL((ln_param_fold_kernel<T>), dim3((2 * C + 63) / 64),
                       dim3(256), 0, s, (const float*)partial, (T*)dbeta,
                       (T*)dgamma, blocks, C, 2 * C);
    return 0;
}

// mean, invstd: what ps_ln_fwd saved; partial: blocks*2*C floats, always
// written (one block included). The plan need not be the forward's.
extern "C" int ps_ln_bwd(const void* x, const void* dy, const void* gamma,
                         const void* mean, const void* invstd, void* dx,
                         void* dgamma, void* dbeta, void* partial,
                         long M, long C, long rows_per_block, long blocks,
                         int dtype, void* stream)
{
    if (!ln_envelope(M, C, dtype) || !x || !dy || !gamma || !mean || !invstd ||
        !dx || !dgamma || !dbeta || !partial)
        return 1;
    const int elt = dtype == PS_BF16 ? 2 : 4;
    if (!ln_plan_ok(M, C, elt, rows_per_block, blocks)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PS_BF16)
        return ln_bwd_t<unsigned short>(x, dy, gamma, mean, invstd, dx, dgamma,
                                        dbeta, partial, M, (int)C,
                                        (int)rows_per_block, (int)blocks, s);
    return ln_bwd_t<float>(x, dy, gamma, mean, invstd, dx, dgamma, dbeta,
                           partial, M, (int)C, (int)rows_per_block, (int)blocks, s);
}

template <typename T>
static int lscale_fwd_t(const void* y, const void* res, const void* lam,
                        void* out, long M, int C, int rpb, int blocks,
                        hipStream_t s)
{
    return ln_dispatch<T>(C, [&](auto lg, auto ng) {
        hipLaunchKernelGGL((lscale_fwd_kernel<T, decltype(lg)::value, decltype(ng)::value>),
                           dim3((unsigned)blocks), dim3(256), 0, s,
                           (const T*)y, (const T*)res, (const T*)lam, (T*)out,
                           M, C, rpb);
        return 0;
    });
}

// out = res + lambda_c * y over [M][C]
extern "C" int ps_lscale_fwd(const void* y, const void* res, const void* lam,
                             void* out, long M, long C, long rows_per_block,
                             long blocks, int dtype, void* stream)
{
    if (!ln_envelope(M, C, dtype) || !y || !res || !lam || !out) return 1;
    const int elt = dtype == PS_BF16 ? 2 : 4;
    if (!ln_plan_ok(M, C, elt, rows_per_block, blocks)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PS_BF16)
        return lscale_fwd_t<unsigned short>(y, res, lam, out, M, (int)C,
                                            (int)rows_per_block, (int)blocks, s);
    return lscale_fwd_t<float>(y, res, lam, out, M, (int)C,
                               (int)rows_per_block, (int)blocks, s);
}

template <typename T>
static int lscale_bwd_t(const void* y, const void* dout, const void* lam,
                        void* dy, void* dlam, void* partial, long M, int C,
                        int rpb, int blocks, hipStream_t s)
{
    const int rc = ln_dispatch<T>(C, [&](auto lg, auto ng) {
        hipLaunchKernelGGL((lscale_bwd_kernel<T, decltype(lg)::value, decltype(ng)::value>),
                           dim3((unsigned)blocks), dim3(256), 0, s,
                           (const T*)y, (const T*)dout, (const T*)lam, (T*)dy,
                           (float*)partial, M, C, rpb);
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL((ln_param_fold_kernel<T>), dim3((C + 63) / 64), dim3(256),
                       0, s, (const float*)partial, (T*)dlam, (T*)nullptr,
                       blocks, C, C);
    return 0;
}

// dy = lambda_c * dout, dlambda_c = sum_rows dout * y; partial: blocks*C
// floats. The gradient of the residual input is dout itself (no copy here).
extern "C" int ps_lscale_bwd(const void* y, const void* dout, const void* lam,
                             void* dy, void* dlam, void* partial,
                             long M, long C, long rows_per_block, long blocks,
                             int dtype, void* stream)
{
    if (!ln_envelope(M, C, dtype) || !y || !dout || !lam || !dy || !dlam ||
        !partial)
        return 1;
    const int elt = dtype == PS_BF16 ? 2 : 4;
    if (!ln_plan_ok(M, C, elt, rows_per_block, blocks)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PS_BF16)
        return lscale_bwd_t<unsigned short>(y, dout, lam, dy, dlam, partial, M,
                                            (int)C, (int)rows_per_block,
                                            (int)blocks, s);
    return lscale_bwd_t<float>(y, dout, lam, dy, dlam, partial, M, (int)C,
                               (int)rows_per_block, (int)blocks, s);
}

static bool gelu_ok(long n, int dtype) {
    return (dtype == PS_F32 || dtype == PS_BF16) && n >= 8 && n % 8 == 0;
}

// y = 0.5 x (1 + erf(x / sqrt 2)), n % 8 == 0 elements
extern "C" int ps_gelu_fwd(const void* x, void* y, long n, int dtype,
                           void* stream)
{
    if (!gelu_ok(n, dtype) || !x || !y) return 1;
    hipStream_t s = (hipStream_t)stream;
    int blocks;
    if (dtype == PS_BF16) {
        ew_grid(n / 8, 256, &blocks);
        hipLaunchKernelGGL((gelu_fwd_kernel<unsigned short>), dim3(blocks), dim3(256),
                           0, s, (const unsigned short*)x, (unsigned short*)y, n / 8);
    } else {
        ew_grid(n / 4, 256, &blocks);
        hipLaunchKernelGGL((gelu_fwd_kernel<float>), dim3(blocks), dim3(256), 0, s,
                           (const float*)x, (float*)y, n / 4);
    }
    return 0;
}

extern "C" int ps_gelu_bwd(const void* x, const void* dy, void* dx, long n,
                           int dtype, void* stream)
{
    if (!gelu_ok(n, dtype) || !x || !dy || !dx) return 1;
    hipStream_t s = (hipStream_t)stream;
    int blocks;
    if (dtype == PS_BF16) {
        ew_grid(n / 8, 256, &blocks);
        hipLaunchKernelGGL((gelu_bwd_kernel<unsigned short>), dim3(blocks), dim3(256),
                           0, s, (const unsigned short*)x, (const unsigned short*)dy,
                           (unsigned short*)dx, n / 8);
    } else {
        ew_grid(n / 4, 256, &blocks);
        hipLaunchKernelGGL((gelu_bwd_kernel<float>), dim3(blocks), dim3(256), 0, s,
                           (const float*)x, (const float*)dy, (float*)dx, n / 4);
    }
    return 0;
}
