// Fused GroupNorm(+residual)(+ReLU) forward/backward for NHWC activations.
//
// GroupNorm statistics belong to one (sample, group), so a block that owns
// sample n and a slab of SC consecutive channels (whole groups) needs nobody
// else's sums. Where the slab's [HW][SC] tile fits the block's LDS budget the
// activation is read from HBM ONCE: reduced on the way into LDS, normalised
// from the on-chip copy ("resident" form; batchnorm.hip reads x twice in the
// forward and x, dy twice in the backward). Larger tiles take the "streamed"
// form, BN's three-kernel schedule with n-local sums. The host picks the form
// (ops/modules.py:_gn_plan, the only place the rule lives) and hands it in as
// `slab` (channels per block, 0 = streamed); the launch functions take it as
// given and reject a plan that breaks the kernels' invariants.
//
// Layout: x is [N][HW][C], C innermost, bf16 or f32; gamma/beta/dgamma/dbeta
// in the type of x. Envelope: C % 8 == 0, C <= 2048, Cg = C/G in {2..64}.
// mask: bit-packed relu activity in batchnorm.hip's layout, one byte per
// channel octet [N*HW*C/8]. save_mean / save_invstd: f32 [N][G].
//
// Arithmetic (f32 throughout, bf16 is storage only; docs/KERNELS.md):
//   per (n, c)  s1 = sum_p x, s2 = sum_p x^2       fixed order
//   per (n, g)  S1, S2 = the channels' sums added in ascending c, m = HW*Cg
//               mean = S1/m, var = max(S2/m - mean^2, 0), invstd = rsqrtf(var+eps)
//   per (n, c)  scale = gamma*invstd, shift = beta - mean*scale
//               v = x*scale + shift (+ res); mask = v > 0; y = relu?(v), one rounding
//   backward    d = mask ? dy : 0, xc = x - mean
//               s_c = sum_p d, t_c = sum_p d*(xc*invstd)  -> partial[N][2][C]
//               A = sum_c gamma*s_c, B = sum_c gamma*t_c  ascending c
//               dx = a*d + b*xc + k, a = gamma*invstd, b = -invstd^2*B/m,
//               k = -invstd*A/m; dres = d
//               dbeta = sum_n s_c, dgamma = sum_n t_c, n ascending, one rounding
// No atomics; every sum has one fixed order, so two runs are bit-identical.
#include "common.h"

#define GN_LDS_TILE_BUDGET 65536    // the resident tile(s) of one block
#define GN_MAX_CHUNKS 64            // streamed form: row chunks per sample

template <typename T> __device__ __forceinline__ float gn_to_f32(T v);
template <> __device__ __forceinline__ float gn_to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float gn_to_f32<unsigned short>(unsigned short v) { return bf16_to_f32(v); }
template <typename T> __device__ __forceinline__ T gn_from_f32(float v);
template <> __device__ __forceinline__ float gn_from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ unsigned short gn_from_f32<unsigned short>(float v) { return f32_to_bf16(v); }

// one 16-B granule: 8 bf16 or 4 f32 (the granule of conv_dw.hip)
template <typename T> struct Gran;
template <> struct Gran<unsigned short> {
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
};
template <> struct Gran<float> {
    static constexpr int VEC = 4;
    static __device__ __forceinline__ void unpack(uint4 r, float* v) {
        v[0] = __uint_as_float(r.x); v[1] = __uint_as_float(r.y);
        v[2] = __uint_as_float(r.z); v[3] = __uint_as_float(r.w);
    }
    static __device__ __forceinline__ uint4 pack(const float* v) {
        return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]),
                          __float_as_uint(v[2]), __float_as_uint(v[3]));
    }
};

// Fold the row lanes of a [row lane][lane] thread grid (thread t = rl*GL +
// gl) by a fixed tree over red[256][VEC+1]; afterwards the slots of row 0
// hold the totals. Bank argument: thread t touches dword t*(VEC+1) + i, and
// its partner (t + s*GL)*(VEC+1) + i. For one i the 64 lanes of a wave are
// consecutive t, so their addresses step by VEC+1 = 9 (or 5) dwords: odd,
// hence coprime with the 32 (or 64) banks, and every lane of a pass lands on
// its own bank. Without the +1 column the step would be 8 (4) dwords and a
// pass would pile 8-way (4-way) onto 4 (8) banks, the conflict batchnorm.hip
// measured. RL need not be a power of two: the first stage folds the rows
// past the largest power of two below RL.
template <int VEC>
__device__ __forceinline__ void gn_row_fold(float* red, const float* v,
                                            int rl, int GL, int RL)
{
    constexpr int RS = VEC + 1;
    float* mine = red + threadIdx.x * RS;
#pragma unroll
    for (int i = 0; i < VEC; ++i) mine[i] = v[i];
    __syncthreads();
    int s = 1;
    while (s * 2 < RL) s *= 2;
    for (; s > 0; s >>= 1) {
        if (rl < s && rl + s < RL) {
            const float* o = mine + s * GL * RS;
#pragma unroll
            for (int i = 0; i < VEC; ++i) mine[i] += o[i];
        }
        __syncthreads();
    }
}

// channels [cs, cs + Cg) of the slab, ascending, from the folded row 0
template <int VEC>
__device__ __forceinline__ float gn_group_sum(const float* red, int cs, int Cg)
{
    float a = 0.f;
    for (int j = 0; j < Cg; ++j) {
        const int c = cs + j;
        a += red[(c / VEC) * (VEC + 1) + c % VEC];
    }
    return a;
}

// the same with each channel's sum weighted by gamma (backward A, B)
template <int VEC, typename T>
__device__ __forceinline__ float gn_group_wsum(const float* red,
                                               const T* __restrict__ gamma_slab,
                                               int cs, int Cg)
{
    float a = 0.f;
    for (int j = 0; j < Cg; ++j) {
        const int c = cs + j;
        a += gn_to_f32<T>(gamma_slab[c]) * red[(c / VEC) * (VEC + 1) + c % VEC];
    }
    return a;
}

// ---------------- resident forward ----------------
// grid N * C/SC, 256 threads = SC/VEC granule lanes x 256/(SC/VEC) row lanes.
// dynamic LDS: tile[HW][GL] granules, then red[256][VEC+1] floats.
// Walk 1: a thread strides its rows in ascending order with 16-B loads,
// adds each value into its per-channel sum / sum-of-squares registers and
// stores the raw granule to tile[p][gl] (address = t + k*RL*GL granules:
// lane-linear, conflict-free). No LDS read-back for the statistics.
// Group fold: for Cg <= VEC a row-0 lane holds VEC/Cg whole groups in its own
// slot; above that the lane whose granule begins the group adds the slots of
// its Cg/VEC neighbours. Walk 2 reads the tile, writes y and the mask bytes;
// the residual comes straight from global memory (used once).
template <typename T, bool RELU, bool RES>
__global__ __launch_bounds__(256) void gn_fwd_resident_kernel(
    const T* __restrict__ x, T* __restrict__ y, const T* __restrict__ res,
    const T* __restrict__ gamma, const T* __restrict__ beta,
    unsigned char* __restrict__ mask, float* __restrict__ save_mean,
    float* __restrict__ save_invstd, int HW, int C, int Cg, int SC, float eps)
{
    constexpr int VEC = Gran<T>::VEC;
    extern __shared__ uint4 gn_smem[];
    const int GL = SC / VEC, RL = 256 / GL;
    const int gl = threadIdx.x % GL, rl = threadIdx.x / GL;
    const int nslab = C / SC;
    const long n = blockIdx.x / nslab;
    const int slab = blockIdx.x % nslab;
    const int c0 = slab * SC + gl * VEC;
    uint4* tile = gn_smem;
    float* red = (float*)(gn_smem + (size_t)HW * GL);
    const long base = n * HW * (long)C + c0;

    float s1[VEC], s2[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
    if (rl < RL) {
#pragma unroll 4
        for (int p = rl; p < HW; p += RL) {
            const uint4 raw = *(const uint4*)(x + base + (long)p * C);
            tile[p * GL + gl] = raw;
            float v[VEC];
            Gran<T>::unpack(raw, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) { s1[i] += v[i]; s2[i] += v[i] * v[i]; }
        }
    }
    constexpr int NG = VEC / 2;                    // most groups one lane leads
    const int ngl = Cg <= VEC ? VEC / Cg : 1;
    const bool lead = rl == 0 && (Cg <= VEC || (gl * VEC) % Cg == 0);
    float g1[NG], g2[NG];
    gn_row_fold<VEC>(red, s1, rl, GL, RL);
    if (lead) {
#pragma unroll
        for (int k = 0; k < NG; ++k)
            if (k < ngl) g1[k] = gn_group_sum<VEC>(red, gl * VEC + k * Cg, Cg);
    }
    __syncthreads();
    gn_row_fold<VEC>(red, s2, rl, GL, RL);
    if (lead) {
#pragma unroll
        for (int k = 0; k < NG; ++k)
            if (k < ngl) g2[k] = gn_group_sum<VEC>(red, gl * VEC + k * Cg, Cg);
    }
    __syncthreads();
    // red is free now: [group of the slab][mean, invstd]
    if (lead) {
        const float m = (float)((long)HW * Cg);
        const long gbase = n * (C / Cg) + slab * (SC / Cg);
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            if (k < ngl) {
                const int lg = (gl * VEC) / Cg + k;
                const float mean = g1[k] / m;
                const float var = fmaxf(g2[k] / m - mean * mean, 0.f);
                const float invstd = rsqrtf(var + eps);
                red[2 * lg] = mean;
                red[2 * lg + 1] = invstd;
                if (save_mean) {
                    save_mean[gbase + lg] = mean;
                    save_invstd[gbase + lg] = invstd;
                }
            }
        }
    }
    __syncthreads();
    if (rl >= RL) return;
    float sc[VEC], sh[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const int lg = (gl * VEC + i) / Cg;
        const float mean = red[2 * lg], invstd = red[2 * lg + 1];
        sc[i] = gn_to_f32<T>(gamma[c0 + i]) * invstd;
        sh[i] = gn_to_f32<T>(beta[c0 + i]) - mean * sc[i];
    }
    for (int p = rl; p < HW; p += RL) {
        const long o = base + (long)p * C;
        float v[VEC];
        Gran<T>::unpack(tile[p * GL + gl], v);
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = v[i] * sc[i] + sh[i];
        if constexpr (RES) {
            float r[VEC];
            Gran<T>::unpack(*(const uint4*)(res + o), r);
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[i] += r[i];
        }
        if constexpr (RELU) {
            if (mask) {
                unsigned mb = 0;
#pragma unroll
                for (int i = 0; i < VEC; ++i) mb |= (unsigned)(v[i] > 0.f) << i;
                if constexpr (VEC == 8) {
                    mask[o >> 3] = (unsigned char)mb;
                } else {
                    // f32: two neighbouring lanes share an octet's byte; GL
                    // is even, so lane t^1 is the same row's other half
                    const unsigned other = (unsigned)__shfl_xor((int)mb, 1);
                    if (!(gl & 1)) mask[o >> 3] = (unsigned char)(mb | (other << 4));
                }
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[i] = fmaxf(v[i], 0.f);
        }
        *(uint4*)(y + o) = Gran<T>::pack(v);
    }
}

// ---------------- resident backward ----------------
// Same map; two tiles (x raw, d = masked dy) then red. s_c, t_c accumulate on
// the way in, go to partial[n][2][C] from row 0 and fold to A, B in the block.
template <typename T, bool RELU, bool DRES>
__global__ __launch_bounds__(256) void gn_bwd_resident_kernel(
    const T* __restrict__ x, const unsigned char* __restrict__ mask,
    const T* __restrict__ dy, const T* __restrict__ gamma,
    const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
    T* __restrict__ dx, T* __restrict__ dres, float* __restrict__ partial,
    int HW, int C, int Cg, int SC)
{
    constexpr int VEC = Gran<T>::VEC;
    extern __shared__ uint4 gn_smem[];
    const int GL = SC / VEC, RL = 256 / GL;
    const int gl = threadIdx.x % GL, rl = threadIdx.x / GL;
    const int nslab = C / SC;
    const long n = blockIdx.x / nslab;
    const int slab = blockIdx.x % nslab;
    const int c0 = slab * SC + gl * VEC;
    const int G = C / Cg;
    uint4* tx = gn_smem;
    uint4* td = gn_smem + (size_t)HW * GL;
    float* red = (float*)(gn_smem + 2 * (size_t)HW * GL);
    const long base = n * HW * (long)C + c0;

    float mu[VEC], inv[VEC], s[VEC], t[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const int g = (c0 + i) / Cg;
        mu[i] = save_mean[n * G + g];
        inv[i] = save_invstd[n * G + g];
        s[i] = 0.f; t[i] = 0.f;
    }
    if (rl < RL) {
#pragma unroll 2
        for (int p = rl; p < HW; p += RL) {
            const long o = base + (long)p * C;
            const uint4 rawx = *(const uint4*)(x + o);
            uint4 rawd = *(const uint4*)(dy + o);
            float xv[VEC], d[VEC];
            Gran<T>::unpack(rawx, xv);
            Gran<T>::unpack(rawd, d);
            if constexpr (RELU) {
                unsigned mb = mask[o >> 3];
                if constexpr (VEC == 4) mb >>= (gl & 1) * 4;
#pragma unroll
                for (int i = 0; i < VEC; ++i) d[i] = (mb >> i) & 1 ? d[i] : 0.f;
                rawd = Gran<T>::pack(d);     // exact: d is dy or 0
            }
            tx[p * GL + gl] = rawx;
            td[p * GL + gl] = rawd;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                s[i] += d[i];
                t[i] += d[i] * ((xv[i] - mu[i]) * inv[i]);
            }
        }
    }
    constexpr int NG = VEC / 2;
    const int ngl = Cg <= VEC ? VEC / Cg : 1;
    const bool lead = rl == 0 && (Cg <= VEC || (gl * VEC) % Cg == 0);
    const T* gamma_slab = gamma + slab * SC;
    float* prow = partial + n * 2 * (long)C;
    float A[NG], B[NG];
    gn_row_fold<VEC>(red, s, rl, GL, RL);
    if (rl == 0) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) prow[c0 + i] = red[threadIdx.x * (VEC + 1) + i];
    }
    if (lead) {
#pragma unroll
        for (int k = 0; k < NG; ++k)
            if (k < ngl) A[k] = gn_group_wsum<VEC, T>(red, gamma_slab, gl * VEC + k * Cg, Cg);
    }
    __syncthreads();
    gn_row_fold<VEC>(red, t, rl, GL, RL);
    if (rl == 0) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) prow[C + c0 + i] = red[threadIdx.x * (VEC + 1) + i];
    }
    if (lead) {
#pragma unroll
        for (int k = 0; k < NG; ++k)
            if (k < ngl) B[k] = gn_group_wsum<VEC, T>(red, gamma_slab, gl * VEC + k * Cg, Cg);
    }
    __syncthreads();
    // red is free now: [group of the slab][b, k]
    if (lead) {
        const float m = (float)((long)HW * Cg);
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            if (k < ngl) {
                const int lg = (gl * VEC) / Cg + k;
                const float invstd = save_invstd[n * G + slab * (SC / Cg) + lg];
                red[2 * lg] = -(invstd * invstd) * B[k] / m;
                red[2 * lg + 1] = -invstd * A[k] / m;
            }
        }
    }
    __syncthreads();
    if (rl >= RL) return;
    float a[VEC], b[VEC], kk[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const int lg = (gl * VEC + i) / Cg;
        a[i] = gn_to_f32<T>(gamma[c0 + i]) * inv[i];
        b[i] = red[2 * lg];
        kk[i] = red[2 * lg + 1];
    }
#pragma unroll 2
    for (int p = rl; p < HW; p += RL) {
        const long o = base + (long)p * C;
        const uint4 rawd = td[p * GL + gl];
        float xv[VEC], d[VEC];
        Gran<T>::unpack(tx[p * GL + gl], xv);
        Gran<T>::unpack(rawd, d);
        if constexpr (DRES) *(uint4*)(dres + o) = rawd;
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            d[i] = a[i] * d[i] + b[i] * (xv[i] - mu[i]) + kk[i];
        *(uint4*)(dx + o) = Gran<T>::pack(d);
    }
}

// ---------------- dgamma / dbeta ----------------
// partial is [N][2C] (row n: s_c then t_c). A block owns 64 columns and adds
// the rows n = 0, 1, ... in order: 64 rows at a time are fetched by all 256
// threads (coalesced, 16 loads in flight each) into LDS, then thread j < 64
// adds its column top to bottom. Reads of buf[r][j] are lane-linear.
template <typename PT>
__global__ __launch_bounds__(256) void gn_param_fold_kernel(
    const float* __restrict__ partial, PT* __restrict__ dgamma,
    PT* __restrict__ dbeta, int N, int C)
{
    __shared__ float buf[64][64];
    const int col0 = blockIdx.x * 64;
    const int j = threadIdx.x & 63, r4 = threadIdx.x >> 6;
    const int col = col0 + j;
    float acc = 0.f;
    for (int n0 = 0; n0 < N; n0 += 64) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int r = r4 + 4 * k;
            buf[r][j] = (n0 + r < N && col < 2 * C)
                ? partial[(long)(n0 + r) * 2 * C + col] : 0.f;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const int rows = N - n0 < 64 ? N - n0 : 64;
            for (int r = 0; r < rows; ++r) acc += buf[r][j];
        }
        __syncthreads();
    }
    if (threadIdx.x < 64 && col < 2 * C) {
        if (col < C) dbeta[col] = gn_from_f32<PT>(acc);
        else dgamma[col - C] = gn_from_f32<PT>(acc);
    }
}

// ---------------- streamed form ----------------
// BN's schedule with n-local sums. Thread map of batchnorm.hip: channel
// octet cg = t % (C/8), row lane t / (C/8), R = 256/(C/8) rows per pass (lanes
// past R*C/8 idle when C/8 does not divide 256). A block owns ONE contiguous
// chunk of CH rows of one sample (CH a multiple of 8R; at most GN_MAX_CHUNKS
// chunks per sample), never a grid-strided set: loads in flight stay inside
// one DRAM-page window (the reason recorded under bn_stats_kernel).
template <typename T>
__device__ __forceinline__ void gn_load8(const T* p, float* v) {
    if constexpr (sizeof(T) == 2) {
        Gran<T>::unpack(*(const uint4*)p, v);
    } else {
        Gran<T>::unpack(*(const uint4*)p, v);
        Gran<T>::unpack(*(const uint4*)(p + 4), v + 4);
    }
}
template <typename T>
__device__ __forceinline__ void gn_store8(T* p, const float* v) {
    if constexpr (sizeof(T) == 2) {
        *(uint4*)p = Gran<T>::pack(v);
    } else {
        *(uint4*)p = Gran<T>::pack(v);
        *(uint4*)(p + 4) = Gran<T>::pack(v + 4);
    }
}

// chunk partials: pc[(n*chunks + chunk)][2][C]
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(
    const T* __restrict__ x, float* __restrict__ pc, int HW, int C,
    int CH, int chunks)
{
    const int G8 = C >> 3, R = 256 / G8;
    const int cg = threadIdx.x % G8, rib = threadIdx.x / G8;
    const long n = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const int r0 = chunk * CH, r1 = min(r0 + CH, HW);
    __shared__ float red[256 * 9];
    float s1[8], s2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
    if (rib < R) {
        const T* xb = x + n * HW * (long)C + cg * 8;
        for (int sub = r0; sub < r1; sub += 8 * R) {
            if (sub + 8 * R <= r1) {        // guard-free: 8 loads as a batch
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    float v[8];
                    gn_load8<T>(xb + (long)(sub + rib + u * R) * C, v);
#pragma unroll
                    for (int i = 0; i < 8; ++i) { s1[i] += v[i]; s2[i] += v[i] * v[i]; }
                }
            } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int r = sub + rib + u * R;
                    if (r < r1) {
                        float v[8];
                        gn_load8<T>(xb + (long)r * C, v);
#pragma unroll
                        for (int i = 0; i < 8; ++i) { s1[i] += v[i]; s2[i] += v[i] * v[i]; }
                    }
                }
            }
        }
    }
    float* dst = pc + (long)blockIdx.x * 2 * C;
    gn_row_fold<8>(red, s1, rib, G8, R);
    if (rib == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[cg * 8 + i] = red[threadIdx.x * 9 + i];
    }
    __syncthreads();
    gn_row_fold<8>(red, s2, rib, G8, R);
    if (rib == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[C + cg * 8 + i] = red[threadIdx.x * 9 + i];
    }
}

// one block per sample: chunks folded in order per channel, channels folded
// in ascending order per group
__global__ __launch_bounds__(256) void gn_finalize_kernel(
    const float* __restrict__ pc, float* __restrict__ save_mean,
    float* __restrict__ save_invstd, int HW, int C, int Cg, int chunks, float eps)
{
    __shared__ float c1[2048], c2[2048];
    const long n = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        float a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < chunks; ++k) {
            const float* row = pc + (n * chunks + k) * 2 * (long)C;
            a1 += row[c];
            a2 += row[C + c];
        }
        c1[c] = a1; c2[c] = a2;
    }
    __syncthreads();
    const int G = C / Cg;
    const float m = (float)((long)HW * Cg);
    for (int g = threadIdx.x; g < G; g += 256) {
        float a1 = 0.f, a2 = 0.f;
        for (int j = 0; j < Cg; ++j) { a1 += c1[g * Cg + j]; a2 += c2[g * Cg + j]; }
        const float mean = a1 / m;
        const float var = fmaxf(a2 / m - mean * mean, 0.f);
        save_mean[n * G + g] = mean;
        save_invstd[n * G + g] = rsqrtf(var + eps);
    }
}

template <typename T, bool RELU, bool RES>
__global__ __launch_bounds__(256) void gn_norm_kernel(
    const T* __restrict__ x, T* __restrict__ y, const T* __restrict__ res,
    const T* __restrict__ gamma, const T* __restrict__ beta,
    const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
    unsigned char* __restrict__ mask, int HW, int C, int Cg, int CH, int chunks)
{
    const int G8 = C >> 3, R = 256 / G8;
    const int cg = threadIdx.x % G8, rib = threadIdx.x / G8;
    if (rib >= R) return;
    const long n = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const int r0 = chunk * CH, r1 = min(r0 + CH, HW);
    const int G = C / Cg;
    float sc[8], sh[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = cg * 8 + i;
        const float mean = save_mean[n * G + c / Cg];
        sc[i] = gn_to_f32<T>(gamma[c]) * save_invstd[n * G + c / Cg];
        sh[i] = gn_to_f32<T>(beta[c]) - mean * sc[i];
    }
    const long base = n * HW * (long)C + cg * 8;
#pragma unroll 4
    for (int r = r0 + rib; r < r1; r += R) {
        const long o = base + (long)r * C;
        float v[8];
        gn_load8<T>(x + o, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = v[i] * sc[i] + sh[i];
        if constexpr (RES) {
            float rr[8];
            gn_load8<T>(res + o, rr);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += rr[i];
        }
        if constexpr (RELU) {
            if (mask) {
                unsigned mb = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) mb |= (unsigned)(v[i] > 0.f) << i;
                mask[o >> 3] = (unsigned char)mb;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], 0.f);
        }
        gn_store8<T>(y + o, v);
    }
}

template <typename T, bool RELU>
__global__ __launch_bounds__(256) void gn_bwd_reduce_kernel(
    const T* __restrict__ x, const unsigned char* __restrict__ mask,
    const T* __restrict__ dy, const float* __restrict__ save_mean,
    const float* __restrict__ save_invstd, float* __restrict__ pc,
    int HW, int C, int Cg, int CH, int chunks)
{
    const int G8 = C >> 3, R = 256 / G8;
    const int cg = threadIdx.x % G8, rib = threadIdx.x / G8;
    const long n = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const int r0 = chunk * CH, r1 = min(r0 + CH, HW);
    const int G = C / Cg;
    __shared__ float red[256 * 9];
    float s[8], t[8], mu[8], inv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s[i] = 0.f; t[i] = 0.f;
        const int g = rib < R ? (cg * 8 + i) / Cg : 0;
        mu[i] = save_mean[n * G + g];
        inv[i] = save_invstd[n * G + g];
    }
    if (rib < R) {
        const long base = n * HW * (long)C + cg * 8;
        for (int sub = r0; sub < r1; sub += 8 * R) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = sub + rib + u * R;
                if (r < r1) {
                    const long o = base + (long)r * C;
                    float xv[8], d[8];
                    gn_load8<T>(dy + o, d);
                    gn_load8<T>(x + o, xv);
                    if constexpr (RELU) {
                        const unsigned mb = mask[o >> 3];
#pragma unroll
                        for (int i = 0; i < 8; ++i) d[i] = (mb >> i) & 1 ? d[i] : 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        s[i] += d[i];
                        t[i] += d[i] * ((xv[i] - mu[i]) * inv[i]);
                    }
                }
            }
        }
    }
    float* dst = pc + (long)blockIdx.x * 2 * C;
    gn_row_fold<8>(red, s, rib, G8, R);
    if (rib == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[cg * 8 + i] = red[threadIdx.x * 9 + i];
    }
    __syncthreads();
    gn_row_fold<8>(red, t, rib, G8, R);
    if (rib == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[C + cg * 8 + i] = red[threadIdx.x * 9 + i];
    }
}

// chunks -> partial[n][2][C]; groups -> coef[n][G][2] = (b, k)
template <typename PT>
__global__ __launch_bounds__(256) void gn_bwd_finalize_kernel(
    const float* __restrict__ pc, const PT* __restrict__ gamma,
    const float* __restrict__ save_invstd, float* __restrict__ partial,
    float* __restrict__ coef, int HW, int C, int Cg, int chunks)
{
    __shared__ float c1[2048], c2[2048];
    const long n = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        float a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < chunks; ++k) {
            const float* row = pc + (n * chunks + k) * 2 * (long)C;
            a1 += row[c];
            a2 += row[C + c];
        }
        partial[n * 2 * C + c] = a1;
        partial[n * 2 * C + C + c] = a2;
        c1[c] = a1; c2[c] = a2;
    }
    __syncthreads();
    const int G = C / Cg;
    const float m = (float)((long)HW * Cg);
    for (int g = threadIdx.x; g < G; g += 256) {
        float A = 0.f, B = 0.f;
        for (int j = 0; j < Cg; ++j) {
            const float gm = gn_to_f32<PT>(gamma[g * Cg + j]);
            A += gm * c1[g * Cg + j];
            B += gm * c2[g * Cg + j];
        }
        const float invstd = save_invstd[n * G + g];
        coef[(n * G + g) * 2] = -(invstd * invstd) * B / m;
        coef[(n * G + g) * 2 + 1] = -invstd * A / m;
    }
}

template <typename T, bool RELU, bool DRES>
__global__ __launch_bounds__(256) void gn_bwd_dx_kernel(
    const T* __restrict__ x, const unsigned char* __restrict__ mask,
    const T* __restrict__ dy, const T* __restrict__ gamma,
    const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
    const float* __restrict__ coef, T* __restrict__ dx, T* __restrict__ dres,
    int HW, int C, int Cg, int CH, int chunks)
{
    const int G8 = C >> 3, R = 256 / G8;
    const int cg = threadIdx.x % G8, rib = threadIdx.x / G8;
    if (rib >= R) return;
    const long n = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const int r0 = chunk * CH, r1 = min(r0 + CH, HW);
    const int G = C / Cg;
    float mu[8], a[8], b[8], kk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = cg * 8 + i;
        const long ng = n * G + c / Cg;
        mu[i] = save_mean[ng];
        a[i] = gn_to_f32<T>(gamma[c]) * save_invstd[ng];
        b[i] = coef[ng * 2];
        kk[i] = coef[ng * 2 + 1];
    }
    const long base = n * HW * (long)C + cg * 8;
#pragma unroll 4
    for (int r = r0 + rib; r < r1; r += R) {
        const long o = base + (long)r * C;
        float xv[8], d[8];
        gn_load8<T>(dy + o, d);
        gn_load8<T>(x + o, xv);
        if constexpr (RELU) {
            const unsigned mb = mask[o >> 3];
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = (mb >> i) & 1 ? d[i] : 0.f;
        }
        if constexpr (DRES) gn_store8<T>(dres + o, d);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            d[i] = a[i] * d[i] + b[i] * (xv[i] - mu[i]) + kk[i];
        gn_store8<T>(dx + o, d);
    }
}

// ---------------- C API ----------------
static bool gn_envelope(long N, long HW, long C, long G, int dtype) {
    if (dtype != PS_F32 && dtype != PS_BF16) return false;
    // N * (slabs or chunks) is the grid: 2^22 * 256 blocks at the most
    if (N < 1 || HW < 1 || HW > (1L << 30) || N > (1L << 22)) return false;
    if (C < 8 || C % 8 || C > 2048 || G < 1 || C % G) return false;
    const long Cg = C / G;
    return Cg == 2 || Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32 || Cg == 64;
}

// the invariants the resident kernels rely on (not the choice among plans)
static bool gn_slab_ok(long HW, long C, long Cg, long SC, int elt, int tiles) {
    const int vec = 16 / elt;
    return SC >= 8 && SC % Cg == 0 && SC % 8 == 0 && C % SC == 0 &&
           SC / vec <= 256 && (long)tiles * HW * SC * elt <= GN_LDS_TILE_BUDGET;
}

// rows per block of the streamed kernels
static int gn_chunk_rows(long HW, long C) {
    const long unit = 8 * (256 / (C >> 3));
    long ch = unit;
    if ((HW + ch - 1) / ch > GN_MAX_CHUNKS) {
        const long want = (HW + GN_MAX_CHUNKS - 1) / GN_MAX_CHUNKS;
        ch = (want + unit - 1) / unit * unit;
    }
    return (int)ch;
}

// f32 words of `ws` the streamed form needs (forward and backward alike):
// chunk partials [N][chunks][2][C] + coefficients [N][G][2]
extern "C" long ps_gn_ws_floats(long N, long HW, long C, long G) {
    const long ch = gn_chunk_rows(HW, C);
    const long chunks = (HW + ch - 1) / ch;
    return N * chunks * 2 * C + N * G * 2;
}

template <typename K>
static int gn_allow_lds(K kernel, size_t bytes) {
    // tiles above 48 KiB of dynamic LDS are opted into per kernel
    return hipFuncSetAttribute((const void*)kernel,
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes) == hipSuccess ? 0 : 1;
}

#define GN_RESIDENT_LDS(T, tiles, HW, SC) \
    ((size_t)(tiles) * (HW) * (SC) * sizeof(T) + 256 * (Gran<T>::VEC + 1) * sizeof(float))

template <typename T, bool RELU, bool RES>
static int gn_fwd_resident_launch(const void* x, void* y, const void* res,
                                  const void* gamma, const void* beta,
                                  void* mask, void* mean, void* invstd,
                                  long N, int HW, int C, int Cg, int SC,
                                  float eps, hipStream_t s)
{
    auto k = gn_fwd_resident_kernel<T, RELU, RES>;
    static int allowed = gn_allow_lds(k, GN_LDS_TILE_BUDGET + 256 * 9 * sizeof(float));
    if (allowed) return 2;
    hipLaunchKernelGGL(k, dim3((unsigned)(N * (C / SC))), dim3(256),
                       GN_RESIDENT_LDS(T, 1, HW, SC), s,
                       (const T*)x, (T*)y, (const T*)res, (const T*)gamma,
                       (const T*)beta, (unsigned char*)mask, (float*)mean,
                       (float*)invstd, HW, C, Cg, SC, eps);
    return 0;
}

template <typename T, bool RELU, bool RES>
static int gn_fwd_streamed_launch(const void* x, void* y, const void* res,
                                  const void* gamma, const void* beta,
                                  void* mask, void* mean, void* invstd, void* ws,
                                  long N, int HW, int C, int Cg, float eps,
                                  hipStream_t s)
{
    const int CH = gn_chunk_rows(HW, C), chunks = (HW + CH - 1) / CH;
    const dim3 grid((unsigned)(N * chunks)), b256(256);
    hipLaunchKernelGGL((gn_stats_kernel<T>), grid, b256, 0, s,
                       (const T*)x, (float*)ws, HW, C, CH, chunks);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((unsigned)N), b256, 0, s,
                       (const float*)ws, (float*)mean, (float*)invstd,
                       HW, C, Cg, chunks, eps);
    hipLaunchKernelGGL((gn_norm_kernel<T, RELU, RES>), grid, b256, 0, s,
                       (const T*)x, (T*)y, (const T*)res, (const T*)gamma,
                       (const T*)beta, (const float*)mean, (const float*)invstd,
                       (unsigned char*)mask, HW, C, Cg, CH, chunks);
    return 0;
}

template <typename T>
static int gn_fwd_t(const void* x, void* y, const void* gamma, const void* beta,
                    const void* res, void* mask, void* mean, void* invstd,
                    void* ws, long N, int HW, int C, int Cg, float eps, int relu,
                    int slab, hipStream_t s)
{
#define GN_FWD(RELU, RES) \
    (slab ? gn_fwd_resident_launch<T, RELU, RES>(x, y, res, gamma, beta, mask, \
                mean, invstd, N, HW, C, Cg, slab, eps, s) \
          : gn_fwd_streamed_launch<T, RELU, RES>(x, y, res, gamma, beta, mask, \
                mean, invstd, ws, N, HW, C, Cg, eps, s))
    if (relu) return res ? GN_FWD(true, true) : GN_FWD(true, false);
    return res ? GN_FWD(false, true) : GN_FWD(false, false);
#undef GN_FWD
}

// y = relu?(gn(x) + res?). mask (relu), mean, invstd may be null in the
// resident form when no backward follows; the streamed form needs mean,
// invstd and ws (ps_gn_ws_floats). slab: channels per block from _gn_plan
// with tiles = 1, 0 = streamed. Nonzero = rejected, nothing launched.
extern "C" int ps_gn_fwd(const void* x, void* y, const void* gamma,
                         const void* beta, const void* res, void* mask,
                         void* mean, void* invstd, void* ws,
                         long N, long HW, long C, long G, float eps, int relu,
                         int slab, int dtype, void* stream)
{
    if (!gn_envelope(N, HW, C, G, dtype) || !x || !y || !gamma || !beta) return 1;
    const int elt = dtype == PS_BF16 ? 2 : 4;
    const long Cg = C / G;
    if (slab) {
        if (!gn_slab_ok(HW, C, Cg, slab, elt, 1)) return 1;
        if ((mean == nullptr) != (invstd == nullptr)) return 1;
    } else if (!mean || !invstd || !ws) {
        return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PS_BF16)
        return gn_fwd_t<unsigned short>(x, y, gamma, beta, res, mask, mean, invstd,
                                        ws, N, (int)HW, (int)C, (int)Cg, eps, relu, slab, s);
    return gn_fwd_t<float>(x, y, gamma, beta, res, mask, mean, invstd, ws,
                           N, (int)HW, (int)C, (int)Cg, eps, relu, slab, s);
}

template <typename T, bool RELU, bool DRES>
static int gn_bwd_launch(const void* x, const void* mask, const void* dy,
                         const void* gamma, const void* mean, const void* invstd,
                         void* dx, void* dres, void* partial, void* ws,
                         long N, int HW, int C, int Cg, int slab, hipStream_t s)
{
    const dim3 b256(256);
    if (slab) {
        auto k = gn_bwd_resident_kernel<T, RELU, DRES>;
        static int allowed = gn_allow_lds(k, GN_LDS_TILE_BUDGET + 256 * 9 * sizeof(float));
        if (allowed) return 2;
        hipLaunchKernelGGL(k, dim3((unsigned)(N * (C / slab))), b256,
                           GN_RESIDENT_LDS(T, 2, HW, slab), s,
                           (const T*)x, (const unsigned char*)mask, (const T*)dy,
                           (const T*)gamma, (const float*)mean, (const float*)invstd,
                           (T*)dx, (T*)dres, (float*)partial, HW, C, Cg, slab);
        return 0;
    }
    const int CH = gn_chunk_rows(HW, C), chunks = (HW + CH - 1) / CH;
    const dim3 grid((unsigned)(N * chunks));
    float* coef = (float*)ws + N * chunks * 2 * (long)C;
    hipLaunchKernelGGL((gn_bwd_reduce_kernel<T, RELU>), grid, b256, 0, s,
                       (const T*)x, (const unsigned char*)mask, (const T*)dy,
                       (const float*)mean, (const float*)invstd, (float*)ws,
                       HW, C, Cg, CH, chunks);
    hipLaunchKernelGGL((gn_bwd_finalize_kernel<T>), dim3((unsigned)N), b256, 0, s,
                       (const float*)ws, (const T*)gamma, (const float*)invstd,
                       (float*)partial, coef, HW, C, Cg, chunks);
    hipLaunchKernelGGL((gn_bwd_dx_kernel<T, RELU, DRES>), grid, b256, 0, s,
                       (const T*)x, (const unsigned char*)mask, (const T*)dy,
                       (const T*)gamma, (const float*)mean, (const float*)invstd,
                       (const float*)coef, (T*)dx, (T*)dres, HW, C, Cg, CH, chunks);
    return 0;
}

template <typename T>
static int gn_bwd_t(const void* x, const void* mask, const void* dy,
                    const void* gamma, const void* mean, const void* invstd,
                    void* dx, void* dgamma, void* dbeta, void* dres,
                    void* partial, void* ws, long N, int HW, int C, int Cg,
                    int relu, int slab, hipStream_t s)
{
#define GN_BWD(RELU, DRES) \
    gn_bwd_launch<T, RELU, DRES>(x, mask, dy, gamma, mean, invstd, dx, dres, \
                                 partial, ws, N, HW, C, Cg, slab, s)
    int rc;
    if (relu) rc = dres ? GN_BWD(true, true) : GN_BWD(true, false);
    else      rc = dres ? GN_BWD(false, true) : GN_BWD(false, false);
#undef GN_BWD
    if (rc) return rc;
    hipLaunchKernelGGL((gn_param_fold_kernel<T>), dim3((2 * C + 63) / 64),
                       dim3(256), 0, s, (const float*)partial, (T*)dgamma,
                       (T*)dbeta, (int)N, C);
    return 0;
}

// mask: the bytes ps_gn_fwd wrote (relu); mean, invstd: its saved f32
// statistics; partial: N*2*C floats; ws: ps_gn_ws_floats, streamed form only.
// slab: _gn_plan with tiles = 2 (x and dy), 0 = streamed.
extern "C" int ps_gn_bwd(const void* x, const void* mask, const void* dy,
                         const void* gamma, const void* mean, const void* invstd,
                         void* dx, void* dgamma, void* dbeta, void* dres,
                         void* partial, void* ws,
                         long N, long HW, long C, long G, int relu, int slab,
                         int dtype, void* stream)
{
    if (!gn_envelope(N, HW, C, G, dtype) || !x || !dy || !gamma || !mean ||
        !invstd || !dx || !dgamma || !dbeta || !partial || (relu && !mask))
        return 1;
    const int elt = dtype == PS_BF16 ? 2 : 4;
    const long Cg = C / G;
    if (slab ? !gn_slab_ok(HW, C, Cg, slab, elt, 2) : !ws) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PS_BF16)
        return gn_bwd_t<unsigned short>(x, mask, dy, gamma, mean, invstd, dx, dgamma,
                                        dbeta, dres, partial, ws, N, (int)HW, (int)C,
                                        (int)Cg, relu, slab, s);
    return gn_bwd_t<float>(x, mask, dy, gamma, mean, invstd, dx, dgamma, dbeta,
                           dres, partial, ws, N, (int)HW, (int)C, (int)Cg, relu, slab, s);
}
