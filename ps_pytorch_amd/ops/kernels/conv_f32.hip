// NHWC implicit-GEMM convolution, f32 in / f32 accumulate / f32 out, on the
// exact-f32 MFMA of gfx950 (v_mfma_f32_16x16x4_f32). This is the
// --compute-dtype fp32 twin of conv.hip: the reference trains in fp32
// (ref: src/model_ops/*.py through nn.Conv2d / nn.Linear), and this family
// keeps that path on in-tree kernels instead of MIOpen / Tensile.
//
// Numerics: every output element is a k-ordered f32 fma chain (one rounding
// per product, no wider internal accumulation), so on inputs whose products
// and partial sums are representable the result is exact, and otherwise it
// obeys the standard gamma(n) summation bound for any order.
//
// One kernel template serves the three GEMMs; MODE selects how the two
// operands are gathered (D[row, col] = sum_kk A[row, kk] * B[kk, col]):
//
//   FWD    rows = Nb*P*Q   cols = K      kk = (r, s, c)
//          A = x[n, p*st-pd+r, q*st-pd+s, c]        B = w[col, kk]
//   DGRAD  rows = Nb*H*W   cols = C      kk = (r, s, k)
//          A = dout[n, (h+pd-r)/st, (w+pd-s)/st, k] B = w[k, r, s, col]
//          (w gathered in place; every dx pixel is a row, so pixels no tap
//          reaches come out as 0, or as dcarry alone)
//   WGRAD  rows = K        cols = R*S*C  kk = output pixel m, split over
//          blockIdx.z into f32 slabs that a second kernel folds in slab
//          order (no atomics: two runs are bit-identical)
//          A = dout[m, row]                         B = x[n, p*st-pd+r, ...]
//
// Tiling: 256 threads = 4 waves, block tile 64 x 64 x 16, each wave a 32x32
// quadrant as 2x2 independent 16x16 accumulators (the 16x16x4 form has a
// 40-cycle dependent latency against a 32-cycle issue interval, so a chain
// needs >= 2 accumulators). Operands are staged through LDS k-major
// (As[k][row], Bs[k][col]) so a fragment read is 16 consecutive floats per
// k; the 80-float row stride puts the four k rows of one MFMA on disjoint
// banks. Lane maps: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15],
// D[row = 4 * (l >> 4) + reg][col = l & 15]. Single LDS buffer; the next
// step's global loads are prefetched into registers under the MFMAs.
//
// Loads: 16-byte global loads only where the address is provably aligned
// (contiguous extent % 4 == 0 and a 16-byte-aligned base, decided on the
// host); otherwise guarded 4-byte loads. All tile tails are predicated and
// every element offset is 64-bit. No padding of C or K anywhere.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { F32_FWD = 0, F32_DGRAD = 1, F32_WGRAD = 2 };

constexpr int TM = 64;       // block tile rows
constexpr int TN = 64;       // block tile cols
constexpr int TKK = 16;      // contraction per k-step
constexpr int LDS_LD = 80;   // LDS row stride (floats)

struct ConvF32 {
    const float* a;
    const float* b;
    float* out;
    const float* extra;   // fwd: bias[K]; dgrad: dcarry[Nb,H,W,C]; or null
    int Nb, H, W, C, K, P, Q, R, S, st, pd;
    long M;               // GEMM rows
    int N;                // GEMM cols
    long KK;              // contraction length
    long kchunk;          // wgrad: contraction per slab (multiple of TKK)
    int veca, vecb;       // 16-byte loads allowed for A / B
};

// fwd:   (ay, ax) = (p*st - pd, q*st - pd), kk = (r*S + s)*C + c -> x offset
// dgrad: (ay, ax) = (h + pd, w + pd),       kk = (r*S + s)*K + k -> dout offset
template <int MODE>
__device__ __forceinline__ long a_gather(const ConvF32& p, int an, int ay,
                                         int ax, long kk, bool& ok)
{
    const int ch = (MODE == F32_FWD) ? p.C : p.K;
    const int rs = (int)(kk / ch);
    const int c = (int)(kk - (long)rs * ch);
    const int r = rs / p.S;
    const int s = rs - r * p.S;
    if (MODE == F32_FWD) {
        const int h = ay + r, w = ax + s;
        ok = (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
        return (((long)an * p.H + h) * p.W + w) * p.C + c;
    } else {
        int hp = ay - r, wp = ax - s;
        ok = hp >= 0 && wp >= 0;
        if (p.st == 2) {
            ok = ok && !(hp & 1) && !(wp & 1);
            hp >>= 1;
            wp >>= 1;
        }
        ok = ok && hp < p.P && wp < p.Q;
        return (((long)an * p.P + hp) * p.Q + wp) * p.K + c;
    }
}

__device__ __forceinline__ void ld4(const float* src, float v[4])
{
    f32x4 t = *(const f32x4*)src;
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}

template <int MODE>
__global__ __launch_bounds__(256) void conv_f32_kernel(ConvF32 p)
{
    __shared__ __attribute__((aligned(16))) float As[TKK][LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[TKK][LDS_LD];

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;
    const long m0 = (long)blockIdx.x * TM;
    const int n0 = blockIdx.y * TN;
    long kbeg = 0, kend = p.KK;
    if (MODE == F32_WGRAD) {
        kbeg = (long)blockIdx.z * p.kchunk;
        kend = kbeg + p.kchunk < p.KK ? kbeg + p.kchunk : p.KK;
    }

    // staging roles: an operand contiguous along the contraction is loaded
    // as (outer o_loc, 4 consecutive kk from kq); one contiguous along its
    // outer dim as (kk k_loc, 4 consecutive outer from oq)
    const int o_loc = t >> 2, kq = (t & 3) * 4;
    const int k_loc = t >> 4, oq = (t & 15) * 4;

    // fwd / dgrad: this thread's A row, decoded once
    int an = 0, ay = 0, ax = 0;
    bool av = false;
    if (MODE != F32_WGRAD) {
        const long m = m0 + o_loc;
        av = m < p.M;
        if (av) {
            const int plane = (MODE == F32_FWD) ? p.P * p.Q : p.H * p.W;
            const int width = (MODE == F32_FWD) ? p.Q : p.W;
            an = (int)(m / plane);
            const int rem = (int)(m - (long)an * plane);
            const int yy = rem / width, xx = rem - yy * width;
            if (MODE == F32_FWD) { ay = yy * p.st - p.pd; ax = xx * p.st - p.pd; }
            else { ay = yy + p.pd; ax = xx + p.pd; }
        }
    }
    // wgrad: this thread's 4 B columns (r, s, c), decoded once
    int cr[4] = {0, 0, 0, 0}, cs[4] = {0, 0, 0, 0}, cc[4] = {0, 0, 0, 0};
    bool cv[4] = {false, false, false, false};
    if (MODE == F32_WGRAD) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = n0 + oq + u;
            cv[u] = col < p.N;
            const int rs = col / p.C;
            cc[u] = col - rs * p.C;
            cr[u] = rs / p.S;
            cs[u] = rs - cr[u] * p.S;
        }
    }

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // register prefetch: the global loads of step k+1 are issued before the
    // MFMAs of step k and land while they run
    float a4[4], b4[4];
    auto load_tile = [&](const long k0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { a4[u] = 0.f; b4[u] = 0.f; }

        // ---- A ----
        if (MODE != F32_WGRAD) {
            const long kk = k0 + kq;
            if (p.veca) {
                // extent % 4 == 0 and kk % 4 == 0: the 4 elements share one
                // tap and one validity, and the address is 16-B aligned
                bool ok = false;
                long off = 0;
                if (av && kk < kend) off = a_gather<MODE>(p, an, ay, ax, kk, ok);
                if (ok) ld4(p.a + off, a4);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    bool ok = false;
                    long off = 0;
                    if (av && kk + u < kend)
                        off = a_gather<MODE>(p, an, ay, ax, kk + u, ok);
                    if (ok) a4[u] = p.a[off];
                }
            }
        } else {
            const long kk = k0 + k_loc;       // output pixel m
            const long row = m0 + oq;         // k
            if (kk < kend) {
                const float* src = p.a + kk * p.K + row;
                if (p.veca) {
                    if (row < p.M) ld4(src, a4);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (row + u < p.M) a4[u] = src[u];
                }
            }
        }

        // ---- B ----
        if (MODE == F32_FWD) {
            const int col = n0 + o_loc;
            const long kk = k0 + kq;
            if (col < p.N) {
                const float* src = p.b + (long)col * p.KK + kk;
                if (p.vecb) {
                    if (kk < kend) ld4(src, b4);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (kk + u < kend) b4[u] = src[u];
                }
            }
        } else if (MODE == F32_DGRAD) {
            const long kk = k0 + k_loc;
            const int col = n0 + oq;          // c
            if (kk < kend) {
                const int rs = (int)(kk / p.K);
                const int k = (int)(kk - (long)rs * p.K);
                const float* src =
                    p.b + ((long)k * (p.R * p.S) + rs) * p.C + col;
                if (p.vecb) {
                    if (col < p.N) ld4(src, b4);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (col + u < p.N) b4[u] = src[u];
                }
            }
        } else {
            const long kk = k0 + k_loc;       // output pixel m
            if (kk < kend) {
                const int plane = p.P * p.Q;
                const int n = (int)(kk / plane);
                const int rem = (int)(kk - (long)n * plane);
                const int pp = rem / p.Q, qq = rem - pp * p.Q;
                const int h0 = pp * p.st - p.pd, w0 = qq * p.st - p.pd;
                if (p.vecb) {
                    const int h = h0 + cr[0], w = w0 + cs[0];
                    if (cv[0] && (unsigned)h < (unsigned)p.H &&
                        (unsigned)w < (unsigned)p.W)
                        ld4(p.b + (((long)n * p.H + h) * p.W + w) * p.C + cc[0],
                            b4);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int h = h0 + cr[u], w = w0 + cs[u];
                        if (cv[u] && (unsigned)h < (unsigned)p.H &&
                            (unsigned)w < (unsigned)p.W)
                            b4[u] = p.b[(((long)n * p.H + h) * p.W + w) * p.C +
                                        cc[u]];
                    }
                }
            }
        }

    };

    if (kbeg < kend) load_tile(kbeg);
    for (long k0 = kbeg; k0 < kend; k0 += TKK) {
        __syncthreads();   // previous step's fragment reads are done
        if (MODE != F32_WGRAD) {
#pragma unroll
            for (int u = 0; u < 4; ++u) As[kq + u][o_loc] = a4[u];
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) As[k_loc][oq + u] = a4[u];
        }
        if (MODE == F32_FWD) {
#pragma unroll
            for (int u = 0; u < 4; ++u) Bs[kq + u][o_loc] = b4[u];
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) Bs[k_loc][oq + u] = b4[u];
        }
        __syncthreads();
        if (k0 + TKK < kend) load_tile(k0 + TKK);

#pragma unroll
        for (int ks = 0; ks < TKK; ks += 4) {
            const int kr = ks + (lane >> 4);
            const float a0 = As[kr][wm + (lane & 15)];
            const float a1 = As[kr][wm + 16 + (lane & 15)];
            const float b0 = Bs[kr][wn + (lane & 15)];
            const float b1 = Bs[kr][wn + 16 + (lane & 15)];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }

    // ---- epilogue: D[row = 4*(l>>4) + reg][col = l & 15] ----
    float* out = p.out;
    if (MODE == F32_WGRAD) out += (long)blockIdx.z * p.M * p.N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
                if (row < p.M && col < p.N) {
                    const long o = row * p.N + col;
                    float v = acc[i][j][r];
                    if (MODE == F32_FWD && p.extra) v += p.extra[col];
                    if (MODE == F32_DGRAD && p.extra) v += p.extra[o];
                    out[o] = v;
                }
            }
        }
}

// dw[i] = sum over slabs in slab order (fixed order => bitwise repeatable)
__global__ __launch_bounds__(256) void wgrad_f32_fold_kernel(
    float* __restrict__ dw, const float* __restrict__ partial, long n,
    int split)
{
    EW_IDX
    for (long i = gid; i < n; i += stride) {
        float acc = partial[i];
        for (int z = 1; z < split; ++z) acc += partial[(long)z * n + i];
        dw[i] = acc;
    }
}

// deterministic column sum, stage 1: part blockIdx.y sums its row range.
// The block is (256 / kt) row lanes x kt columns (kt a power of two sized
// to K, so narrow LeNet / classifier rows still fill the block); each lane
// strides the rows, then lane 0 folds the row lanes in lane order.
__global__ __launch_bounds__(256) void colsum_f32_part_kernel(
    float* __restrict__ partial, const float* __restrict__ dout, long M,
    int K, long chunk, int ktshift)
{
    __shared__ float red[256];
    const int kt = 1 << ktshift, rlanes = 256 >> ktshift;
    const int kx = threadIdx.x & (kt - 1), rl = threadIdx.x >> ktshift;
    const int k = blockIdx.x * kt + kx;
    const long beg = (long)blockIdx.y * chunk;
    const long end = beg + chunk < M ? beg + chunk : M;
    float acc = 0.f;
    if (k < K)
        for (long m = beg + rl; m < end; m += rlanes) acc += dout[m * K + k];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (rl == 0 && k < K) {
        float s = 0.f;
        for (int j = 0; j < rlanes; ++j) s += red[j * kt + kx];
        partial[(long)blockIdx.y * K + k] = s;
    }
}

__global__ __launch_bounds__(256) void colsum_f32_fold_kernel(
    float* __restrict__ db, const float* __restrict__ partial, int K,
    int parts)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    float acc = 0.f;
    for (int q = 0; q < parts; ++q) acc += partial[(long)q * K + k];
    db[k] = acc;
}

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

extern "C" void ps_conv_fwd_f32(
    const void* x, const void* w, const void* bias, void* out,
    int Nb, int H, int W, int C, int K, int P, int Q, int R, int S,
    int stride, int pad, void* strm)
{
    ConvF32 p;
    p.a = (const float*)x; p.b = (const float*)w; p.out = (float*)out;
    p.extra = (const float*)bias;
    p.Nb = Nb; p.H = H; p.W = W; p.C = C; p.K = K; p.P = P; p.Q = Q;
    p.R = R; p.S = S; p.st = stride; p.pd = pad;
    p.M = (long)Nb * P * Q; p.N = K; p.KK = (long)R * S * C; p.kchunk = 0;
    p.veca = (C % 4 == 0) && al16(x);
    p.vecb = (p.KK % 4 == 0) && al16(w);
    if (p.M <= 0 || p.N <= 0) return;
    dim3 grid((unsigned)((p.M + TM - 1) / TM), (unsigned)((p.N + TN - 1) / TN));
    hipLaunchKernelGGL(conv_f32_kernel<F32_FWD>, grid, dim3(256), 0,
                       (hipStream_t)strm, p);
}

extern "C" void ps_conv_dgrad_f32(
    const void* dout, const void* w, void* dx, const void* dcarry,
    int Nb, int H, int W, int C, int K, int P, int Q, int R, int S,
    int stride, int pad, void* strm)
{
    ConvF32 p;
    p.a = (const float*)dout; p.b = (const float*)w; p.out = (float*)dx;
    p.extra = (const float*)dcarry;
    p.Nb = Nb; p.H = H; p.W = W; p.C = C; p.K = K; p.P = P; p.Q = Q;
    p.R = R; p.S = S; p.st = stride; p.pd = pad;
    p.M = (long)Nb * H * W; p.N = C; p.KK = (long)R * S * K; p.kchunk = 0;
    p.veca = (K % 4 == 0) && al16(dout);
    p.vecb = (C % 4 == 0) && al16(w);
    if (p.M <= 0 || p.N <= 0) return;
    dim3 grid((unsigned)((p.M + TM - 1) / TM), (unsigned)((p.N + TN - 1) / TN));
    hipLaunchKernelGGL(conv_f32_kernel<F32_DGRAD>, grid, dim3(256), 0,
                       (hipStream_t)strm, p);
}

// partial: split * K * R*S*C floats (unused when split == 1)
extern "C" void ps_conv_wgrad_f32(
    const void* dout, const void* x, void* partial, void* dw,
    int Nb, int H, int W, int C, int K, int P, int Q, int R, int S,
    int stride, int pad, int split, void* strm)
{
    ConvF32 p;
    if (split < 1) split = 1;
    p.a = (const float*)dout; p.b = (const float*)x;
    p.out = (float*)(split == 1 ? dw : partial);
    p.extra = nullptr;
    p.Nb = Nb; p.H = H; p.W = W; p.C = C; p.K = K; p.P = P; p.Q = Q;
    p.R = R; p.S = S; p.st = stride; p.pd = pad;
    p.M = K; p.N = R * S * C; p.KK = (long)Nb * P * Q;
    const long per = (p.KK + split - 1) / split;
    p.kchunk = (per + TKK - 1) / TKK * TKK;
    if (p.kchunk < TKK) p.kchunk = TKK;
    p.veca = (K % 4 == 0) && al16(dout);
    p.vecb = (C % 4 == 0) && al16(x);
    if (p.M <= 0 || p.N <= 0) return;
    dim3 grid((unsigned)((p.M + TM - 1) / TM), (unsigned)((p.N + TN - 1) / TN),
              (unsigned)split);
    hipLaunchKernelGGL(conv_f32_kernel<F32_WGRAD>, grid, dim3(256), 0,
                       (hipStream_t)strm, p);
    if (split > 1) {
        const long n = p.M * p.N;
        int blocks; ew_grid(n, 256, &blocks);
        hipLaunchKernelGGL(wgrad_f32_fold_kernel, dim3(blocks), dim3(256), 0,
                           (hipStream_t)strm, (float*)dw,
                           (const float*)partial, n, split);
    }
}

// partial: 256 * K floats
extern "C" void ps_conv_bias_grad_f32(
    void* db, const void* dout, void* partial, long M, int K, void* strm)
{
    if (K <= 0) return;
    long parts = (M + 63) / 64;
    if (parts < 1) parts = 1;
    if (parts > 256) parts = 256;
    const long chunk = (M + parts - 1) / parts;
    int ktshift = 3;
    while (ktshift < 8 && (1 << ktshift) < K) ++ktshift;
    const int kt = 1 << ktshift;
    const unsigned kb = (unsigned)((K + 255) / 256);
    hipLaunchKernelGGL(colsum_f32_part_kernel,
                       dim3((unsigned)((K + kt - 1) / kt), (unsigned)parts),
                       dim3(256), 0, (hipStream_t)strm, (float*)partial,
                       (const float*)dout, M, K, chunk < 1 ? 1 : chunk,
                       ktshift);
    hipLaunchKernelGGL(colsum_f32_fold_kernel, dim3(kb), dim3(256), 0,
                       (hipStream_t)strm, (float*)db, (const float*)partial,
                       K, (int)parts);
}
