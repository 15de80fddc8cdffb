// Fused loss + prec@k metrics for [M, C] logits (bf16 / f32), int64 targets.
// Replaces the F.cross_entropy + topk/eq/expand/sum chain (and its three
// host syncs per batch) of the evaluation loops (ref: nn_ops.py:94-106,
// distributed_evaluator.py:90-106), and gives the training step a
// Prec@1/Prec@5 (ref: nn_ops.py:80-86) that lives inside the captured graph.
//
// Softmax cross-entropy already walks every logit of a row with one wave;
// the rank of the target logit falls out of the same walk:
//
//   rank(m) = #{c != t : x[c] > x[t] or isnan(x[c])} + #{c < t : x[c] == x[t]}
//
// (ties go to the lower index, so no sort order is involved). Row m is a hit
// at k iff rank(m) < min(k, C). A NaN at the target is a miss for every k. A
// row whose target is outside [0, C) is INVALID: the target is never used as
// an index, the row adds 0 to the loss sum and to every hit count and is
// counted on its own.
//
// Two kernels per call, no atomics:
//   row kernel : one wave per row, 4 waves per block, capped grid striding
//                over rows. The row is read ONCE into registers (C <= 2048);
//                max, sum-exp and the rank compare all run on the registers.
//                Longer rows take the same code with the registers replaced
//                by re-reads (RS == 0). Writes row_ws[m], rank[m] (-1 =
//                invalid) and, for training, lse[m].
//   fold kernel: ONE block, fixed per-thread stride then a fixed tree (as
//                rowloss_fold[_f32]_kernel), integer sums for the counts; the
//                same block adds the batch totals into the state buffer —
//                launches on one stream are ordered, so that is race-free.
//
// The row loss is the expression of softmax_ce_fwd[_f32]_kernel in the same
// lane / shuffle order (f32 math for bf16 logits, f64 for f32 logits), so the
// training entry's loss / lse / row_ws equal ps_softmax_ce_fwd[_f32]'s bit
// for bit on valid targets.
//
// State buffer (8-byte slots): [0] f64 loss sum, [1] i64 valid rows,
// [2] i64 invalid rows, [3 .. 3+nk) i64 hits per k; nk <= 4.
#include "common.h"

typedef unsigned short ushort8_t __attribute__((ext_vector_type(8)));

#define MET_MAX_K 4
#define MET_GRID_CAP 256      // one block (4 rows in flight) per CU

struct MetKs { int nk; int k[MET_MAX_K]; };   // k already clamped to C

__device__ __forceinline__ float met_wave_max(float v) {
#pragma unroll
    for (int m = 32; m; m >>= 1)
        v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

__device__ __forceinline__ float met_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m; m >>= 1)
        v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ double met_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m; m >>= 1)
        v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ int met_wave_sum(int v) {
#pragma unroll
    for (int m = 32; m; m >>= 1)
        v += __shfl_xor(v, m);
    return v;
}

// 8 consecutive bf16 at p, n (1..8) of them in bounds. The 16-B vector load
// is used only where the address is 16-B aligned (a row start is not when
// C % 8 != 0 or the tensor base is a 2-B-aligned view); otherwise the widest
// aligned access, down to element loads. All lanes of a wave share the
// row's alignment, so the branch does not diverge.
__device__ __forceinline__ void met_load8(float* __restrict__ v,
                                          const unsigned short* __restrict__ p,
                                          int n)
{
    unsigned short us[8];
    if (n == 8) {
        const size_t a = (size_t)p;
        if ((a & 15) == 0) {
            ushort8_t w = *(const ushort8_t*)p;
#pragma unroll
            for (int u = 0; u < 8; ++u) us[u] = w[u];
        } else if ((a & 3) == 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                unsigned int w = ((const unsigned int*)p)[u];
                us[2 * u] = (unsigned short)(w & 0xffffu);
                us[2 * u + 1] = (unsigned short)(w >> 16);
            }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) us[u] = p[u];
        }
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) us[u] = u < n ? p[u] : (unsigned short)0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = bf16_to_f32(us[u]);
}

// hit / miss contribution of element (value v at class c) against target
// (value xt at class t)
__device__ __forceinline__ int met_above(float v, int c, float xt, int t) {
    return (c != t && (v > xt || v != v)) || (c < t && v == xt);
}

// ---- bf16 rows: lane owns 8-element chunks at lane*8 + j*512 (the layout of
// softmax_ce_fwd_kernel); RS chunks live in registers, RS == 0 re-reads ----
template <int RS, bool TRAIN>
__global__ __launch_bounds__(256) void ce_metrics_row_kernel(
    float* __restrict__ row_ws,            // [M] per-row loss (0 if invalid)
    float* __restrict__ lse,               // [M] (TRAIN only)
    int* __restrict__ rank,                // [M] rank, -1 = invalid target
    const unsigned short* __restrict__ x,  // [M, C] bf16
    const long* __restrict__ target,       // [M]
    long M, int C)
{
    const int lane = threadIdx.x & 63;
    const long nwave = (long)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < M;
         row += nwave) {
        const unsigned short* xr = x + row * C;
        const long t64 = target[row];
        const bool valid = t64 >= 0 && t64 < (long)C;
        const int t = valid ? (int)t64 : 0;
        const float xt = valid ? bf16_to_f32(xr[t]) : 0.f;

        constexpr int NR = RS > 0 ? RS : 1;
        float v[NR][8];
        if constexpr (RS > 0) {
#pragma unroll
            for (int j = 0; j < RS; ++j) {
                const int base = lane * 8 + j * 512;
                const int n = C - base < 8 ? C - base : 8;
                if (n > 0) met_load8(v[j], xr + base, n);
            }
        }

        float mx = -3.4e38f;
        float s = 0.f;
        int cnt = 0;
        if constexpr (RS > 0) {
#pragma unroll
            for (int j = 0; j < RS; ++j) {
                const int n = C - (lane * 8 + j * 512);
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (u < n) mx = fmaxf(mx, v[j][u]);
            }
            mx = met_wave_max(mx);
#pragma unroll
            for (int j = 0; j < RS; ++j) {
                const int base = lane * 8 + j * 512;
                const int n = C - base;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (u < n) {
                        s += __expf(v[j][u] - mx);
                        cnt += met_above(v[j][u], base + u, xt, t);
                    }
            }
        } else {
            for (int base = lane * 8; base < C; base += 512) {
                const int n = C - base < 8 ? C - base : 8;
                met_load8(v[0], xr + base, n);
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (u < n) mx = fmaxf(mx, v[0][u]);
            }
            mx = met_wave_max(mx);
            for (int base = lane * 8; base < C; base += 512) {
                const int n = C - base < 8 ? C - base : 8;
                met_load8(v[0], xr + base, n);
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (u < n) {
                        s += __expf(v[0][u] - mx);
                        cnt += met_above(v[0][u], base + u, xt, t);
                    }
            }
        }
        s = met_wave_sum(s);
        cnt = met_wave_sum(cnt);

        if (lane == 0) {
            float l = mx + __logf(s);
            if constexpr (TRAIN) lse[row] = l;
            row_ws[row] = valid ? l - xt : 0.f;
            rank[row] = !valid ? -1 : (xt != xt ? C : cnt);
        }
    }
}

// ---- f32 rows: lane owns elements lane + 64*j (the layout of
// softmax_ce_fwd_f32_kernel; 4-B element loads, coalesced across the wave,
// aligned for any C and any f32 view); f64 row math ----
template <int RS, bool TRAIN>
__global__ __launch_bounds__(256) void ce_metrics_row_f32_kernel(
    double* __restrict__ row_ws, double* __restrict__ lse,
    int* __restrict__ rank, const float* __restrict__ x,
    const long* __restrict__ target, long M, int C)
{
    const int lane = threadIdx.x & 63;
    const long nwave = (long)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < M;
         row += nwave) {
        const float* xr = x + row * C;
        const long t64 = target[row];
        const bool valid = t64 >= 0 && t64 < (long)C;
        const int t = valid ? (int)t64 : 0;
        const float xt = valid ? xr[t] : 0.f;

        constexpr int NR = RS > 0 ? RS : 1;
        float v[NR];
        float mx = -INFINITY;
        double s = 0.0;
        int cnt = 0;
        if constexpr (RS > 0) {
#pragma unroll
            for (int j = 0; j < RS; ++j) {
                const int c = lane + 64 * j;
                v[j] = c < C ? xr[c] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < RS; ++j)
                if (lane + 64 * j < C) mx = fmaxf(mx, v[j]);
            mx = met_wave_max(mx);
#pragma unroll
            for (int j = 0; j < RS; ++j) {
                const int c = lane + 64 * j;
                if (c < C) {
                    s += exp((double)v[j] - (double)mx);
                    cnt += met_above(v[j], c, xt, t);
                }
            }
        } else {
            for (int c = lane; c < C; c += 64) mx = fmaxf(mx, xr[c]);
            mx = met_wave_max(mx);
            for (int c = lane; c < C; c += 64) {
                const float e = xr[c];
                s += exp((double)e - (double)mx);
                cnt += met_above(e, c, xt, t);
            }
        }
        s = met_wave_sum(s);
        cnt = met_wave_sum(cnt);

        if (lane == 0) {
            double l = (double)mx + log(s);
            if constexpr (TRAIN) lse[row] = l;
            row_ws[row] = valid ? l - (double)xt : 0.0;
            rank[row] = !valid ? -1 : (xt != xt ? C : cnt);
        }
    }
}

// deterministic fold: ONE block, fixed-stride per-thread partials + fixed
// tree, the loss in W (f32 / f64) exactly as rowloss_fold[_f32]_kernel, the
// counts as integers. Thread 0 then writes the mean loss (TRAIN) and adds the
// batch totals into the state buffer.
template <typename W, bool TRAIN>
__global__ __launch_bounds__(256) void ce_metrics_fold_kernel(
    float* __restrict__ loss,              // [1] mean over M (TRAIN only)
    unsigned long long* __restrict__ state,   // [3 + nk] 8-byte slots
    const W* __restrict__ row_ws, const int* __restrict__ rank,
    long M, MetKs ks)
{
    __shared__ W red[256];
    __shared__ int redi[2 + MET_MAX_K][256];
    W acc = (W)0;
    int ci[2 + MET_MAX_K];    // valid, invalid, hits per k (M < 2^31 rows)
#pragma unroll
    for (int q = 0; q < 2 + MET_MAX_K; ++q) ci[q] = 0;
    for (long i = threadIdx.x; i < M; i += 256) {
        acc += row_ws[i];
        const int r = rank[i];
        ci[0] += r >= 0;
        ci[1] += r < 0;
#pragma unroll
        for (int q = 0; q < MET_MAX_K; ++q)
            ci[2 + q] += q < ks.nk && r >= 0 && r < ks.k[q];
    }
    red[threadIdx.x] = acc;
#pragma unroll
    for (int q = 0; q < 2 + MET_MAX_K; ++q) redi[q][threadIdx.x] = ci[q];
    __syncthreads();
#pragma unroll
    for (int w = 128; w; w >>= 1) {
        if (threadIdx.x < w) {
            red[threadIdx.x] += red[threadIdx.x + w];
#pragma unroll
            for (int q = 0; q < 2 + MET_MAX_K; ++q)
                redi[q][threadIdx.x] += redi[q][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if constexpr (TRAIN) {
            if constexpr (sizeof(W) == 4) loss[0] = red[0] / (float)M;
            else loss[0] = (float)(red[0] / (double)M);
        }
        double* sum = (double*)state;
        sum[0] += (double)red[0];
        long long* cs = (long long*)state;
        cs[1] += redi[0][0];
        cs[2] += redi[1][0];
        for (int q = 0; q < ks.nk; ++q) cs[3 + q] += redi[2 + q][0];
    }
}

static inline MetKs met_ks(int C, int nk, int k0, int k1, int k2, int k3) {
    MetKs ks;
    const int k[MET_MAX_K] = {k0, k1, k2, k3};
    ks.nk = nk < 0 ? 0 : (nk > MET_MAX_K ? MET_MAX_K : nk);
    for (int q = 0; q < MET_MAX_K; ++q) ks.k[q] = k[q] < C ? k[q] : C;
    return ks;
}

static inline unsigned met_blocks(long M) {
    long b = (M + 3) / 4;
    return (unsigned)(b < 1 ? 1 : (b > MET_GRID_CAP ? MET_GRID_CAP : b));
}

#define MET_LAUNCH_ROW(KERN, RS, WT, XT)                                     \
    hipLaunchKernelGGL((KERN<RS, TRAIN>), dim3(met_blocks(M)), dim3(256), 0, \
                       strm, (WT*)row_ws, (WT*)lse, (int*)rank,              \
                       (const XT*)logits, (const long*)target, M, C)

template <bool TRAIN>
static void met_run_bf16(void* loss, void* lse, void* row_ws, void* rank,
                         void* state, const void* logits, const void* target,
                         long M, int C, MetKs ks, hipStream_t strm)
{
    if (M <= 0) {}   // nothing to walk; the fold still writes the outputs
    else if (C <= 512) MET_LAUNCH_ROW(ce_metrics_row_kernel, 1, float, unsigned short);
    else if (C <= 1024) MET_LAUNCH_ROW(ce_metrics_row_kernel, 2, float, unsigned short);
    else if (C <= 2048) MET_LAUNCH_ROW(ce_metrics_row_kernel, 4, float, unsigned short);
    else MET_LAUNCH_ROW(ce_metrics_row_kernel, 0, float, unsigned short);
    hipLaunchKernelGGL((ce_metrics_fold_kernel<float, TRAIN>), dim3(1),
                       dim3(256), 0, strm, (float*)loss,
                       (unsigned long long*)state, (const float*)row_ws,
                       (const int*)rank, M, ks);
}

template <bool TRAIN>
static void met_run_f32(void* loss, void* lse, void* row_ws, void* rank,
                        void* state, const void* logits, const void* target,
                        long M, int C, MetKs ks, hipStream_t strm)
{
    if (M <= 0) {}
    else if (C <= 128) MET_LAUNCH_ROW(ce_metrics_row_f32_kernel, 2, double, float);
    else if (C <= 1024) MET_LAUNCH_ROW(ce_metrics_row_f32_kernel, 16, double, float);
    else if (C <= 2048) MET_LAUNCH_ROW(ce_metrics_row_f32_kernel, 32, double, float);
    else MET_LAUNCH_ROW(ce_metrics_row_f32_kernel, 0, double, float);
    hipLaunchKernelGGL((ce_metrics_fold_kernel<double, TRAIN>), dim3(1),
                       dim3(256), 0, strm, (float*)loss,
                       (unsigned long long*)state, (const double*)row_ws,
                       (const int*)rank, M, ks);
}

// Evaluation: state += (loss sum, valid, invalid, hits per k) of this batch.
// row_ws: [M] f32 (bf16 logits) / f64 (f32 logits); rank: [M] i32. Caller
// workspaces, no allocation or sync here.
extern "C" void ps_ce_metrics(
    void* state, void* row_ws, void* rank, const void* logits,
    const void* target, long M, int C, int nk, int k0, int k1, int k2, int k3,
    void* strm)
{
    met_run_bf16<false>(nullptr, nullptr, row_ws, rank, state, logits, target,
                        M, C, met_ks(C, nk, k0, k1, k2, k3),
                        (hipStream_t)strm);
}

extern "C" void ps_ce_metrics_f32(
    void* state, void* row_ws, void* rank, const void* logits,
    const void* target, long M, int C, int nk, int k0, int k1, int k2, int k3,
    void* strm)
{
    met_run_f32<false>(nullptr, nullptr, row_ws, rank, state, logits, target,
                       M, C, met_ks(C, nk, k0, k1, k2, k3), (hipStream_t)strm);
}

// Training: loss / lse / row_ws of ps_softmax_ce_fwd[_f32] plus the state
// update, in the same pass over the logits. Backward is ps_softmax_ce_bwd.
extern "C" void ps_softmax_ce_fwd_metrics(
    void* loss, void* lse, void* row_ws, void* rank, void* state,
    const void* logits, const void* target, long M, int C,
    int nk, int k0, int k1, int k2, int k3, void* strm)
{
    met_run_bf16<true>(loss, lse, row_ws, rank, state, logits, target, M, C,
                       met_ks(C, nk, k0, k1, k2, k3), (hipStream_t)strm);
}

extern "C" void ps_softmax_ce_fwd_metrics_f32(
    void* loss, void* lse, void* row_ws, void* rank, void* state,
    const void* logits, const void* target, long M, int C,
    int nk, int k0, int k1, int k2, int k3, void* strm)
{
    met_run_f32<true>(loss, lse, row_ws, rank, state, logits, target, M, C,
                      met_ks(C, nk, k0, k1, k2, k3), (hipStream_t)strm);
}
