// Fused LARS (layer-wise adaptive rate scaling, You et al.) over the flat
// parameter buffer, with the learning rate read from device memory so a
// captured hipGraph follows the schedule.
//
// A *segment* is one parameter tensor of the flat layout (start, numel,
// adapt = ndim > 1). A *chunk* is a LARS_CHUNK-element piece of a segment
// counted from the segment's own start (the last one short), so a chunk
// never spans two tensors. The host builds the tables once per layout:
//
//   chunk_start[c]  i64  flat offset of chunk c; chunk_start[nchunk] is the
//                        end of the buffer. Chunk starts are multiples of 8.
//   chunk_len[c]    i32  the parameter's own elements in the chunk
//   chunk_seg[c]    i32  its segment
//   seg_chunk0[s]   i32  first chunk of segment s (seg_chunk0[nseg] = nchunk)
//   seg_adapt[s]    i32  1 where the trust ratio and the decay apply
//
// One step() of a region (a contiguous chunk range == a contiguous segment
// range) is three launches, whatever the number of tensors:
//
//   1. lars_norm_chunks   one block per chunk: (sum w^2, sum g^2) of the
//                         chunk's own elements (not the <= 7 alignment-gap
//                         elements behind a tensor), every element widened
//                         to f64 and accumulated in f64: lane-strided quads
//                         in ascending order, a fixed shuffle tree per wave,
//                         the four waves folded 0..3 through LDS. With
//                         `advance`, thread 0 of block 0 also latches
//                         lr_cur = lr_table[min(step_ctr, T-1)] and
//                         increments step_ctr; nobody in this launch reads
//                         lr_cur, so the kernel boundary orders the latch
//                         against its readers.
//   2. lars_norm_segments one wave per segment: lane l folds the chunk
//                         partials l, l+64, ... in ascending order, then the
//                         same shuffle tree. In f64, wn = sqrt(Sw),
//                         gn = grad_scale * sqrt(Sg),
//                           ratio = eta*wn / (gn + wd*wn + eps)
//                                   if adapt && wn > 0 && gn > 0, else 1
//                         local_lr[s] = (float)((double)lr_cur * ratio)
//                         wd_seg[s]   = adapt ? (float)wd : 0
//   3. lars_update        one block per chunk over the region, gap elements
//                         included (they take the segment's step size; their
//                         gradient is zero), lars_update_elem per element,
//                         optional wire re-pack as ps_fused_sgd.
//
// f64 because the kernels are memory-bound (the FMAs are free) and a 2^21
// element sum of squares then carries a relative error below n * 2^-52
// instead of f32's n * 2^-24, which would reach the trust ratio's 4th digit.
// No atomics, no host sync, no allocation: capturable.
#include "common.h"
#include "sgd_update.h"

#define LARS_CHUNK 4096
#define LARS_THREADS 256

__device__ __forceinline__ double lars_wave_sum(double v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    return v;   // lane 0 holds the sum
}

template <bool G_BF16>
__global__ __launch_bounds__(LARS_THREADS) void lars_norm_chunks(
    const float* __restrict__ w, const void* __restrict__ g_,
    const long* __restrict__ chunk_start, const int* __restrict__ chunk_len,
    int chunk0, double* __restrict__ partial,
    const float* __restrict__ lr_table, int T, long* __restrict__ step_ctr,
    float* __restrict__ lr_cur, int advance)
{
    const int c = chunk0 + blockIdx.x;
    const long base = chunk_start[c];
    const int len = chunk_len[c];
    const int nvec = len >> 2;
    const int tid = threadIdx.x;

    if (advance && blockIdx.x == 0 && tid == 0) {
        long s = *step_ctr;
        long i = s < (long)T - 1 ? s : (long)T - 1;
        *lr_cur = lr_table[i < 0 ? 0 : i];
        *step_ctr = s + 1;
    }

    const float4_t* wv = (const float4_t*)(w + base);
    double sw = 0.0, sg = 0.0;
    for (int v = tid; v < nvec; v += LARS_THREADS) {
        float4_t a = wv[v];
        float4_t b;
        if constexpr (G_BF16) {
            ushort4_t u = ((const ushort4_t*)((const unsigned short*)g_ + base))[v];
            b = {bf16_to_f32(u.x), bf16_to_f32(u.y), bf16_to_f32(u.z), bf16_to_f32(u.w)};
        } else {
            b = ((const float4_t*)((const float*)g_ + base))[v];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double x = (double)a[k], y = (double)b[k];
            sw = fma(x, x, sw);
            sg = fma(y, y, sg);
        }
    }
    // the len % 4 tail: thread 0, after its quads
    if (tid == 0) {
        for (int e = nvec << 2; e < len; ++e) {
            double x = (double)w[base + e];
            double y = G_BF16
                ? (double)bf16_to_f32(((const unsigned short*)g_)[base + e])
                : (double)((const float*)g_)[base + e];
            sw = fma(x, x, sw);
            sg = fma(y, y, sg);
        }
    }
    sw = lars_wave_sum(sw);
    sg = lars_wave_sum(sg);
    __shared__ double red[2][LARS_THREADS / WAVE];
    if ((tid & (WAVE - 1)) == 0) {
        red[0][tid / WAVE] = sw;
        red[1][tid / WAVE] = sg;
    }
    __syncthreads();
    if (tid == 0) {
        double a = red[0][0], b = red[1][0];
#pragma unroll
        for (int i = 1; i < LARS_THREADS / WAVE; ++i) { a += red[0][i]; b += red[1][i]; }
        partial[2 * (long)c] = a;
        partial[2 * (long)c + 1] = b;
    }
}

__global__ __launch_bounds__(WAVE) void lars_norm_segments(
    const double* __restrict__ partial, const int* __restrict__ seg_chunk0,
    const int* __restrict__ seg_adapt, int seg0,
    const float* __restrict__ lr_cur, double grad_scale, double eta, double wd,
    double eps, double* __restrict__ seg_sums, float* __restrict__ local_lr,
    float* __restrict__ wd_seg)
{
    const int s = seg0 + blockIdx.x;
    const int c0 = seg_chunk0[s], c1 = seg_chunk0[s + 1];
    double sw = 0.0, sg = 0.0;
    for (int c = c0 + (int)threadIdx.x; c < c1; c += WAVE) {
        sw += partial[2 * (long)c];
        sg += partial[2 * (long)c + 1];
    }
    sw = lars_wave_sum(sw);
    sg = lars_wave_sum(sg);
    if (threadIdx.x == 0) {
        const bool adapt = seg_adapt[s] != 0;
        double wn = sqrt(sw);
        double gn = grad_scale * sqrt(sg);
        double ratio = 1.0;
        if (adapt && wn > 0.0 && gn > 0.0) ratio = eta * wn / (gn + wd * wn + eps);
        seg_sums[2 * (long)s] = sw;
        seg_sums[2 * (long)s + 1] = sg;
        local_lr[s] = (float)((double)(*lr_cur) * ratio);
        wd_seg[s] = adapt ? (float)wd : 0.0f;
    }
}

template <bool G_BF16, int WIRE>   // WIRE: 0 none, 1 f32, 2 bf16
__global__ __launch_bounds__(LARS_THREADS) void lars_update(
    float* __restrict__ w, const void* __restrict__ g_, float* __restrict__ m,
    void* __restrict__ wire_, const long* __restrict__ chunk_start,
    const int* __restrict__ chunk_seg, int chunk0,
    const float* __restrict__ local_lr, const float* __restrict__ wd_seg,
    float mu, float scale)
{
    const int c = chunk0 + blockIdx.x;
    const long base = chunk_start[c];
    // up to the next chunk: the alignment gap behind a tensor travels with
    // its last chunk; both ends are multiples of 8
    const int nvec = (int)((chunk_start[c + 1] - base) >> 2);
    const int seg = chunk_seg[c];
    const float llr = local_lr[seg];
    const float wds = wd_seg[seg];
    float4_t* wp = (float4_t*)(w + base);
    float4_t* mp = (float4_t*)(m + base);
    for (int v = threadIdx.x; v < nvec; v += LARS_THREADS) {
        float4_t wv = wp[v];
        float4_t mv = mp[v];
        float4_t gv;
        if constexpr (G_BF16) {
            ushort4_t u = ((const ushort4_t*)((const unsigned short*)g_ + base))[v];
            gv = {bf16_to_f32(u.x), bf16_to_f32(u.y), bf16_to_f32(u.z), bf16_to_f32(u.w)};
        } else {
            gv = ((const float4_t*)((const float*)g_ + base))[v];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float wk = wv[k], mk = mv[k];
            lars_update_elem(wk, mk, gv[k], scale, llr, mu, wds);
            wv[k] = wk; mv[k] = mk;
        }
        wp[v] = wv;
        mp[v] = mv;
        if constexpr (WIRE == 1) {
            ((float4_t*)((float*)wire_ + base))[v] = wv;
        } else if constexpr (WIRE == 2) {
            ushort4_t o = {f32_to_bf16(wv.x), f32_to_bf16(wv.y),
                           f32_to_bf16(wv.z), f32_to_bf16(wv.w)};
            ((ushort4_t*)((unsigned short*)wire_ + base))[v] = o;
        }
    }
}

// Stages 1 + 2 over chunks [chunk0, chunk0 + nchunk) == segments
// [seg0, seg0 + nseg). w / g are the bases of the WHOLE flat buffers (the
// tables hold flat offsets). Returns nonzero and launches nothing for
// arguments it rejects.
extern "C" int ps_lars_norms(
    const void* w, const void* g, int g_dtype,
    const void* chunk_start, const void* chunk_len, int chunk0, int nchunk,
    const void* seg_chunk0, const void* seg_adapt, int seg0, int nseg,
    void* partial, void* seg_sums, void* local_lr, void* wd_seg,
    const void* lr_table, int T, void* step_ctr, void* lr_cur, int advance,
    double grad_scale, double eta, double wd, double eps, void* stream)
{
    if (chunk0 < 0 || nchunk < 0 || seg0 < 0 || nseg < 0 || T < 1) return 1;
    if (g_dtype != PS_F32 && g_dtype != PS_BF16) return 2;
    if (advance && nchunk == 0) return 3;   // the latch rides on stage 1
    hipStream_t s = (hipStream_t)stream;
    if (nchunk > 0) {
        dim3 grid(nchunk), block(LARS_THREADS);
        if (g_dtype == PS_BF16)
            hipLaunchKernelGGL((lars_norm_chunks<true>), grid, block, 0, s,
                (const float*)w, g, (const long*)chunk_start,
                (const int*)chunk_len, chunk0, (double*)partial,
                (const float*)lr_table, T, (long*)step_ctr, (float*)lr_cur,
                advance);
        else
            hipLaunchKernelGGL((lars_norm_chunks<false>), grid, block, 0, s,
                (const float*)w, g, (const long*)chunk_start,
                (const int*)chunk_len, chunk0, (double*)partial,
                (const float*)lr_table, T, (long*)step_ctr, (float*)lr_cur,
                advance);
    }
    if (nseg > 0)
        hipLaunchKernelGGL(lars_norm_segments, dim3(nseg), dim3(WAVE), 0, s,
            (const double*)partial, (const int*)seg_chunk0,
            (const int*)seg_adapt, seg0, (const float*)lr_cur, grad_scale,
            eta, wd, eps, (double*)seg_sums, (float*)local_lr, (float*)wd_seg);
    return 0;
}

// Stage 3 over chunks [chunk0, chunk0 + nchunk) with the per-segment step
// sizes stage 2 left in local_lr / wd_seg. wire may be null.
extern "C" int ps_lars_update(
    void* w, const void* g, void* m, void* wire, int g_dtype, int wire_dtype,
    const void* chunk_start, const void* chunk_seg, int chunk0, int nchunk,
    const void* local_lr, const void* wd_seg, float mu, float scale,
    void* stream)
{
    if (chunk0 < 0 || nchunk < 0) return 1;
    if (g_dtype != PS_F32 && g_dtype != PS_BF16) return 2;
    if (wire && wire_dtype != PS_F32 && wire_dtype != PS_BF16) return 2;
    if (nchunk == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(nchunk), block(LARS_THREADS);
#define LU(GB, WI) hipLaunchKernelGGL((lars_update<GB, WI>), grid, block, 0, s, \
        (float*)w, g, (float*)m, wire, (const long*)chunk_start,                 \
        (const int*)chunk_seg, chunk0, (const float*)local_lr,                   \
        (const float*)wd_seg, mu, scale)
    const int wi = !wire ? 0 : (wire_dtype == PS_BF16 ? 2 : 1);
    if (g_dtype == PS_BF16) { if (wi == 0) LU(true, 0); else if (wi == 1) LU(true, 1); else LU(true, 2); }
    else                    { if (wi == 0) LU(false, 0); else if (wi == 1) LU(false, 1); else LU(false, 2); }
#undef LU
    return 0;
}
