// Counter-based dropout / ReLU family: y = (keep && (!relu || x > 0)) ?
// x * scale : 0, with a bit-packed combined keep-and-positive mask for the
// backward (same layout as batchnorm.hip's relu mask: bit k of byte i is
// element 8*i+k).
//
// Replaces the at::native dropout / relu the reference reaches through
// nn.Dropout / nn.ReLU (ref: src/model_ops/vgg.py:22-30 classifier head).
//
// RNG: Philox4x32-10. Element e takes word (e & 3) of the block whose
// counter is (lo32(e>>2), hi32(e>>2), step, (stream << 16) | salt) under key
// (lo32(seed), hi32(seed)) — a pure function of the element index, so the
// mask does not depend on grid geometry, vector width or alignment path and
// the CPU oracle (ops/functional.py dropout_keep_mask) reproduces it bit for
// bit. keep iff word >= thr, thr = round(p * 2^32) computed on the host: no
// float compare on the device.
//
// The step lives in DEVICE memory (*step_ptr, int64) and is bumped by a
// one-thread kernel launched right behind the forward on the same stream:
// a captured step replays with a fresh mask every time, with kernel nodes
// only (no memcpy/memset node, no atomic), and stays bit-identical to eager
// stepping.
//
// Each lane handles 8 elements — one 16-B access for bf16, two for f32 —
// i.e. two Philox blocks and one mask byte. 16-B accesses are taken only
// when every pointer is 16-B aligned (host check); misaligned views run the
// same octet loop with scalar accesses.
#include "common.h"
#include "philox.h"

typedef unsigned short ushort8_t __attribute__((ext_vector_type(8)));

struct DropRng {
    unsigned thr, k0, k1, c2, c3;
};

// keep bits of the 4 elements of Philox block `blk` (bit u: element 4*blk+u)
__device__ __forceinline__ unsigned keep4(long blk, const DropRng& g) {
    unsigned w[4];
    philox4x32_10((unsigned)blk, (unsigned)((unsigned long long)blk >> 32),
                  g.c2, g.c3, g.k0, g.k1, w);
    return (unsigned)(w[0] >= g.thr) | ((unsigned)(w[1] >= g.thr) << 1) |
           ((unsigned)(w[2] >= g.thr) << 2) | ((unsigned)(w[3] >= g.thr) << 3);
}

// keep modes (wave-uniform): ALL — no dropout, no Philox work (pure ReLU);
// RNG — Philox mask; NONE — p >= 1, everything dropped, no Philox work
enum { KEEP_ALL = 0, KEEP_RNG = 1, KEEP_NONE = 2 };

__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const unsigned short* p) {
    return bf16_to_f32(*p);
}
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(unsigned short* p, float v) {
    *p = f32_to_bf16(v);
}

template <bool VEC>
__device__ __forceinline__ void load8(const float* p, float v[8]) {
    if (VEC) {
        float4_t a = ((const float4_t*)p)[0], b = ((const float4_t*)p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[u];
    }
}
template <bool VEC>
__device__ __forceinline__ void load8(const unsigned short* p, float v[8]) {
    if (VEC) {
        ushort8_t a = *(const ushort8_t*)p;
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = bf16_to_f32(a[u]);
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = bf16_to_f32(p[u]);
    }
}
template <bool VEC>
__device__ __forceinline__ void store8(float* p, const float v[8]) {
    if (VEC) {
        float4_t a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
        ((float4_t*)p)[0] = a;
        ((float4_t*)p)[1] = b;
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = v[u];
    }
}
template <bool VEC>
__device__ __forceinline__ void store8(unsigned short* p, const float v[8]) {
    if (VEC) {
        ushort8_t o;
#pragma unroll
        for (int u = 0; u < 8; ++u) o[u] = f32_to_bf16(v[u]);
        *(ushort8_t*)p = o;
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = f32_to_bf16(v[u]);
    }
}

// thread covers one element octet (= one mask byte); the n % 8 scalar tail
// (and its partial mask byte) is handled by thread 0.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void act_drop_fwd_kernel(
    T* __restrict__ y, unsigned char* __restrict__ mask,
    const T* __restrict__ x, long n, int relu, int mode, float scale,
    DropRng g, const long long* __restrict__ step_ptr)
{
    EW_IDX
    if (mode == KEEP_RNG) g.c2 = (unsigned)(unsigned long long)*step_ptr;
    const long noct = n >> 3;
    for (long i = gid; i < noct; i += stride) {
        float v[8];
        load8<VEC>(x + i * 8, v);
        unsigned keep = mode == KEEP_NONE ? 0u : 0xffu;
        if (mode == KEEP_RNG)
            keep = keep4(2 * i, g) | (keep4(2 * i + 1, g) << 4);
        unsigned bits = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool on = ((keep >> u) & 1u) && (!relu || v[u] > 0.f);
            bits |= (unsigned)on << u;
            v[u] = on ? v[u] * scale : 0.f;
        }
        store8<VEC>(y + i * 8, v);
        mask[i] = (unsigned char)bits;
    }
    if (gid == 0 && (n & 7)) {
        const long e0 = noct << 3;
        unsigned keep = mode == KEEP_NONE ? 0u : 0xffu;
        if (mode == KEEP_RNG) {
            keep = keep4(2 * noct, g);
            if (n - e0 > 4) keep |= keep4(2 * noct + 1, g) << 4;
        }
        unsigned bits = 0;
        for (long e = e0; e < n; ++e) {
            const int u = (int)(e - e0);
            const float f = ld1(x + e);
            const bool on = ((keep >> u) & 1u) && (!relu || f > 0.f);
            bits |= (unsigned)on << u;
            st1(y + e, on ? f * scale : 0.f);
        }
        mask[noct] = (unsigned char)bits;
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void act_drop_bwd_kernel(
    T* __restrict__ dx, const T* __restrict__ dy,
    const unsigned char* __restrict__ mask, long n, float scale)
{
    EW_IDX
    const long noct = n >> 3;
    for (long i = gid; i < noct; i += stride) {
        float v[8];
        load8<VEC>(dy + i * 8, v);
        const unsigned bits = mask[i];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            v[u] = ((bits >> u) & 1u) ? v[u] * scale : 0.f;
        store8<VEC>(dx + i * 8, v);
    }
    if (gid == 0 && (n & 7)) {
        const long e0 = noct << 3;
        const unsigned bits = mask[noct];
        for (long e = e0; e < n; ++e)
            st1(dx + e, ((bits >> (int)(e - e0)) & 1u) ? ld1(dy + e) * scale
                                                       : 0.f);
    }
}

__global__ void rng_advance_kernel(long long* step) { *step += 1; }

static inline bool al16(const void* a, const void* b) {
    return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;
}

template <typename T>
static void launch_fwd(void* y, void* mask, const void* x, long n, int relu,
                       int mode, float scale, DropRng g, const void* step_ptr,
                       hipStream_t strm)
{
    int blocks; ew_grid(n >> 3, 256, &blocks);
    if (al16(y, x))
        hipLaunchKernelGGL((act_drop_fwd_kernel<T, true>), dim3(blocks),
                           dim3(256), 0, strm, (T*)y, (unsigned char*)mask,
                           (const T*)x, n, relu, mode, scale, g,
                           (const long long*)step_ptr);
    else
        hipLaunchKernelGGL((act_drop_fwd_kernel<T, false>), dim3(blocks),
                           dim3(256), 0, strm, (T*)y, (unsigned char*)mask,
                           (const T*)x, n, relu, mode, scale, g,
                           (const long long*)step_ptr);
}

template <typename T>
static void launch_bwd(void* dx, const void* dy, const void* mask, long n,
                       float scale, hipStream_t strm)
{
    int blocks; ew_grid(n >> 3, 256, &blocks);
    if (al16(dx, dy))
        hipLaunchKernelGGL((act_drop_bwd_kernel<T, true>), dim3(blocks),
                           dim3(256), 0, strm, (T*)dx, (const T*)dy,
                           (const unsigned char*)mask, n, scale);
    else
        hipLaunchKernelGGL((act_drop_bwd_kernel<T, false>), dim3(blocks),
                           dim3(256), 0, strm, (T*)dx, (const T*)dy,
                           (const unsigned char*)mask, n, scale);
}

extern "C" void ps_rng_advance(void* step_ptr, void* strm) {
    hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0,
                       (hipStream_t)strm, (long long*)step_ptr);
}

// thr == 0: keep everything (no Philox work; with relu == 1 a pure ReLU).
// scale == 0 is the host's encoding of p >= 1 (1/(1-p) does not exist):
// everything is dropped, again with no Philox work. Otherwise the Philox
// mask at step *step_ptr, and the counter is advanced behind the forward.
extern "C" void ps_act_drop_fwd(
    void* y, void* mask, const void* x, long n, int dtype, int relu,
    unsigned int thr, float scale, unsigned long long seed,
    unsigned int salt_stream, void* step_ptr, void* strm)
{
    const int mode = scale == 0.f ? KEEP_NONE : (thr ? KEEP_RNG : KEEP_ALL);
    DropRng g = {thr, (unsigned)seed, (unsigned)(seed >> 32), 0u, salt_stream};
    if (dtype == PS_BF16)
        launch_fwd<unsigned short>(y, mask, x, n, relu, mode, scale, g,
                                   step_ptr, (hipStream_t)strm);
    else
        launch_fwd<float>(y, mask, x, n, relu, mode, scale, g, step_ptr,
                          (hipStream_t)strm);
    if (mode == KEEP_RNG) ps_rng_advance(step_ptr, strm);
}

extern "C" void ps_act_drop_bwd(void* dx, const void* dy, const void* mask,
                                long n, int dtype, float scale, void* strm)
{
    if (dtype == PS_BF16)
        launch_bwd<unsigned short>(dx, dy, mask, n, scale, (hipStream_t)strm);
    else
        launch_bwd<float>(dx, dy, mask, n, scale, (hipStream_t)strm);
}
