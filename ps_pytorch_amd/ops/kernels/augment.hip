// Fused batch loader for device-resident uint8 datasets: one launch gathers
// B samples by index, applies the train-time augmentation (random crop out
// of a reflect- or zero-padded image, horizontal flip), normalizes and
// writes the batch in channels-last (NHWC) memory, plus the B labels.
//
// Replaces the index_select / pad / gather / flip / where / normalize / cast
// chain of data/real.py RealDataset.augment and the trainer's channels-last
// copy (ref: the torchvision stack in src/util.py:36-47).
//
// RNG: Philox4x32-10, one block per batch slot b. Counter
// (b, 0, lo32(step), (stream << 16) | 0xDA7A) under key (lo32(seed),
// hi32(seed)); oy = (w0 * (2p+1)) >> 32, ox = (w1 * (2p+1)) >> 32,
// flip = hflip && (w2 >> 31). The salt 0xDA7A keeps the draws apart from
// the dropout layers' small salts under the same seed. Integer arithmetic
// only: the CPU oracle (ops/functional.py augment_draws / augment_ref)
// reproduces the batch bit for bit.
//
// Source pixel of output (b, h, w), crop first, then flip:
//   w' = flip ? W-1-w : w;  sy = oy + h - p;  sx = ox + w' - p
//   reflect : s < 0 -> -s, s >= L -> 2(L-1) - s   (host checks p <= L-1)
//   constant: an out-of-range source reads uint8 0 (normalized like any
//             other value)
// Value: T((float(u8) - mean255[c]) * inv_std255[c]); subtract and multiply
// are each rounded to f32 (no fma contraction).
//
// With p == 0 and no hflip there is no Philox work, step_ptr may be null and
// the counter is not advanced (the KEEP_ALL convention of dropout.hip).
// Otherwise the step is read from device memory and ps_rng_advance bumps it
// behind the kernel: kernel nodes only, so a captured loader draws fresh
// offsets on every replay.
//
// One thread per output pixel, lanes running along w: the C channel values
// of neighbouring lanes are adjacent in the NHWC output, so a wave's stores
// cover one contiguous span. Indices are NOT range-checked here; the host
// side builds them.
#include "common.h"
#include "philox.h"

#define AUG_SALT 0xDA7Au
#define AUG_MAX_C 4

struct AugParams {
    float mean[AUG_MAX_C], inv_std[AUG_MAX_C];
    unsigned k0, k1, c3;
    int C, H, W, pad, reflect, hflip, rng;
};

__device__ __forceinline__ void aug_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void aug_st(unsigned short* p, float v) {
    *p = f32_to_bf16(v);
}

__device__ __forceinline__ int aug_reflect(int s, int L) {
    s = s < 0 ? -s : s;
    return s >= L ? 2 * (L - 1) - s : s;
}

template <typename T>
__global__ __launch_bounds__(256) void augment_batch_kernel(
    T* __restrict__ out, long long* __restrict__ out_y,
    const unsigned char* __restrict__ x, const long long* __restrict__ y,
    const long long* __restrict__ idx, long npix, AugParams a,
    const long long* __restrict__ step_ptr)
{
    EW_IDX
    const unsigned step = a.rng ? (unsigned)(unsigned long long)*step_ptr : 0u;
    const int H = a.H, W = a.W, C = a.C, p = a.pad;
    const long HW = (long)H * W;
    for (long pix = gid; pix < npix; pix += stride) {
        const long b = pix / HW;
        const int r = (int)(pix - b * HW);
        const int h = r / W, w = r - h * W;
        int oy = 0, ox = 0;
        bool flip = false;
        if (a.rng) {
            unsigned wd[4];
            philox4x32_10((unsigned)b, 0u, step, a.c3, a.k0, a.k1, wd);
            const unsigned long long span = 2ull * (unsigned)p + 1ull;
            oy = (int)((wd[0] * span) >> 32);
            ox = (int)((wd[1] * span) >> 32);
            flip = a.hflip && (wd[2] >> 31);
        }
        int sy = oy + h - p;
        int sx = ox + (flip ? W - 1 - w : w) - p;
        bool inb = true;
        if (a.reflect) {
            sy = aug_reflect(sy, H);
            sx = aug_reflect(sx, W);
        } else {
            inb = sy >= 0 && sy < H && sx >= 0 && sx < W;
            if (!inb) sy = sx = 0;     // keep src inside the image
        }
        const long n = idx[b];
        const unsigned char* src = x + (n * C * H + sy) * W + sx;
        T* o = out + pix * C;
#pragma unroll
        for (int c = 0; c < AUG_MAX_C; ++c) {
            if (c < C) {
                const float u = inb ? (float)src[c * HW] : 0.f;
                aug_st(o + c, __fmul_rn(__fsub_rn(u, a.mean[c]),
                                        a.inv_std[c]));
            }
        }
        if (r == 0) out_y[b] = y[n];
    }
}

extern "C" void ps_rng_advance(void* step_ptr, void* strm);   // dropout.hip

// mean255 / inv_std255: HOST pointers to C floats (copied into the kernel
// arguments at launch). reflect: 1 = reflect padding, 0 = constant 0.
extern "C" void ps_augment_batch(
    void* out, void* out_y, const void* x_u8, const void* y, const void* idx,
    long B, int C, int H, int W, int dtype, int pad, int reflect, int hflip,
    const float* mean255, const float* inv_std255, unsigned long long seed,
    unsigned int stream, void* step_ptr, void* strm)
{
    if (B <= 0) return;
    AugParams a = {};
    for (int c = 0; c < C && c < AUG_MAX_C; ++c) {
        a.mean[c] = mean255[c];
        a.inv_std[c] = inv_std255[c];
    }
    a.k0 = (unsigned)seed;
    a.k1 = (unsigned)(seed >> 32);
    a.c3 = ((stream & 0xFFFFu) << 16) | AUG_SALT;
    a.C = C; a.H = H; a.W = W;
    a.pad = pad; a.reflect = reflect; a.hflip = hflip;
    a.rng = pad > 0 || hflip;
    const long npix = B * (long)H * W;
    int blocks; ew_grid(npix, 256, &blocks);
    if (dtype == PS_BF16)
        hipLaunchKernelGGL(augment_batch_kernel<unsigned short>, dim3(blocks),
                           dim3(256), 0, (hipStream_t)strm,
                           (unsigned short*)out, (long long*)out_y,
                           (const unsigned char*)x_u8, (const long long*)y,
                           (const long long*)idx, npix, a,
                           (const long long*)step_ptr);
    else
        hipLaunchKernelGGL(augment_batch_kernel<float>, dim3(blocks),
                           dim3(256), 0, (hipStream_t)strm, (float*)out,
                           (long long*)out_y, (const unsigned char*)x_u8,
                           (const long long*)y, (const long long*)idx, npix,
                           a, (const long long*)step_ptr);
    if (a.rng) ps_rng_advance(step_ptr, strm);
}
