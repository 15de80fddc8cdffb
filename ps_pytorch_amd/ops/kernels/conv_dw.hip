// Depthwise NHWC convolution (groups == C == K), bf16 or f32 storage, all
// math in f32, on the VALU. With one input channel per output channel there
// is no contraction for an MFMA (a 16-column tile would hold 15/16 zeros),
// and at 9 FMAs per element against one read and one write the operation is
// memory-bound; the grouped kernels of conv_group.hip do not apply.
//
// Terms. A *granule* is 16 B of channels of one pixel: VEC = 8 bf16 or 4 f32
// channels. A *slab* is 8 granules = 128 B of channels (64 bf16 / 32 f32
// channels), so one LDS layout and one thread map serve both types. The last
// slab is masked per granule (C % 8 == 0, so a granule is whole or absent);
// nothing is read or written at or past channel C.
//
// fwd / dgrad (dwconv_kernel<T, R, ST, DG>): 256 threads = 8 granules x 16
// columns x 2 row groups; a block owns a TH x 16 tile of output pixels (dx
// pixels for dgrad) of one image x one slab, a thread one granule and one
// column of THG = TH/2 rows. The block stages the tile's halo patch of the
// source (x, or dout for dgrad) into LDS once with 16-B loads, zeros outside
// the image, and the slab's R*R weights as f32, tap-major. A thread keeps
// THG x VEC accumulators and walks the taps in ascending (r, s); the patch
// offsets are compile-time constants, so at R = 3 (fully unrolled, weights in
// registers) a patch granule that several output rows share is read once.
// At R = 5 / 7 the r loop is kept rolled with one weight row in registers:
// the full window would take 200 / 392 registers.
//   fwd:           patch (orow*ST + r, c*ST + s)
//   dgrad, ST 1:   patch (orow + R-1-r, c + R-1-s)
//   dgrad, ST 2:   e = orow + R-1-r + (pad & 1); patch row e >> 1, the tap
//                  counts when e is even (tile origins are even); same for
//                  columns. Taps of the wrong parity are predicated off.
// LDS pixel = 128 B, 8 granules; a b128 read is served 16 lanes at a time =
// 8 granules x 2 adjacent columns, which must fall into different 128-B
// halves of the 256-B bank line. Adjacent columns are adjacent patch pixels
// (or the same one) except for the stride-2 fwd, where they are two pixels
// apart: there pixel j is stored at slot swap(bit0, bit1)(j).
//
// wgrad (dwconv_wgrad_kernel<T, R, ST, TR> + dwconv_fold_kernel): a block
// owns (slab, tap rows r0..r0+TR-1, chunk z of the Nb * tiles pixel tiles),
// stages per tile the same x patch and the dout tile, and every thread adds
// x * dout of its pixels into TR*R*VEC accumulators. The block folds them
// over the 8 columns of a wave by xor-shuffles (8, 16, 32), then over waves
// 0..3 through LDS, and writes partial[z][R*R][C] f32 (always, also at
// split 1). The fold kernel adds z = 0, 1, ... and writes dw[C][R*R],
// rounded once. No atomics; every order is fixed.
//
// All element offsets are 64-bit. The launch functions do not allocate,
// sync or copy; they return nonzero without launching outside the envelope.
#include "common.h"

namespace {

constexpr int DW_TW = 16;     // tile columns
constexpr int DW_RG = 2;      // row groups of a block

template <typename T> struct Gran;
template <> struct Gran<unsigned short> {
    static constexpr int VEC = 8;
    static __device__ __forceinline__ void unpack(uint4 u, float* f) {
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = __uint_as_float(w[i] << 16);
            f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ uint4 pack(const float* f) {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = (unsigned)f32_to_bf16(f[2 * i]) |
                   ((unsigned)f32_to_bf16(f[2 * i + 1]) << 16);
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
    static __device__ __forceinline__ float ld(const unsigned short* p) {
        return bf16_to_f32(*p);
    }
    static __device__ __forceinline__ void st(unsigned short* p, float v) {
        *p = f32_to_bf16(v);
    }
};
template <> struct Gran<float> {
    static constexpr int VEC = 4;
    static __device__ __forceinline__ void unpack(uint4 u, float* f) {
        f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y);
        f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
    }
    static __device__ __forceinline__ uint4 pack(const float* f) {
        return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]),
                          __float_as_uint(f[2]), __float_as_uint(f[3]));
    }
    static __device__ __forceinline__ float ld(const float* p) { return *p; }
    static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
};

// tile geometry of one instantiation (wgrad uses the fwd geometry)
template <int R, int ST, bool DG>
struct DwTile {
    static constexpr int THG = (!DG && ST == 2) ? (R == 7 ? 1 : 2) : 4;
    static constexpr int TH = DW_RG * THG;
    static constexpr int PH = !DG ? (TH - 1) * ST + R
                              : (ST == 1 ? TH + R - 1 : (TH + R - 1) / 2 + 1);
    static constexpr int PW = !DG ? (DW_TW - 1) * ST + R
                              : (ST == 1 ? DW_TW + R - 1
                                         : (DW_TW + R - 1) / 2 + 1);
    static constexpr int SWAP = (!DG && ST == 2) ? 1 : 0;
    static constexpr int PWP = SWAP ? (PW + 3) / 4 * 4 : PW;   // row pitch
};

template <int SWAP>
__device__ __forceinline__ int dw_slot(int j) {
    return SWAP ? ((j & ~3) | ((j & 1) << 1) | ((j >> 1) & 1)) : j;
}

// PH x PW pixels x one slab of src[n][SH][SW][C] from (oh, ow) into LDS
template <typename T, int PH, int PW, int PWP, int SWAP>
__device__ __forceinline__ void dw_stage(
    uint4* lds, const T* __restrict__ src, long img, int SH, int SW, int C,
    int oh, int ow, int c0, int tid)
{
    constexpr int VEC = Gran<T>::VEC;
    for (int i = tid; i < PH * PW * 8; i += 256) {
        const int gr = i & 7, pix = i >> 3;
        const int pr = pix / PW, j = pix - pr * PW;
        const int row = oh + pr, col = ow + j, ch = c0 + gr * VEC;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if ((unsigned)row < (unsigned)SH && (unsigned)col < (unsigned)SW &&
            ch < C)
            v = *(const uint4*)&src[((img * SH + row) * SW + col) * C + ch];
        lds[(pr * PWP + dw_slot<SWAP>(j)) * 8 + gr] = v;
    }
}

struct DwArgs {
    const void* src;    // fwd: x [Nb,H,W,C]; dgrad: dout [Nb,P,Q,C]
    const void* w;      // [C][R*R]
    const void* bias;   // [C] or null (fwd only)
    void* dst;          // fwd: out [Nb,P,Q,C]; dgrad: dx [Nb,H,W,C]
    int SH, SW;         // source image
    int OH, OW;         // destination image
    int C, pad, tiles_h, tiles_w;
};

// ------------------------------------------------------------ fwd / dgrad
template <typename T, int R, int ST, bool DG>
__global__ __launch_bounds__(256) void dwconv_kernel(DwArgs p)
{
    using G = Gran<T>;
    using TL = DwTile<R, ST, DG>;
    constexpr int VEC = G::VEC, THG = TL::THG;
    constexpr int UNR = R == 3 ? 3 : 1;     // the r loop: see the header
    __shared__ uint4 patch[TL::PH * TL::PWP * 8];
    __shared__ __attribute__((aligned(16))) float wl[R * R * 8 * VEC];

    const int tid = threadIdx.x;
    const int gr = tid & 7, c = (tid >> 3) & (DW_TW - 1), g = tid >> 7;
    int b = blockIdx.x;
    const int tw = b % p.tiles_w;
    b /= p.tiles_w;
    const int th = b % p.tiles_h;
    const long img = b / p.tiles_h;
    const int c0 = blockIdx.y * (8 * VEC);
    const int h0 = th * TL::TH, w0 = tw * DW_TW;
    const int pb = p.pad & 1;

    int oh, ow;
    if (!DG) {
        oh = h0 * ST - p.pad;
        ow = w0 * ST - p.pad;
    } else if (ST == 1) {
        oh = h0 + p.pad - (R - 1);
        ow = w0 + p.pad - (R - 1);
    } else {
        oh = (h0 + p.pad - (R - 1)) >> 1;       // floor, also below zero
        ow = (w0 + p.pad - (R - 1)) >> 1;
    }
    dw_stage<T, TL::PH, TL::PW, TL::PWP, TL::SWAP>(
        patch, (const T*)p.src, img, p.SH, p.SW, p.C, oh, ow, c0, tid);
    for (int i = tid; i < R * R * 8 * VEC; i += 256) {
        const int cc = i / (R * R), tap = i - cc * (R * R);
        wl[tap * (8 * VEC) + cc] =
            c0 + cc < p.C ? G::ld((const T*)p.w + (long)(c0 + cc) * (R * R) + tap)
                          : 0.f;
    }
    __syncthreads();

    float acc[THG][VEC];
#pragma unroll
    for (int o = 0; o < THG; ++o)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[o][v] = 0.f;

#pragma unroll UNR
    for (int r = 0; r < R; ++r) {
        float wr[R][VEC];
#pragma unroll
        for (int s = 0; s < R; ++s)
#pragma unroll
            for (int v = 0; v < VEC; v += 4) {
                const float4 q =
                    *(const float4*)&wl[(r * R + s) * (8 * VEC) + gr * VEC + v];
                wr[s][v] = q.x; wr[s][v + 1] = q.y;
                wr[s][v + 2] = q.z; wr[s][v + 3] = q.w;
            }
#pragma unroll
        for (int o = 0; o < THG; ++o) {
            const int orow = g * THG + o;
            int prow;
            bool vr = true;
            if (!DG) {
                prow = orow * ST + r;
            } else if (ST == 1) {
                prow = orow + R - 1 - r;
            } else {
                const int e = orow + R - 1 - r + pb;
                prow = e >> 1;
                vr = !(e & 1);
            }
#pragma unroll
            for (int s = 0; s < R; ++s) {
                int pcol;
                bool ok = vr;
                if (!DG) {
                    pcol = c * ST + s;
                } else if (ST == 1) {
                    pcol = c + R - 1 - s;
                } else {
                    const int e = c + R - 1 - s + pb;
                    pcol = e >> 1;
                    ok = vr && !(e & 1);
                }
                float xv[VEC];
                G::unpack(patch[(prow * TL::PWP + dw_slot<TL::SWAP>(pcol)) * 8
                                + gr], xv);
                if (ok) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v)
                        acc[o][v] = fmaf(xv[v], wr[s][v], acc[o][v]);
                }
            }
        }
    }

    const int ch = c0 + gr * VEC, wcol = w0 + c;
    if (ch >= p.C || wcol >= p.OW) return;
    float bv[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        bv[v] = (!DG && p.bias) ? G::ld((const T*)p.bias + ch + v) : 0.f;
#pragma unroll
    for (int o = 0; o < THG; ++o) {
        const int hrow = h0 + g * THG + o;
        if (hrow >= p.OH) break;
        if (!DG && p.bias) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[o][v] += bv[v];
        }
        *(uint4*)&((T*)p.dst)[((img * p.OH + hrow) * p.OW + wcol) * p.C + ch] =
            G::pack(acc[o]);
    }
}

// ------------------------------------------------------------------ wgrad
template <typename T, int R, int ST, int TR>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(
    const T* __restrict__ dout, const T* __restrict__ x,
    float* __restrict__ partial, int H, int W, int C, int P, int Q, int pad,
    int tiles_h, int tiles_w, int units, int per)
{
    using G = Gran<T>;
    using TL = DwTile<R, ST, false>;
    constexpr int VEC = G::VEC, THG = TL::THG, NA = TR * R * VEC;
    __shared__ uint4 patch[TL::PH * TL::PWP * 8];
    __shared__ uint4 dyt[TL::TH * DW_TW * 8];
    __shared__ float red[4][8][NA];

    const int tid = threadIdx.x;
    const int gr = tid & 7, c = (tid >> 3) & (DW_TW - 1), g = tid >> 7;
    const int c0 = blockIdx.x * (8 * VEC);
    const int r0 = blockIdx.y * TR, z = blockIdx.z;

    float acc[TR][R][VEC];
#pragma unroll
    for (int rr = 0; rr < TR; ++rr)
#pragma unroll
        for (int s = 0; s < R; ++s)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[rr][s][v] = 0.f;

    const int u1 = min(units, (z + 1) * per);
    for (int u = z * per; u < u1; ++u) {
        int b = u;
        const int tw = b % tiles_w;
        b /= tiles_w;
        const int th = b % tiles_h;
        const long img = b / tiles_h;
        const int p0 = th * TL::TH, q0 = tw * DW_TW;
        __syncthreads();                  // the previous tile is consumed
        dw_stage<T, TL::PH, TL::PW, TL::PWP, TL::SWAP>(
            patch, x, img, H, W, C, p0 * ST - pad, q0 * ST - pad, c0, tid);
        dw_stage<T, TL::TH, DW_TW, DW_TW, 0>(dyt, dout, img, P, Q, C, p0, q0,
                                             c0, tid);
        __syncthreads();
#pragma unroll
        for (int o = 0; o < THG; ++o) {
            const int orow = g * THG + o;
            float dv[VEC];
            G::unpack(dyt[(orow * DW_TW + c) * 8 + gr], dv);
#pragma unroll
            for (int rr = 0; rr < TR; ++rr)
#pragma unroll
                for (int s = 0; s < R; ++s) {
                    float xv[VEC];
                    G::unpack(patch[((orow * ST + r0 + rr) * TL::PWP +
                                     dw_slot<TL::SWAP>(c * ST + s)) * 8 + gr],
                              xv);
#pragma unroll
                    for (int v = 0; v < VEC; ++v)
                        acc[rr][s][v] = fmaf(xv[v], dv[v], acc[rr][s][v]);
                }
        }
    }

    // lanes gr, gr+8, ..., gr+56 of a wave hold the same channels
    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int rr = 0; rr < TR; ++rr)
#pragma unroll
        for (int s = 0; s < R; ++s)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float a = acc[rr][s][v];
                a += __shfl_xor(a, 8);
                a += __shfl_xor(a, 16);
                a += __shfl_xor(a, 32);
                if (lane < 8) red[wid][gr][(rr * R + s) * VEC + v] = a;
            }
    __syncthreads();
    for (int i = tid; i < TR * R * 8 * VEC; i += 256) {
        const int tapl = i / (8 * VEC), cc = i - tapl * (8 * VEC);
        const int k = tapl * VEC + cc % VEC;
        float a = red[0][cc / VEC][k];
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) a += red[wv][cc / VEC][k];
        if (c0 + cc < C)
            partial[((long)z * (R * R) + r0 * R + tapl) * C + c0 + cc] = a;
    }
}

// dw[c][tap] = sum over chunks in chunk order of partial[z][tap][c]
template <typename T>
__global__ __launch_bounds__(256) void dwconv_fold_kernel(
    T* __restrict__ dw, const float* __restrict__ partial, int C, int RR,
    int split)
{
    const long n = (long)C * RR;
    EW_IDX
    for (long i = gid; i < n; i += stride) {
        const int tap = (int)(i % RR);
        const long idx = (long)tap * C + i / RR;
        float a = partial[idx];
        for (int zz = 1; zz < split; ++zz) a += partial[zz * n + idx];
        Gran<T>::st(&dw[i], a);
    }
}

inline bool dal16(const void* q) { return q && ((uintptr_t)q & 15) == 0; }

// the envelope
bool dw_ok(int Nb, int H, int W, int C, int P, int Q, int R, int stride,
           int pad, int dtype)
{
    if (dtype != PS_F32 && dtype != PS_BF16) return false;
    if (Nb <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return false;
    if (R != 3 && R != 5 && R != 7) return false;
    if ((stride != 1 && stride != 2) || pad < 0 || pad >= R) return false;
    if (H + 2 * pad < R || W + 2 * pad < R) return false;
    if (P != (H + 2 * pad - R) / stride + 1) return false;
    if (Q != (W + 2 * pad - R) / stride + 1) return false;
    if (C / 32 + 1 > 65535) return false;
    // one block per tile of the larger image: the grid's x extent
    return (long)Nb * ((H + 1) / 2) * ((W + DW_TW - 1) / DW_TW) < (1L << 31);
}

template <typename T, int R, int ST, bool DG>
void launch_dw(const DwArgs& a, int Nb, hipStream_t s)
{
    DwArgs p = a;
    p.tiles_h = (p.OH + DwTile<R, ST, DG>::TH - 1) / DwTile<R, ST, DG>::TH;
    p.tiles_w = (p.OW + DW_TW - 1) / DW_TW;
    const int slab = 8 * Gran<T>::VEC;
    dim3 grid((unsigned)((long)Nb * p.tiles_h * p.tiles_w),
              (unsigned)((p.C + slab - 1) / slab));
    hipLaunchKernelGGL((dwconv_kernel<T, R, ST, DG>), grid, dim3(256), 0, s, p);
}

template <typename T, bool DG>
void dispatch_dw(const DwArgs& a, int Nb, int R, int stride, hipStream_t s)
{
#define DW_CASE(RV, SV) \
    if (R == RV && stride == SV) return launch_dw<T, RV, SV, DG>(a, Nb, s);
    DW_CASE(3, 1) DW_CASE(3, 2) DW_CASE(5, 1) DW_CASE(5, 2)
    DW_CASE(7, 1) DW_CASE(7, 2)
#undef DW_CASE
}

template <typename T, int R, int ST>
void launch_dw_wgrad(const void* dout, const void* x, void* partial, void* dw,
                     int Nb, int H, int W, int C, int P, int Q, int pad,
                     int split, hipStream_t s)
{
    constexpr int TR = R == 3 ? 3 : 1;
    using TL = DwTile<R, ST, false>;
    const int tiles_h = (P + TL::TH - 1) / TL::TH;
    const int tiles_w = (Q + DW_TW - 1) / DW_TW;
    const int units = Nb * tiles_h * tiles_w;
    const int per = (units + split - 1) / split;
    const int slab = 8 * Gran<T>::VEC;
    dim3 grid((unsigned)((C + slab - 1) / slab), (unsigned)(R / TR),
              (unsigned)split);
    hipLaunchKernelGGL((dwconv_wgrad_kernel<T, R, ST, TR>), grid, dim3(256), 0,
                       s, (const T*)dout, (const T*)x, (float*)partial, H, W,
                       C, P, Q, pad, tiles_h, tiles_w, units, per);
    int blocks;
    ew_grid((long)C * R * R, 256, &blocks);
    hipLaunchKernelGGL(dwconv_fold_kernel<T>, dim3(blocks), dim3(256), 0, s,
                       (T*)dw, (const float*)partial, C, R * R, split);
}

template <typename T>
void dispatch_dw_wgrad(const void* dout, const void* x, void* partial,
                       void* dw, int Nb, int H, int W, int C, int P, int Q,
                       int R, int stride, int pad, int split, hipStream_t s)
{
#define DW_CASE(RV, SV) \
    if (R == RV && stride == SV) \
        return launch_dw_wgrad<T, RV, SV>(dout, x, partial, dw, Nb, H, W, C, \
                                          P, Q, pad, split, s);
    DW_CASE(3, 1) DW_CASE(3, 2) DW_CASE(5, 1) DW_CASE(5, 2)
    DW_CASE(7, 1) DW_CASE(7, 2)
#undef DW_CASE
}

}  // namespace

// w: [C][R*R], the channels_last memory of the [C, 1, R, R] parameter
extern "C" int ps_dwconv_fwd(
    const void* x, const void* w, const void* bias, void* out,
    int Nb, int H, int W, int C, int P, int Q, int R, int stride, int pad,
    int dtype, void* strm)
{
    if (!dw_ok(Nb, H, W, C, P, Q, R, stride, pad, dtype) || !dal16(x) || !w ||
        !dal16(out))
        return 1;
    DwArgs a;
    a.src = x; a.w = w; a.bias = bias; a.dst = out;
    a.SH = H; a.SW = W; a.OH = P; a.OW = Q; a.C = C; a.pad = pad;
    a.tiles_h = a.tiles_w = 0;
    if (dtype == PS_BF16)
        dispatch_dw<unsigned short, false>(a, Nb, R, stride, (hipStream_t)strm);
    else
        dispatch_dw<float, false>(a, Nb, R, stride, (hipStream_t)strm);
    return 0;
}

extern "C" int ps_dwconv_dgrad(
    const void* dout, const void* w, void* dx,
    int Nb, int H, int W, int C, int P, int Q, int R, int stride, int pad,
    int dtype, void* strm)
{
    if (!dw_ok(Nb, H, W, C, P, Q, R, stride, pad, dtype) || !dal16(dout) ||
        !w || !dal16(dx))
        return 1;
    DwArgs a;
    a.src = dout; a.w = w; a.bias = nullptr; a.dst = dx;
    a.SH = P; a.SW = Q; a.OH = H; a.OW = W; a.C = C; a.pad = pad;
    a.tiles_h = a.tiles_w = 0;
    if (dtype == PS_BF16)
        dispatch_dw<unsigned short, true>(a, Nb, R, stride, (hipStream_t)strm);
    else
        dispatch_dw<float, true>(a, Nb, R, stride, (hipStream_t)strm);
    return 0;
}

// partial: split * R*R * C floats; dw: [C][R*R] in the storage type
extern "C" int ps_dwconv_wgrad(
    const void* dout, const void* x, void* partial, void* dw,
    int Nb, int H, int W, int C, int P, int Q, int R, int stride, int pad,
    int split, int dtype, void* strm)
{
    if (!dw_ok(Nb, H, W, C, P, Q, R, stride, pad, dtype) || split < 1 ||
        split > 256 || !dal16(dout) || !dal16(x) || !partial || !dw)
        return 1;
    hipStream_t s = (hipStream_t)strm;
    if (dtype == PS_BF16)
        dispatch_dw_wgrad<unsigned short>(dout, x, partial, dw, Nb, H, W, C,
                                          P, Q, R, stride, pad, split, s);
    else
        dispatch_dw_wgrad<float>(dout, x, partial, dw, Nb, H, W, C, P, Q, R,
                                 stride, pad, split, s);
    return 0;
}
