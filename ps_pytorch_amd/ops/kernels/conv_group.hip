// Grouped NHWC convolution (groups = G > 1, C == K), bf16 in / f32
// accumulate / bf16 out, on mfma_f32_16x16x32_bf16. The dense kernels of
// conv.hip cannot serve it: with Cg = C/G in {4..64} channels per group one
// 16x16x32 MFMA spans several groups and a tap's contraction (Cg) is shorter
// than one k-step, so the operands are packed differently here.
//
// Terms. A *slab* is 64 consecutive channels; it holds 64/Cg whole groups,
// so output slab s depends on input slab s only and a block never looks at
// another slab. A *super-group* is SG = max(Cg, 16) channels, the narrowest
// width one MFMA column tile serves: the weight inside a super-group is
// dense for Cg >= 16 and block-diagonal (Cg x Cg blocks) for Cg < 16.
//
// Weight image (gconv_expand_kernel, every forward and backward): from
// w[K][R][S][Cg] build, per (slab, tap), 64 rows x SG bf16: row = output
// column (channel within the slab), SG contraction values contiguous, zeros
// off the group diagonal. fwd: row = ko, k = ci; dgrad: row = ci, k = ko
// (the per-tap transpose). A B fragment is then one ds_read_b128 per lane:
// SG 64 rows carry the gswz swizzle in LDS, SG 32 / 16 images are stored in
// fragment order so that the 64 lanes of a read are contiguous.
//
// fwd / dgrad (gconv_kernel<SG, DGRAD>): 256 threads, block = 128 rows
// (output pixels; dx pixels for dgrad) x one slab, grid ceil(M/128) x C/64,
// 32 accumulator tiles split over the waves as in conv_gemm_kernel (wave =
// 64 rows x 32 cols = 4 x 2 tiles). Per step a tap's A tile (128 pixels x
// the slab's 64 channels, one 16-B gather per granule at pixel pitch C,
// zero outside the image) and its B image go to LDS; the A tile carries
// the gswz mode-2 granule swizzle of conv.hip. Contraction per SG:
//   64: two 32-channel k-steps per tap, the four column tiles share A
//   32: one k-step per tap; column tiles 0-1 contract channels 0-31,
//       tiles 2-3 channels 32-63
//   16: one k-step covers TWO taps: column tile j contracts
//       [tap t, ch 16j..16j+15 | tap t+1, same channels]; with an odd tap
//       count the phantom half multiplies a zero B image against a ZERO A
//       tile (never live data: Inf x 0 must not appear)
// SG 64/32 double-buffer the LDS tiles (one barrier per step). SG 16 stages
// two 16-KiB tap tiles per step; double-buffering them would take 72 KiB,
// over the 64-KiB block budget, so it keeps ONE LDS stage and prefetches
// the next step into registers under the MFMAs (two barriers per step).
// dgrad gathers dout at ((h + pad - r)/stride, (w + pad - s)/stride),
// predicated on divisibility and range; dx pixels no tap reaches are 0.
// The epilogue stages f32 through LDS and writes 16-B bf16 segments; fwd
// adds the bias in f32; each output is rounded once.
//
// wgrad (gconv_wgrad_kernel<SG>): block = (slab, tap, split chunk z),
// contraction over the chunk's pixels, 32 per MFMA step. The dout tile and
// the tap-shifted x tile (32 px x 64 ch each) are stored [pixel][channel]
// in 16-channel subtiles and read through ds_read_b64_tr_b16 with conv.hip's
// pswz row permutation. Only the diagonal super-group tiles are computed
// (SG/16 per wave). f32 partials partial[split][C/64][R*S][64/SG][SG][SG];
// the fold kernel adds the chunks in order and writes the Cg x Cg group
// blocks into dw[K][R][S][Cg], rounded once. No atomics.
//
// All element offsets are 64-bit. The launch functions do not allocate,
// sync or copy; they return nonzero without launching outside the envelope.
#include "common.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

#define GMFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)

union G16 {
    uint4 u4;
    unsigned short us[8];
};

__device__ __forceinline__ uint4 zero4() { return make_uint4(0u, 0u, 0u, 0u); }

// conv.hip's mode-2 granule swizzle: position of granule g in row's 128 B
__device__ __forceinline__ int gswz2(int row, int g) {
    return g ^ (((row >> 1) & 3) << 1);
}

// conv.hip's pixel-row permutation for the transpose-read subtiles
__device__ __forceinline__ int gpswz(int r) {
    return r ^ (((r >> 3) & 1) << 2);
}

__device__ __forceinline__ bf16x4_t g_tr16(const unsigned short* p) {
    typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 v4;
    auto lp = (__attribute__((address_space(3))) v4*)(p);
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(lp);
}

// ------------------------------------------------------- weight expansion
// img[slab][tap][row 0..63][k 0..SG-1] (granule order within a tap: see the
// store); one thread per 8 k (16-B store).
// tr == 0 (fwd): row = ko, k = ci. tr == 1 (dgrad): row = ci, k = ko.
__global__ __launch_bounds__(256) void gconv_expand_kernel(
    unsigned short* __restrict__ img, const unsigned short* __restrict__ w,
    int C, int RS, int Cg, int SG, int tr)
{
    const int kgs = SG >> 3;                       // granules per row
    const long n = (long)C * RS * kgs;
    EW_IDX
    for (long i = gid; i < n; i += stride) {
        const int kg = (int)(i % kgs);
        long q = i / kgs;
        const int row = (int)(q & 63);
        q >>= 6;
        const int tap = (int)(q % RS);
        const int slab = (int)(q / RS);
        const int crow = slab * 64 + row;
        const int sgbase = slab * 64 + (row / SG) * SG;
        G16 o;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int ck = sgbase + kg * 8 + u;
            unsigned short v = 0;
            if (crow / Cg == ck / Cg) {
                const int ko = tr ? ck : crow, ci = tr ? crow : ck;
                v = w[((long)ko * RS + tap) * Cg + ci % Cg];
            }
            o.us[u] = v;
        }
        // SG 64: row-major (the kernel swizzles granules on its LDS write).
        // SG < 64: fragment order [16-row tile][k granule][row in tile], so
        // the linear LDS copy leaves lane (fr, fq) of a B read at 16 B x
        // its lane index: contiguous, conflict-free ds_read_b128.
        long d = i;
        if (SG < 64)
            d = (q * 64 + (row >> 4) * 16) * kgs + kg * 16 + (row & 15);
        *(uint4*)&img[d * 8] = o.u4;
    }
}

// ------------------------------------------------------------ fwd / dgrad
struct GconvArgs {
    const unsigned short* src;   // fwd: x [Nb,H,W,C]; dgrad: dout [Nb,P,Q,C]
    const unsigned short* img;   // expanded weights (see above)
    const unsigned short* bias;  // [C] or null (fwd only)
    unsigned short* dst;         // fwd: out [Nb,P,Q,C]; dgrad: dx [Nb,H,W,C]
    int Nb, H, W, C, P, Q, R, st, pd;
};

template <int SG, bool DGRAD>
__global__ __launch_bounds__(256) void gconv_kernel(GconvArgs p)
{
    constexpr int NT = SG == 16 ? 2 : 1;        // tap tiles per step
    constexpr int NBUF = SG == 16 ? 1 : 2;      // LDS stages
    constexpr int BEL = 64 * SG;                // B image elements per tap
    constexpr int BGT = BEL / 8;                // B granules per tap
    constexpr int BG = BGT * NT / 256;          // B granules per thread
    __shared__ __attribute__((aligned(16)))
        unsigned short ldsA[NBUF][NT][128][64];
    __shared__ __attribute__((aligned(16))) unsigned short ldsB[NBUF][NT][BEL];
    static_assert(sizeof(ldsA) >= 128 * 64 * 4, "f32 staging fits ldsA");

    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int trow = t >> 3, g = t & 7;
    const int C = p.C, R = p.R, RS = p.R * p.R;
    const long M = DGRAD ? (long)p.Nb * p.H * p.W : (long)p.Nb * p.P * p.Q;
    const long m0 = (long)blockIdx.x * 128;
    const int slab = blockIdx.y;
    const int sH = DGRAD ? p.P : p.H, sW = DGRAD ? p.Q : p.W;   // source dims
    const unsigned short* srcc = p.src + slab * 64 + g * 8;
    const unsigned short* imgs = p.img + (long)slab * RS * BEL;

    // this thread's four A rows, decoded once
    int rn[4], ry[4], rx[4];
    bool rv[4];
    {
        const int plane = DGRAD ? p.H * p.W : p.P * p.Q;
        const int width = DGRAD ? p.W : p.Q;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const long m = m0 + trow + 32 * rr;
            rv[rr] = m < M;
            const long mm = rv[rr] ? m : 0;
            rn[rr] = (int)(mm / plane);
            const int rem = (int)(mm - (long)rn[rr] * plane);
            const int yy = rem / width, xx = rem - yy * width;
            if (DGRAD) { ry[rr] = yy + p.pd; rx[rr] = xx + p.pd; }
            else { ry[rr] = yy * p.st - p.pd; rx[rr] = xx * p.st - p.pd; }
        }
    }

    f32x4_t acc[4][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj) acc[mi][nj] = {0.f, 0.f, 0.f, 0.f};

    uint4 areg[NT][4], breg[BG];
    auto load_step = [&](int step) {
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            const int tap = step * NT + tt;
            const int r = tap / R, s = tap - r * R;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                int h, w;
                bool ok = rv[rr] && tap < RS;     // phantom tap: zero A
                if (DGRAD) {
                    h = ry[rr] - r; w = rx[rr] - s;
                    ok = ok && h >= 0 && w >= 0;
                    if (p.st == 2) {
                        ok = ok && !(h & 1) && !(w & 1);
                        h >>= 1; w >>= 1;
                    }
                    ok = ok && h < sH && w < sW;
                } else {
                    h = ry[rr] + r; w = rx[rr] + s;
                    ok = ok && (unsigned)h < (unsigned)sH &&
                         (unsigned)w < (unsigned)sW;
                }
                areg[tt][rr] = zero4();
                if (ok)
                    areg[tt][rr] = *(const uint4*)
                        (srcc + (((long)rn[rr] * sH + h) * sW + w) * C);
            }
        }
#pragma unroll
        for (int bi = 0; bi < BG; ++bi) {
            const int gi = t + 256 * bi;
            const int tap = step * NT + gi / BGT;
            breg[bi] = zero4();                   // phantom tap: zero B
            if (tap < RS)
                breg[bi] = *(const uint4*)
                    (imgs + (long)tap * BEL + (gi % BGT) * 8);
        }
    };

    auto write_lds = [&](int buf) {
#pragma unroll
        for (int tt = 0; tt < NT; ++tt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int row = trow + 32 * rr;
                *(uint4*)&ldsA[buf][tt][row][gswz2(row, g) * 8] = areg[tt][rr];
            }
#pragma unroll
        for (int bi = 0; bi < BG; ++bi) {
            const int gi = t + 256 * bi;
            const int tt = gi / BGT, wi = gi % BGT;
            int pos = wi * 8;
            if (SG == 64) pos = (wi >> 3) * 64 + gswz2(wi >> 3, wi & 7) * 8;
            *(uint4*)&ldsB[buf][tt][pos] = breg[bi];
        }
    };

    auto mfma_step = [&](int buf) {
        if constexpr (SG == 64) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8_t a[4], b[2];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    const int row = wm * 64 + mi * 16 + fr;
                    a[mi] = *(const bf16x8_t*)
                        &ldsA[buf][0][row][gswz2(row, kk * 4 + fq) * 8];
                }
#pragma unroll
                for (int nj = 0; nj < 2; ++nj) {
                    const int br = (wn * 2 + nj) * 16 + fr;
                    b[nj] = *(const bf16x8_t*)
                        &ldsB[buf][0][br * 64 + gswz2(br, kk * 4 + fq) * 8];
                }
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int nj = 0; nj < 2; ++nj)
                        acc[mi][nj] = GMFMA(a[mi], b[nj], acc[mi][nj]);
            }
        } else if constexpr (SG == 32) {
            // both column tiles of this wave sit in super-group wn
            bf16x8_t a[4], b[2];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int row = wm * 64 + mi * 16 + fr;
                a[mi] = *(const bf16x8_t*)
                    &ldsA[buf][0][row][gswz2(row, wn * 4 + fq) * 8];
            }
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                b[nj] = *(const bf16x8_t*)
                    &ldsB[buf][0][(wn * 2 + nj) * 512 + lane * 8];
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int nj = 0; nj < 2; ++nj)
                    acc[mi][nj] = GMFMA(a[mi], b[nj], acc[mi][nj]);
        } else {
            // k = [tap 2i: 16 channels | tap 2i+1: the same 16 channels]
            const int tt = fq >> 1, kg = fq & 1;
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                const int jt = wn * 2 + nj;
                const bf16x8_t b = *(const bf16x8_t*)
                    &ldsB[buf][tt][jt * 256 + (lane & 31) * 8];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    const int row = wm * 64 + mi * 16 + fr;
                    const bf16x8_t a = *(const bf16x8_t*)
                        &ldsA[buf][tt][row][gswz2(row, jt * 2 + kg) * 8];
                    acc[mi][nj] = GMFMA(a, b, acc[mi][nj]);
                }
            }
        }
    };

    const int nsteps = (RS + NT - 1) / NT;
    load_step(0);
    write_lds(0);
    if (nsteps > 1) load_step(1);
    __syncthreads();
    for (int it = 0; it < nsteps; ++it) {
        if constexpr (NBUF == 2) {
            if (it + 1 < nsteps) {
                write_lds((it + 1) & 1);
                if (it + 2 < nsteps) load_step(it + 2);
            }
            mfma_step(it & 1);
            __syncthreads();
        } else {
            mfma_step(0);
            __syncthreads();          // the stage's reads are done
            if (it + 1 < nsteps) {
                write_lds(0);
                if (it + 2 < nsteps) load_step(it + 2);
                __syncthreads();
            }
        }
    }

    // ---- epilogue: f32 through LDS, 16-B bf16 row segments ----
    float* sf = reinterpret_cast<float*>(&ldsA[0][0][0][0]);
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
        const int cl = (wn * 2 + nj) * 16 + fr;
        const float bv = (!DGRAD && p.bias)
                         ? bf16_to_f32(p.bias[slab * 64 + cl]) : 0.f;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                sf[(wm * 64 + mi * 16 + fq * 4 + e) * 64 + cl] =
                    acc[mi][nj][e] + bv;
    }
    __syncthreads();
    const int segc = (t & 7) * 8, rl0 = t >> 3;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
        const int rl = ps * 32 + rl0;
        const long om = m0 + rl;
        if (om >= M) continue;
        const f32x4_t v0 = *(const f32x4_t*)&sf[rl * 64 + segc];
        const f32x4_t v1 = *(const f32x4_t*)&sf[rl * 64 + segc + 4];
        G16 o;
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) {
            o.us[k2] = f32_to_bf16(v0[k2]);
            o.us[4 + k2] = f32_to_bf16(v1[k2]);
        }
        *(uint4*)&p.dst[om * C + slab * 64 + segc] = o.u4;
    }
}

// ------------------------------------------------------------------ wgrad
#define GW_SUB (32 * 16 + 16)          // [32 px][16 ch] + pad (elements)

template <int SG>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(
    const unsigned short* __restrict__ dout,   // [Nb,P,Q,C]
    const unsigned short* __restrict__ x,      // [Nb,H,W,C]
    float* __restrict__ partial,   // [split][C/64][R*S][64/SG][SG][SG]
    int Nb, int H, int W, int C, int P, int Q, int R, int st, int pd,
    long chunk)
{
    constexpr int NTW = SG / 16;               // tiles per wave
    __shared__ __attribute__((aligned(16))) unsigned short ldsD[2][4][GW_SUB];
    __shared__ __attribute__((aligned(16))) unsigned short ldsX[2][4][GW_SUB];

    const int slab = blockIdx.x, tap = blockIdx.y, z = blockIdx.z;
    const int r = tap / R, s = tap - r * R, RS = R * R;
    const long M = (long)Nb * P * Q;
    const long mbeg = (long)z * chunk;
    const long mend = mbeg + chunk < M ? mbeg + chunk : M;
    const int nsteps = mend > mbeg ? (int)((mend - mbeg + 31) >> 5) : 0;

    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int px = t >> 3, g = t & 7;
    const int plane = P * Q;
    const int wpos = gpswz(px) * 16 + (g & 1) * 8;   // in subtile g >> 1

    f32x4_t acc[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};

    uint4 dreg, xreg;
    auto load_step = [&](int it) {
        const long m = mbeg + (long)it * 32 + px;
        dreg = zero4();
        xreg = zero4();
        if (m < mend) {
            const int n = (int)(m / plane);
            const int rem = (int)(m - (long)n * plane);
            const int pp = rem / Q, qq = rem - pp * Q;
            dreg = *(const uint4*)(dout + m * C + slab * 64 + g * 8);
            const int h = pp * st - pd + r, w = qq * st - pd + s;
            if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W)
                xreg = *(const uint4*)
                    (x + (((long)n * H + h) * W + w) * C + slab * 64 + g * 8);
        }
    };
    auto write_lds = [&](int buf) {
        *(uint4*)&ldsD[buf][g >> 1][wpos] = dreg;
        *(uint4*)&ldsX[buf][g >> 1][wpos] = xreg;
    };
    // lane fr reads 4 bf16 of pixel row fq*8 + i*4 + (fr >> 2), quad fr & 3,
    // and receives its channel's 4 pixel values (hardware transpose)
    int ro[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
        ro[i] = gpswz(fq * 8 + i * 4 + (fr >> 2)) * 16 + (fr & 3) * 4;
    union U8 { bf16x4_t h[2]; bf16x8_t v; };
    auto mfma_step = [&](int buf) {
        U8 a;
        a.h[0] = g_tr16(&ldsD[buf][wid][ro[0]]);
        a.h[1] = g_tr16(&ldsD[buf][wid][ro[1]]);
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            const int sub = (wid / NTW) * NTW + j;
            U8 b;
            b.h[0] = g_tr16(&ldsX[buf][sub][ro[0]]);
            b.h[1] = g_tr16(&ldsX[buf][sub][ro[1]]);
            acc[j] = GMFMA(a.v, b.v, acc[j]);
        }
    };

    if (nsteps > 0) {
        load_step(0);
        write_lds(0);
        if (nsteps > 1) load_step(1);
    }
    __syncthreads();
    for (int it = 0; it < nsteps; ++it) {
        if (it + 1 < nsteps) {
            write_lds((it + 1) & 1);
            if (it + 2 < nsteps) load_step(it + 2);
        }
        mfma_step(it & 1);
        __syncthreads();
    }

    // D[ko = 4*fq + e][ci = fr] of (super-group wid / NTW)
    float* dstp = partial +
        (((long)z * (C >> 6) + slab) * RS + tap) * (64 * SG) +
        (wid / NTW) * (SG * SG);
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            dstp[((wid % NTW) * 16 + fq * 4 + e) * SG + j * 16 + fr] = acc[j][e];
}

// dw[ko][tap][cl] = sum over chunks in chunk order of the group-diagonal
// element of the partial image; rounded once
__global__ __launch_bounds__(256) void gconv_wgrad_fold_kernel(
    unsigned short* __restrict__ dw, const float* __restrict__ partial,
    int C, int RS, int Cg, int SG, int split)
{
    const long n = (long)C * RS * Cg;
    const long per = (long)C * RS * SG;
    EW_IDX
    for (long i = gid; i < n; i += stride) {
        const int cl = (int)(i % Cg);
        const long q = i / Cg;
        const int tap = (int)(q % RS);
        const int ko = (int)(q / RS);
        const int slab = ko >> 6, kr = ko & 63;
        const int ci = (ko / Cg) * Cg + cl;
        const long idx = ((long)slab * RS + tap) * (64 * SG) +
                         (kr / SG) * (SG * SG) + (kr % SG) * SG +
                         (ci & 63) % SG;
        float a = partial[idx];
        for (int zz = 1; zz < split; ++zz) a += partial[zz * per + idx];
        dw[i] = f32_to_bf16(a);
    }
}

inline bool gal16(const void* q) { return q && ((uintptr_t)q & 15) == 0; }

// the envelope; returns SG, or 0 when the arguments fall outside it
int gconv_sg(int Nb, int H, int W, int C, int G, int P, int Q, int R,
             int stride, int pad)
{
    if (Nb <= 0 || H <= 0 || W <= 0 || C <= 0 || G <= 1) return 0;
    if (C % 64 || C % G || C / 64 > 65535) return 0;
    const int Cg = C / G;
    if (Cg != 4 && Cg != 8 && Cg != 16 && Cg != 32 && Cg != 64) return 0;
    if (R < 1 || R > 7 || (stride != 1 && stride != 2) || pad < 0) return 0;
    if (H + 2 * pad < R || W + 2 * pad < R) return 0;
    if (P != (H + 2 * pad - R) / stride + 1) return 0;
    if (Q != (W + 2 * pad - R) / stride + 1) return 0;
    if ((long)Nb * H * W >= (1L << 31) * 128) return 0;
    return Cg < 16 ? 16 : Cg;
}

void launch_expand(void* img, const void* w, int C, int RS, int Cg, int SG,
                   int tr, hipStream_t strm)
{
    int blocks;
    ew_grid((long)C * RS * (SG / 8), 256, &blocks);
    hipLaunchKernelGGL(gconv_expand_kernel, dim3(blocks), dim3(256), 0, strm,
                       (unsigned short*)img, (const unsigned short*)w, C, RS,
                       Cg, SG, tr);
}

template <bool DGRAD>
int launch_gconv(const void* src, const void* w, const void* bias, void* dst,
                 void* wimg, int Nb, int H, int W, int C, int G, int P, int Q,
                 int R, int stride, int pad, void* strm)
{
    const int SG = gconv_sg(Nb, H, W, C, G, P, Q, R, stride, pad);
    if (!SG || !gal16(src) || !w || !gal16(dst) || !gal16(wimg))
        return 1;
    hipStream_t s = (hipStream_t)strm;
    launch_expand(wimg, w, C, R * R, C / G, SG, DGRAD ? 1 : 0, s);
    GconvArgs p;
    p.src = (const unsigned short*)src;
    p.img = (const unsigned short*)wimg;
    p.bias = DGRAD ? nullptr : (const unsigned short*)bias;
    p.dst = (unsigned short*)dst;
    p.Nb = Nb; p.H = H; p.W = W; p.C = C; p.P = P; p.Q = Q; p.R = R;
    p.st = stride; p.pd = pad;
    const long M = DGRAD ? (long)Nb * H * W : (long)Nb * P * Q;
    dim3 grid((unsigned)((M + 127) / 128), (unsigned)(C / 64));
    if (SG == 64)
        hipLaunchKernelGGL((gconv_kernel<64, DGRAD>), grid, dim3(256), 0, s, p);
    else if (SG == 32)
        hipLaunchKernelGGL((gconv_kernel<32, DGRAD>), grid, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((gconv_kernel<16, DGRAD>), grid, dim3(256), 0, s, p);
    return 0;
}

}  // namespace

// wimg: C * R*R * SG bf16 of workspace (SG = max(C/G, 16)), 16-B aligned
extern "C" int ps_gconv_fwd(
    const void* x, const void* w, const void* bias, void* out, void* wimg,
    int Nb, int H, int W, int C, int G, int P, int Q, int R, int stride,
    int pad, void* strm)
{
    return launch_gconv<false>(x, w, bias, out, wimg, Nb, H, W, C, G, P, Q, R,
                               stride, pad, strm);
}

extern "C" int ps_gconv_dgrad(
    const void* dout, const void* w, void* dx, void* wimg,
    int Nb, int H, int W, int C, int G, int P, int Q, int R, int stride,
    int pad, void* strm)
{
    return launch_gconv<true>(dout, w, nullptr, dx, wimg, Nb, H, W, C, G, P,
                              Q, R, stride, pad, strm);
}

// partial: split * C * R*R * SG floats
extern "C" int ps_gconv_wgrad(
    const void* dout, const void* x, void* partial, void* dw,
    int Nb, int H, int W, int C, int G, int P, int Q, int R, int stride,
    int pad, int split, void* strm)
{
    const int SG = gconv_sg(Nb, H, W, C, G, P, Q, R, stride, pad);
    if (!SG || split < 1 || split > 256 || !gal16(dout) || !gal16(x) ||
        !gal16(partial) || !dw)
        return 1;
    hipStream_t s = (hipStream_t)strm;
    const long M = (long)Nb * P * Q;
    const long chunk = ((M + split - 1) / split + 31) / 32 * 32;
    dim3 grid((unsigned)(C / 64), (unsigned)(R * R), (unsigned)split);
    float* part = (float*)partial;
    const unsigned short* d = (const unsigned short*)dout;
    const unsigned short* xi = (const unsigned short*)x;
    if (SG == 64)
        hipLaunchKernelGGL(gconv_wgrad_kernel<64>, grid, dim3(256), 0, s, d,
                           xi, part, Nb, H, W, C, P, Q, R, stride, pad, chunk);
    else if (SG == 32)
        hipLaunchKernelGGL(gconv_wgrad_kernel<32>, grid, dim3(256), 0, s, d,
                           xi, part, Nb, H, W, C, P, Q, R, stride, pad, chunk);
    else
        hipLaunchKernelGGL(gconv_wgrad_kernel<16>, grid, dim3(256), 0, s, d,
                           xi, part, Nb, H, W, C, P, Q, R, stride, pad, chunk);
    int blocks;
    ew_grid((long)C * R * R * (C / G), 256, &blocks);
    hipLaunchKernelGGL(gconv_wgrad_fold_kernel, dim3(blocks), dim3(256), 0, s,
                       (unsigned short*)dw, (const float*)part, C, R * R,
                       C / G, SG, split);
    return 0;
}
