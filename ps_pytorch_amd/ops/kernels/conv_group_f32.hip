// Grouped NHWC convolution (groups = G > 1, C == K), f32 in / f32 accumulate
// / f32 out: the --compute-dtype fp32 twin of conv_group.hip, on the two
// exact-f32 MFMA forms of gfx950. Same envelope as the bf16 family: C % 64
// == 0, Cg = C/G in {4, 8, 16, 32, 64}, square R <= 7, stride 1 or 2, square
// padding, optional bias. The weight is used in place as w[K][R][R][Cg] (the
// channels_last memory of the parameter) and dw is written in that layout;
// there is no expanded weight image, because nothing here needs zeros off
// the group diagonal.
//
// A *slab* is 64 consecutive channels = 64/Cg whole groups; output slab s
// depends on input slab s only, and every block works on one slab.
//
// Cg in {4, 8}: the 16-block form, v_mfma_f32_4x4x1_16b_f32 -------------
// One instruction is sixteen independent 4x4x1 products. Lane maps (as the
// exact tests confirm them): A and B of lane l belong to block l >> 2, row /
// column l & 3; D register v of lane l is row v, column l & 3 of block
// l >> 2. With block b = output-channel quad 4b..4b+3 of the slab, lane l
// *is* slab channel l in B and in D, and the four rows are four pixels:
//   fwd    A = x[pixel l&3][group(b) * Cg + k]   B = w[l][tap][k]
//   dgrad  A = dout[pixel l&3][group(b) * Cg + k] B = w[group * Cg + k][tap][l % Cg]
//   D reg v = out[pixel v][channel l]
// so one tap costs Cg instructions per 4 pixels, no zero enters the matrix
// unit, and an output row is one 256-B store per register.
//  * Tile: 256 threads = 4 waves on 8 rows x 16 columns of one image; a wave
//    owns 4 image rows (the MFMA rows) x 8 columns (8 independent
//    accumulators, which hide the MFMA latency).
//  * A: at stride 1 and R <= 3 the slab's halo patch of the tile goes to LDS
//    once (row pitch 18 * 64 + 16 floats: the four rows of a read sit on
//    disjoint bank quarters). A lane's A operands of one pixel are one
//    ds_read_b128 per 4 channels, and one window read per tap row serves all
//    s taps. dgrad at stride 1 is the same walk with the taps mirrored.
//    Deviation: stride 2 and R > 3 do not fit the 64-KiB patch budget at this
//    tile; they gather A from global memory with 16-B loads (each 256-B
//    pixel row segment is shared by the 16 blocks), stride-2 dgrad taps
//    predicated on parity. dx pixels no tap reaches come out 0.
//  * B: one tap row (R * Cg floats per lane) is held in registers at a time;
//    a block computes one tile, so every weight is loaded once per block,
//    straight from global memory (dgrad: the in-group transpose, gathered in
//    place; deviation: not staged through LDS, it is read once).
//  * wgrad contracts pixels, one per instruction: A = dout[pix][l], B =
//    x[pix @ tap][group * Cg + 4h + (l & 3)], D reg v of quad (tap, h) =
//    dw[4 * (l >> 2) + v][tap][4h + (l & 3)]. One wave per (slab, split
//    chunk) holds all 9 taps of a 3x3 (36 / 72 accumulator VGPR); for other
//    R the tap row goes into the grid.
//
// Cg in {16, 32, 64}: v_mfma_f32_16x16x4_f32 ------------------------------
// A 16-column tile lies inside one group, so its contraction is dense. The
// tile of conv_f32.hip: 256 threads, 64 pixels x the 64-channel slab, 2x2
// accumulators per wave, k-major LDS with the 80-float stride. Per tap the A
// tile (64 pixels x 64 slab channels) is staged once and shared by the 64/Cg
// groups; column tile j contracts only the Cg channels of its own group
// against Bs[k][column]. wgrad computes only the diagonal Cg x Cg blocks.
// The split between the forms is at Cg 16 because there a 16-column tile
// first fits in one group: below it the 16x16x4 form would multiply zeros
// (4x of the work at Cg 4, 2x at Cg 8).
//
// Arithmetic: f32 fma chains, taps in ascending (r, s), the bias added in
// f32, one rounding per output. wgrad always writes f32 partials per split
// chunk (in dw layout) and a fold kernel adds chunks 0, 1, ... in order: no
// atomics, two runs are bit-identical. Offsets are 64-bit. The entry points
// do not allocate, sync or copy and return nonzero without launching
// outside the envelope.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MFMA16B(a, b, c) __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0)
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

struct GfArgs {
    const float* src;    // fwd: x [Nb,H,W,C]; dgrad: dout [Nb,P,Q,C]
    const float* w;      // [C][R][R][Cg]
    const float* bias;   // [C] or null (fwd only)
    float* dst;          // fwd: out [Nb,P,Q,C]; dgrad: dx [Nb,H,W,C]
    int Nb, H, W, C, P, Q, R, st, pd;
};

// ===================================================== 16-block form ====
constexpr int TP = 8;                 // tile rows
constexpr int TQ = 16;                // tile columns
constexpr int NC = 8;                 // columns (accumulators) per wave
constexpr int PW_MAX = TQ + 2;        // patch columns at R = 3
constexpr int PROW = PW_MAX * 64 + 16;   // patch row pitch (floats)

template <int CG, int SMAX, bool DGRAD, bool PATCH>
__global__ __launch_bounds__(256) void gconv_b16_kernel(GfArgs p, int tilesY,
                                                        int tilesX)
{
    constexpr int NH = CG / 4;        // channel quads per group
    constexpr int NWIN = NC + SMAX - 1;
    __shared__ __attribute__((aligned(16)))
        float patch[PATCH ? (TP + 2) * PROW : 4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int slab = blockIdx.y, C = p.C, R = p.R, RS = R * R;
    const int dH = DGRAD ? p.H : p.P, dW = DGRAD ? p.W : p.Q;
    const int sH = DGRAD ? p.P : p.H, sW = DGRAD ? p.Q : p.W;
    int bid = blockIdx.x;
    const int tx = bid % tilesX;
    bid /= tilesX;
    const int ty = bid % tilesY, n = bid / tilesY;
    const int wr0 = (wv >> 1) * 4, wc0 = (wv & 1) * NC;   // wave's corner
    const int ri = lane & 3;
    const int y = ty * TP + wr0 + ri;         // this lane's A pixel row
    const int xc = tx * TQ + wc0;             // the wave's first column
    const int ch = slab * 64 + lane;          // this lane's B / D channel
    const int achan = slab * 64 + (lane >> 2) * 4 / CG * CG;
    const float* srcn = p.src + (long)n * sH * sW * C;

    if constexpr (PATCH) {
        // stride 1, R <= 3: the halo patch, zero outside the image
        const int PW = TQ + R - 1, PH = TP + R - 1;
        const int o = DGRAD ? p.pd - (R - 1) : -p.pd;
        const int py0 = ty * TP + o, px0 = tx * TQ + o;
        for (int i = t; i < PH * PW * 16; i += 256) {
            const int gq = i & 15, pix = i >> 4;
            const int py = pix / PW, px = pix - py * PW;
            const int sy = py0 + py, sx = px0 + px;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if ((unsigned)sy < (unsigned)sH && (unsigned)sx < (unsigned)sW)
                v = *(const f32x4*)(srcn + ((long)sy * sW + sx) * C +
                                    slab * 64 + gq * 4);
            *(f32x4*)&patch[py * PROW + px * 64 + gq * 4] = v;
        }
        __syncthreads();
    }

    f32x4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int r = 0; r < R; ++r) {
        // ---- B: this lane's tap row, wr[s * CG + k] ----
        float wr[SMAX * CG];
        if (!DGRAD) {
            const float* wp = p.w + ((long)ch * RS + r * R) * CG;
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (s < R) {
#pragma unroll
                    for (int h = 0; h < NH; ++h) {
                        const f32x4 v = *(const f32x4*)(wp + s * CG + h * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) wr[s * CG + h * 4 + e] = v[e];
                    }
                }
        } else {
            const float* wp = p.w + ((long)(ch / CG * CG) * RS + r * R) * CG +
                              ch % CG;
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (s < R) {
#pragma unroll
                    for (int k = 0; k < CG; ++k)
                        wr[s * CG + k] = wp[((long)k * RS + s) * CG];
                }
        }

        if constexpr (PATCH) {
            // one window read serves every s tap of this tap row
            const int rr = DGRAD ? R - 1 - r : r;
            const int PW = TQ + R - 1;
            const float* prow = patch + (wr0 + ri + rr) * PROW +
                                (achan - slab * 64);
            f32x4 win[NWIN][NH];
#pragma unroll
            for (int j = 0; j < NWIN; ++j) {
                const int pc = wc0 + (DGRAD ? R - 1 + j - (SMAX - 1) : j);
#pragma unroll
                for (int h = 0; h < NH; ++h) {
                    win[j][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (pc >= 0 && pc < PW)
                        win[j][h] = *(const f32x4*)(prow + pc * 64 + h * 4);
                }
            }
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (s < R) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const int j = DGRAD ? c - s + SMAX - 1 : c + s;
#pragma unroll
                        for (int h = 0; h < NH; ++h)
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                acc[c] = MFMA16B(win[j][h][e],
                                                 wr[s * CG + h * 4 + e], acc[c]);
                    }
                }
        } else {
            // direct gather: the source row of this lane for tap row r
            int sy;
            bool rok;
            if (!DGRAD) {
                sy = y * p.st - p.pd + r;
                rok = (unsigned)sy < (unsigned)sH;
            } else {
                sy = y + p.pd - r;
                rok = sy >= 0;
                if (p.st == 2) { rok = rok && !(sy & 1); sy >>= 1; }
                rok = rok && sy < sH;
            }
            const float* prow = srcn + (long)(rok ? sy : 0) * sW * C + achan;
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (s < R) {
                    f32x4 a[NC][NH];
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        int sx;
                        bool ok = rok;
                        if (!DGRAD) {
                            sx = (xc + c) * p.st - p.pd + s;
                            ok = ok && (unsigned)sx < (unsigned)sW;
                        } else {
                            sx = xc + c + p.pd - s;
                            ok = ok && sx >= 0;
                            if (p.st == 2) { ok = ok && !(sx & 1); sx >>= 1; }
                            ok = ok && sx < sW;
                        }
#pragma unroll
                        for (int h = 0; h < NH; ++h) {
                            a[c][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
                            if (ok)
                                a[c][h] = *(const f32x4*)
                                    (prow + (long)sx * C + h * 4);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < NC; ++c)
#pragma unroll
                        for (int h = 0; h < NH; ++h)
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                acc[c] = MFMA16B(a[c][h][e],
                                                 wr[s * CG + h * 4 + e], acc[c]);
                }
        }
    }

    // ---- epilogue: register v = image row, lane = channel ----
    const float bv = (!DGRAD && p.bias) ? p.bias[ch] : 0.f;
    float* dstn = p.dst + (long)n * dH * dW * C + ch;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int oy = ty * TP + wr0 + v;
        if (oy >= dH) continue;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (xc + c < dW)
                dstn[((long)oy * dW + xc + c) * C] = acc[c][v] + bv;
    }
}

// One wave per (slab, tap row group, chunk). NTAP 9: all taps of a 3x3;
// NTAP 7: tap row blockIdx.y of an R x R, taps s < R.
template <int CG, int NTAP>
__global__ __launch_bounds__(64) void gconv_b16_wgrad_kernel(
    const float* __restrict__ dout,    // [Nb,P,Q,C]
    const float* __restrict__ x,       // [Nb,H,W,C]
    float* __restrict__ partial,       // [split][C][R*R][CG]
    int Nb, int H, int W, int C, int P, int Q, int R, int st, int pd,
    long chunk)
{
    constexpr int NH = CG / 4;
    const int lane = threadIdx.x, slab = blockIdx.x, z = blockIdx.z;
    const int RS = R * R;
    const long M = (long)Nb * P * Q;
    const long mbeg = (long)z * chunk;
    const long mend = mbeg + chunk < M ? mbeg + chunk : M;
    int xch[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h)
        xch[h] = slab * 64 + (lane >> 2) * 4 / CG * CG + h * 4 + (lane & 3);

    f32x4 acc[NTAP][NH];
#pragma unroll
    for (int tt = 0; tt < NTAP; ++tt)
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[tt][h] = (f32x4){0.f, 0.f, 0.f, 0.f};

    int n = 0, pp = 0, qq = 0;
    if (mbeg < mend) {
        n = (int)(mbeg / ((long)P * Q));
        const int rem = (int)(mbeg - (long)n * P * Q);
        pp = rem / Q;
        qq = rem - pp * Q;
    }
    for (long m = mbeg; m < mend; ++m) {
        const float d = dout[m * C + slab * 64 + lane];
        const float* xn = x + (long)n * H * W * C;
#pragma unroll
        for (int tt = 0; tt < NTAP; ++tt) {
            const int r = NTAP == 9 ? tt / 3 : (int)blockIdx.y;
            const int s = NTAP == 9 ? tt % 3 : tt;
            if (NTAP == 9 || s < R) {
                const int h = pp * st - pd + r, w = qq * st - pd + s;
                const bool ok = (unsigned)h < (unsigned)H &&
                                (unsigned)w < (unsigned)W;
#pragma unroll
                for (int hh = 0; hh < NH; ++hh) {
                    float xv = 0.f;
                    if (ok) xv = xn[((long)h * W + w) * C + xch[hh]];
                    acc[tt][hh] = MFMA16B(d, xv, acc[tt][hh]);
                }
            }
        }
        if (++qq == Q) { qq = 0; if (++pp == P) { pp = 0; ++n; } }
    }

    float* dstp = partial + (long)z * C * RS * CG;
#pragma unroll
    for (int tt = 0; tt < NTAP; ++tt) {
        const int r = NTAP == 9 ? tt / 3 : (int)blockIdx.y;
        const int s = NTAP == 9 ? tt % 3 : tt;
        if (NTAP == 9 || s < R) {
#pragma unroll
            for (int hh = 0; hh < NH; ++hh)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const long ko = slab * 64 + (lane >> 2) * 4 + v;
                    dstp[(ko * RS + r * R + s) * CG + hh * 4 + (lane & 3)] =
                        acc[tt][hh][v];
                }
        }
    }
}

// ======================================================= 16x16x4 form ====
constexpr int LDS_LD = 80;            // LDS row stride (floats)

// fwd:   source pixel of (output pixel, tap); dgrad: the dout pixel
template <bool DGRAD>
__device__ __forceinline__ long gf_gather(const GfArgs& p, int an, int ay,
                                          int ax, int r, int s, bool& ok)
{
    if (!DGRAD) {
        const int h = ay + r, w = ax + s;
        ok = (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
        return ((long)an * p.H + h) * p.W + w;
    }
    int hp = ay - r, wp = ax - s;
    ok = hp >= 0 && wp >= 0;
    if (p.st == 2) {
        ok = ok && !(hp & 1) && !(wp & 1);
        hp >>= 1;
        wp >>= 1;
    }
    ok = ok && hp < p.P && wp < p.Q;
    return ((long)an * p.P + hp) * p.Q + wp;
}

template <int CG, bool DGRAD>
__global__ __launch_bounds__(256) void gconv_d16_kernel(GfArgs p)
{
    constexpr int NB4 = CG / 16;      // B float4 per thread per tap
    __shared__ __attribute__((aligned(16))) float As[64][LDS_LD];  // [ch][px]
    __shared__ __attribute__((aligned(16))) float Bs[CG][LDS_LD];  // [k][col]

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;
    const int slab = blockIdx.y, C = p.C, R = p.R, RS = R * R;
    const long M = DGRAD ? (long)p.Nb * p.H * p.W : (long)p.Nb * p.P * p.Q;
    const long m0 = (long)blockIdx.x * 64;
    const int o_loc = t >> 2, q0 = t & 3;     // A: pixel, channel quads q0+4u

    int an = 0, ay = 0, ax = 0;
    const bool av = m0 + o_loc < M;
    if (av) {
        const long m = m0 + o_loc;
        const int plane = DGRAD ? p.H * p.W : p.P * p.Q;
        const int width = DGRAD ? p.W : p.Q;
        an = (int)(m / plane);
        const int rem = (int)(m - (long)an * plane);
        const int yy = rem / width, xx = rem - yy * width;
        if (DGRAD) { ay = yy + p.pd; ax = xx + p.pd; }
        else { ay = yy * p.st - p.pd; ax = xx * p.st - p.pd; }
    }

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    f32x4 a4[4], b4[NB4];
    auto load_tap = [&](int tap) {
        const int r = tap / R, s = tap - r * R;
        bool ok = false;
        long pix = 0;
        if (av) pix = gf_gather<DGRAD>(p, an, ay, ax, r, s, ok);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a4[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (ok)
                a4[u] = *(const f32x4*)(p.src + pix * C + slab * 64 +
                                        (q0 + 4 * u) * 4);
        }
        // w rows of the slab: row = channel 0..63, CG floats per (row, tap)
#pragma unroll
        for (int bi = 0; bi < NB4; ++bi) {
            const int idx = t + 256 * bi;
            const int row = idx / (CG / 4), kq = idx % (CG / 4);
            b4[bi] = *(const f32x4*)(p.w + ((long)(slab * 64 + row) * RS + tap) *
                                     CG + kq * 4);
        }
    };

    load_tap(0);
    for (int tap = 0; tap < RS; ++tap) {
        __syncthreads();   // previous tap's fragment reads are done
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                As[(q0 + 4 * u) * 4 + e][o_loc] = a4[u][e];
#pragma unroll
        for (int bi = 0; bi < NB4; ++bi) {
            const int idx = t + 256 * bi;
            const int row = idx / (CG / 4), kq = idx % (CG / 4);
            if (!DGRAD) {
                // row = ko (column), k = ci in group
#pragma unroll
                for (int e = 0; e < 4; ++e) Bs[kq * 4 + e][row] = b4[bi][e];
            } else {
                // row = ko = g * CG + k, columns = the group's ci
                *(f32x4*)&Bs[row % CG][row / CG * CG + kq * 4] = b4[bi];
            }
        }
        __syncthreads();
        if (tap + 1 < RS) load_tap(tap + 1);

#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cb = wn + 16 * j;
            // first slab channel of the column tile's group
            const int gb = CG == 16 ? cb : (CG == 32 ? wn : 0);
#pragma unroll
            for (int ks = 0; ks < CG; ks += 4) {
                const int kr = ks + (lane >> 4);
                const float a0 = As[gb + kr][wm + (lane & 15)];
                const float a1 = As[gb + kr][wm + 16 + (lane & 15)];
                const float b = Bs[kr][cb + (lane & 15)];
                acc[0][j] = MFMA16(a0, b, acc[0][j]);
                acc[1][j] = MFMA16(a1, b, acc[1][j]);
            }
        }
    }

    // ---- epilogue: D[row = 4 * (l >> 4) + reg][col = l & 15] ----
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = slab * 64 + wn + j * 16 + (lane & 15);
        const float bv = (!DGRAD && p.bias) ? p.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long row = m0 + wm + i * 16 + (lane >> 4) * 4 + e;
                if (row < M) p.dst[row * C + col] = acc[i][j][e] + bv;
            }
    }
}

// block = (slab, tap, chunk); D rows = ko, columns = ci of the slab, only
// the 16x16 tiles of the diagonal CG x CG blocks (CG / 16 per wave)
template <int CG>
__global__ __launch_bounds__(256) void gconv_d16_wgrad_kernel(
    const float* __restrict__ dout, const float* __restrict__ x,
    float* __restrict__ partial,       // [split][C][R*R][CG]
    int Nb, int H, int W, int C, int P, int Q, int R, int st, int pd,
    long chunk)
{
    constexpr int NTW = CG / 16;
    __shared__ __attribute__((aligned(16))) float As[16][LDS_LD];  // [px][ko]
    __shared__ __attribute__((aligned(16))) float Bs[16][LDS_LD];  // [px][ci]

    const int slab = blockIdx.x, tap = blockIdx.y, z = blockIdx.z;
    const int r = tap / R, s = tap - r * R, RS = R * R;
    const long M = (long)Nb * P * Q;
    const long mbeg = (long)z * chunk;
    const long mend = mbeg + chunk < M ? mbeg + chunk : M;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int k_loc = t >> 4, oq = (t & 15) * 4;
    const int plane = P * Q;

    int ti[NTW], tj[NTW];
#pragma unroll
    for (int u = 0; u < NTW; ++u) {
        if (CG == 64) { ti[u] = (wv >> 1) * 2 + (u >> 1); tj[u] = (wv & 1) * 2 + (u & 1); }
        else if (CG == 32) { ti[u] = wv; tj[u] = (wv >> 1) * 2 + u; }
        else { ti[u] = wv; tj[u] = wv; }
    }
    f32x4 acc[NTW];
#pragma unroll
    for (int u = 0; u < NTW; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};

    f32x4 a4, b4;
    auto load_step = [&](long mb) {
        const long m = mb + k_loc;
        a4 = (f32x4){0.f, 0.f, 0.f, 0.f};
        b4 = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (m < mend) {
            a4 = *(const f32x4*)(dout + m * C + slab * 64 + oq);
            const int n = (int)(m / plane);
            const int rem = (int)(m - (long)n * plane);
            const int pp = rem / Q, qq = rem - pp * Q;
            const int h = pp * st - pd + r, w = qq * st - pd + s;
            if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W)
                b4 = *(const f32x4*)
                    (x + (((long)n * H + h) * W + w) * C + slab * 64 + oq);
        }
    };

    if (mbeg < mend) load_step(mbeg);
    for (long mb = mbeg; mb < mend; mb += 16) {
        __syncthreads();
        *(f32x4*)&As[k_loc][oq] = a4;
        *(f32x4*)&Bs[k_loc][oq] = b4;
        __syncthreads();
        if (mb + 16 < mend) load_step(mb + 16);
#pragma unroll
        for (int ks = 0; ks < 16; ks += 4) {
            const int kr = ks + (lane >> 4);
#pragma unroll
            for (int u = 0; u < NTW; ++u) {
                const float a = As[kr][ti[u] * 16 + (lane & 15)];
                const float b = Bs[kr][tj[u] * 16 + (lane & 15)];
                acc[u] = MFMA16(a, b, acc[u]);
            }
        }
    }

    float* dstp = partial + (long)z * C * RS * CG;
#pragma unroll
    for (int u = 0; u < NTW; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long ko = slab * 64 + ti[u] * 16 + (lane >> 4) * 4 + e;
            const int cl = (tj[u] * 16 + (lane & 15)) % CG;
            dstp[(ko * RS + tap) * CG + cl] = acc[u][e];
        }
}

// dw[i] = sum over chunks in chunk order (fixed order: bitwise repeatable)
__global__ __launch_bounds__(256) void gconv_f32_fold_kernel(
    float* __restrict__ dw, const float* __restrict__ partial, long n,
    int split)
{
    EW_IDX
    for (long i = gid; i < n; i += stride) {
        float a = partial[i];
        for (int zz = 1; zz < split; ++zz) a += partial[(long)zz * n + i];
        dw[i] = a;
    }
}

inline bool gfal16(const void* q) { return q && ((uintptr_t)q & 15) == 0; }

// the envelope; returns Cg, or 0 when the arguments fall outside it
int gconv_f32_cg(int Nb, int H, int W, int C, int G, int P, int Q, int R,
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
    if ((long)Nb * H * W >= (1L << 31)) return 0;
    return Cg;
}

template <int CG, bool DGRAD>
void launch_b16(const GfArgs& p, hipStream_t s)
{
    const int dH = DGRAD ? p.H : p.P, dW = DGRAD ? p.W : p.Q;
    const int tilesY = (dH + TP - 1) / TP, tilesX = (dW + TQ - 1) / TQ;
    dim3 grid((unsigned)((long)p.Nb * tilesY * tilesX), (unsigned)(p.C / 64));
    if (p.st == 1 && p.R <= 3)
        hipLaunchKernelGGL((gconv_b16_kernel<CG, 3, DGRAD, true>), grid,
                           dim3(256), 0, s, p, tilesY, tilesX);
    else if (p.R <= 3)
        hipLaunchKernelGGL((gconv_b16_kernel<CG, 3, DGRAD, false>), grid,
                           dim3(256), 0, s, p, tilesY, tilesX);
    else
        hipLaunchKernelGGL((gconv_b16_kernel<CG, 7, DGRAD, false>), grid,
                           dim3(256), 0, s, p, tilesY, tilesX);
}

template <int CG, bool DGRAD>
void launch_d16(const GfArgs& p, hipStream_t s)
{
    const long M = DGRAD ? (long)p.Nb * p.H * p.W : (long)p.Nb * p.P * p.Q;
    dim3 grid((unsigned)((M + 63) / 64), (unsigned)(p.C / 64));
    hipLaunchKernelGGL((gconv_d16_kernel<CG, DGRAD>), grid, dim3(256), 0, s, p);
}

template <bool DGRAD>
int launch_gconv_f32(const void* src, const void* w, const void* bias,
                     void* dst, int Nb, int H, int W, int C, int G, int P,
                     int Q, int R, int stride, int pad, void* strm)
{
    const int Cg = gconv_f32_cg(Nb, H, W, C, G, P, Q, R, stride, pad);
    if (!Cg || !gfal16(src) || !gfal16(w) || !gfal16(dst)) return 1;
    const int dH = DGRAD ? H : P, dW = DGRAD ? W : Q;
    if ((long)Nb * ((dH + TP - 1) / TP) * ((dW + TQ - 1) / TQ) >= (1L << 31))
        return 1;
    hipStream_t s = (hipStream_t)strm;
    GfArgs p;
    p.src = (const float*)src;
    p.w = (const float*)w;
    p.bias = DGRAD ? nullptr : (const float*)bias;
    p.dst = (float*)dst;
    p.Nb = Nb; p.H = H; p.W = W; p.C = C; p.P = P; p.Q = Q; p.R = R;
    p.st = stride; p.pd = pad;
    switch (Cg) {
    case 4: launch_b16<4, DGRAD>(p, s); break;
    case 8: launch_b16<8, DGRAD>(p, s); break;
    case 16: launch_d16<16, DGRAD>(p, s); break;
    case 32: launch_d16<32, DGRAD>(p, s); break;
    default: launch_d16<64, DGRAD>(p, s); break;
    }
    return 0;
}

}  // namespace

extern "C" int ps_gconv_fwd_f32(
    const void* x, const void* w, const void* bias, void* out,
    int Nb, int H, int W, int C, int G, int P, int Q, int R, int stride,
    int pad, void* strm)
{
    return launch_gconv_f32<false>(x, w, bias, out, Nb, H, W, C, G, P, Q, R,
                                   stride, pad, strm);
}

extern "C" int ps_gconv_dgrad_f32(
    const void* dout, const void* w, void* dx,
    int Nb, int H, int W, int C, int G, int P, int Q, int R, int stride,
    int pad, void* strm)
{
    return launch_gconv_f32<true>(dout, w, nullptr, dx, Nb, H, W, C, G, P, Q,
                                  R, stride, pad, strm);
}

// partial: split * C * R*R * Cg floats, 16-B aligned
extern "C" int ps_gconv_wgrad_f32(
    const void* dout, const void* x, void* partial, void* dw,
    int Nb, int H, int W, int C, int G, int P, int Q, int R, int stride,
    int pad, int split, void* strm)
{
    const int Cg = gconv_f32_cg(Nb, H, W, C, G, P, Q, R, stride, pad);
    if (!Cg || split < 1 || split > 1024 || !gfal16(dout) || !gfal16(x) ||
        !gfal16(partial) || !dw)
        return 1;
    hipStream_t s = (hipStream_t)strm;
    const long M = (long)Nb * P * Q;
    const long chunk = ((M + split - 1) / split + 15) / 16 * 16;
    const float* d = (const float*)dout;
    const float* xi = (const float*)x;
    float* part = (float*)partial;
#define GF_WG_ARGS d, xi, part, Nb, H, W, C, P, Q, R, stride, pad, chunk
    if (Cg <= 8) {
        dim3 grid((unsigned)(C / 64), (unsigned)(R == 3 ? 1 : R),
                  (unsigned)split);
        if (Cg == 4 && R == 3)
            hipLaunchKernelGGL((gconv_b16_wgrad_kernel<4, 9>), grid, dim3(64),
                               0, s, GF_WG_ARGS);
        else if (Cg == 4)
            hipLaunchKernelGGL((gconv_b16_wgrad_kernel<4, 7>), grid, dim3(64),
                               0, s, GF_WG_ARGS);
        else if (R == 3)
            hipLaunchKernelGGL((gconv_b16_wgrad_kernel<8, 9>), grid, dim3(64),
                               0, s, GF_WG_ARGS);
        else
            hipLaunchKernelGGL((gconv_b16_wgrad_kernel<8, 7>), grid, dim3(64),
                               0, s, GF_WG_ARGS);
    } else {
        dim3 grid((unsigned)(C / 64), (unsigned)(R * R), (unsigned)split);
        if (Cg == 16)
            hipLaunchKernelGGL(gconv_d16_wgrad_kernel<16>, grid, dim3(256), 0,
                               s, GF_WG_ARGS);
        else if (Cg == 32)
            hipLaunchKernelGGL(gconv_d16_wgrad_kernel<32>, grid, dim3(256), 0,
                               s, GF_WG_ARGS);
        else
            hipLaunchKernelGGL(gconv_d16_wgrad_kernel<64>, grid, dim3(256), 0,
                               s, GF_WG_ARGS);
    }
#undef GF_WG_ARGS
    const long n = (long)C * R * R * Cg;
    int blocks;
    ew_grid(n, 256, &blocks);
    hipLaunchKernelGGL(gconv_f32_fold_kernel, dim3(blocks), dim3(256), 0, s,
                       (float*)dw, (const float*)part, n, split);
    return 0;
}
