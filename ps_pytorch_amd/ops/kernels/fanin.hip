// Rank-ordered gradient fan-in for the gather-mode PS, fused with the
// SGD/momentum update and the wire re-pack.
//
// The arrival-order fan-in (quant.hip / topk.hip accumulate-decodes) zeroes
// an f32 accumulator, reads and rewrites it once per (bucket, worker)
// arrival, and hands it to fused_sgd.hip. Here one launch per bucket decodes
// every selected worker's staged payload in registers, sums them in the
// order the caller lists them (ascending worker rank), and either stores the
// sum (ps_fanin_reduce) or runs the update of fused_sgd_kernel on it without
// the sum ever reaching memory (ps_fanin_sgd).
//
// Sum contract (bit-exact; contraction is off in this file):
//   s = +0.0f; for j = 0 .. nsrc-1 in order: s = s + dec_j, one f32 add each.
//   raw f32 : dec = the value.              raw bf16 : dec = exact widening.
//   q8      : dec = f32(q) * scale_block, one rounded multiply, then the add
//             (the CPU path of unpack_q8; not the fma of unpack_q8_kernel).
//   top-k   : within source j the entries t = 0 .. K-1 are applied in payload
//             order, s[idx_t] += f32(val_t) where blk*256 + idx_t < n;
//             indices may repeat.
//   nsrc = 0 gives +0 everywhere.
// Update contract: sgd_update.h on g = s, then wire = cast(w) — what
// ps_fused_sgd computes from the materialised sum, bit for bit.
//
// Payload layouts are those of quant.hip ([int8 x n][f32 scale x nblk]) and
// topk.hip ([u8 idx x nblk*K][bf16 val x nblk*K]); q8 and top-k payloads
// need 4-B alignment only (slices of the PS stage byte buffer), raw sources
// and dst / w / m / wire are quad-aligned (16 B, bf16 8 B). n % 4 == 0.
//
// Mapping: raw and q8 grid-stride over quads (one float4 of w, m per lane);
// top-k runs one wave per 256-block, each lane keeping its quad in registers
// across all sources while lanes 0..K-1 fetch a source's entries, which
// reach their owner lanes through a wave-private tag map in LDS (a readlane
// loop over all entries in every lane is VALU-bound at 7 sources). Sources
// are taken four at a time so their loads are in flight together before the
// ordered adds. No atomics, no workgroup barrier; nesterov / weight decay /
// wire dtype are wave-uniform runtime branches.
#include "common.h"
#include "sgd_update.h"

#pragma clang fp contract(off)

typedef char fi_char4_t __attribute__((ext_vector_type(4)));

#define FANIN_MAX_SRCS 16
#define FANIN_BLOCK 256

// codec tags shared with ops/functional.py
enum FaninCodec : int { FANIN_F32 = 0, FANIN_BF16 = 1, FANIN_Q8 = 2,
                        FANIN_TOPK = 3 };

struct FaninSrcs { const void* p[FANIN_MAX_SRCS]; };

struct FaninUpd {
    float* w; float* m; void* wire;
    float lr, mu, wd, scale;
    int wire_bf16, nesterov, has_wd;
};

// one source's quad i, decoded
template <int CODEC>
__device__ __forceinline__ float4_t fanin_load(const void* p, long i,
                                               long qbytes) {
    if constexpr (CODEC == FANIN_F32) {
        return ((const float4_t*)p)[i];
    } else if constexpr (CODEC == FANIN_BF16) {
        unsigned long long u = ((const unsigned long long*)p)[i];
        ushort4_t h = *(ushort4_t*)&u;
        return {bf16_to_f32(h.x), bf16_to_f32(h.y), bf16_to_f32(h.z),
                bf16_to_f32(h.w)};
    } else {
        fi_char4_t c = ((const fi_char4_t*)p)[i];
        // a quad never straddles a 256-block
        float sc = ((const float*)((const char*)p + qbytes))[i >> 6];
        return {(float)c.x * sc, (float)c.y * sc, (float)c.z * sc,
                (float)c.w * sc};
    }
}

// sources j .. j+G-1: all loads first, then the adds in source order
template <int CODEC, int G>
__device__ __forceinline__ void fanin_ew_group(float4_t& s,
                                               const FaninSrcs& srcs, int j,
                                               long i, long qbytes) {
    float4_t d[G];
#pragma unroll
    for (int t = 0; t < G; ++t) d[t] = fanin_load<CODEC>(srcs.p[j + t], i, qbytes);
#pragma unroll
    for (int t = 0; t < G; ++t) s = s + d[t];
}

// store the sum, or update w / m / wire from it
template <bool UPDATE>
__device__ __forceinline__ void fanin_finish(float* dst, long i, float4_t s,
                                             float4_t wv, float4_t mv,
                                             const FaninUpd& u) {
    if constexpr (!UPDATE) {
        ((float4_t*)dst)[i] = s;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float wk = wv[k], mk = mv[k];
            sgd_update_elem(wk, mk, s[k], u.scale, u.lr, u.mu, u.wd,
                            u.has_wd != 0, u.nesterov != 0);
            wv[k] = wk; mv[k] = mk;
        }
        ((float4_t*)u.w)[i] = wv;
        ((float4_t*)u.m)[i] = mv;
        if (u.wire != nullptr) {
            if (u.wire_bf16) {
                ushort4_t o = {f32_to_bf16(wv.x), f32_to_bf16(wv.y),
                               f32_to_bf16(wv.z), f32_to_bf16(wv.w)};
                ((ushort4_t*)u.wire)[i] = o;
            } else {
                ((float4_t*)u.wire)[i] = wv;
            }
        }
    }
}

template <int CODEC, bool UPDATE>
__global__ __launch_bounds__(256) void fanin_ew_kernel(
    float* __restrict__ dst, FaninSrcs srcs, int nsrc, long nvec, long qbytes,
    FaninUpd u)
{
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
         i += stride) {
        float4_t wv = {0.f, 0.f, 0.f, 0.f}, mv = {0.f, 0.f, 0.f, 0.f};
        if constexpr (UPDATE) {
            wv = ((const float4_t*)u.w)[i];
            mv = ((const float4_t*)u.m)[i];
        }
        float4_t s = {0.f, 0.f, 0.f, 0.f};
        int j = 0;
        for (; j + 4 <= nsrc; j += 4)
            fanin_ew_group<CODEC, 4>(s, srcs, j, i, qbytes);
        switch (nsrc - j) {
        case 3: fanin_ew_group<CODEC, 3>(s, srcs, j, i, qbytes); break;
        case 2: fanin_ew_group<CODEC, 2>(s, srcs, j, i, qbytes); break;
        case 1: fanin_ew_group<CODEC, 1>(s, srcs, j, i, qbytes); break;
        default: break;
        }
        fanin_finish<UPDATE>(dst, i, s, wv, mv, u);
    }
}

// order LDS traffic between the lanes of one wave (its LDS operations
// execute in issue order; this keeps the compiler from moving them)
__device__ __forceinline__ void fanin_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One top-k source in payload order, whatever its indices: the entries
// (held by lanes 0..K-1) are read lane by lane, wave-uniform, and every lane
// tests its four positions. ~14 VALU instructions per entry: the fallback
// for a source whose block repeats an index (a killed worker's all-zero
// payload).
template <int K>
__device__ __forceinline__ void fanin_topk_ordered(float4_t& d, int e_idx,
                                                   int e_val, int lane) {
    int pos = lane * 4;
#pragma unroll
    for (int e = 0; e < K; ++e) {
        int i = __builtin_amdgcn_readlane(e_idx, e);
        float v = __int_as_float(__builtin_amdgcn_readlane(e_val, e));
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = (i == pos + k) ? d[k] + v : d[k];
    }
}

// top-k sources j .. j+G-1 of block blk: lanes 0..K-1 (K <= 32 < 64) fetch
// every source's entries first; then, source by source, the entries are
// routed to their owner lanes through the wave's 256-word tag map in LDS
// (`tags`, all zero between sources): entry lane t writes t + 1 at its
// index, every lane reads the tags of its quad and pulls the value of a
// tagged position from lane t with one bpermute — per source 4 LDS
// accesses, 4 bpermutes and 4 adds, however large K is. With distinct
// indices a position gets at most one entry of a source, so the payload
// order inside the source cannot matter; a repeated index loses a tag,
// which the entry lanes see when they read theirs back, and that source
// takes fanin_topk_ordered instead. Entries at or past n land in lanes that
// store nothing.
template <int K, int G>
__device__ __forceinline__ void fanin_topk_group(float4_t& d,
                                                 const FaninSrcs& srcs, int j,
                                                 long blk, long nblk,
                                                 int lane, unsigned* tags) {
    int e_idx[G], e_val[G];
#pragma unroll
    for (int t = 0; t < G; ++t) {
        e_idx[t] = 0; e_val[t] = 0;
        if (lane < K) {
            const unsigned char* idxs = (const unsigned char*)srcs.p[j + t];
            const unsigned short* vals =
                (const unsigned short*)(idxs + nblk * K);
            e_idx[t] = idxs[blk * K + lane];
            e_val[t] = (int)((unsigned)vals[blk * K + lane] << 16);
        }
    }
#pragma unroll
    for (int t = 0; t < G; ++t) {
        unsigned mine = (unsigned)lane + 1u, back = mine;
        if (lane < K) tags[e_idx[t]] = mine;
        fanin_wave_sync();
        if (lane < K) back = tags[e_idx[t]];
        uint4 tg = *(const uint4*)(tags + lane * 4);
        fanin_wave_sync();
        if (lane < K) tags[e_idx[t]] = 0u;
        fanin_wave_sync();
        if (__ballot(back != mine) == 0ull) {
            unsigned tk[4] = {tg.x, tg.y, tg.z, tg.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // untagged positions read some lane's value and drop it
                float v = __int_as_float(__builtin_amdgcn_ds_bpermute(
                    (int)((tk[k] - 1u) << 2), e_val[t]));
                d[k] = tk[k] ? d[k] + v : d[k];
            }
        } else {
            fanin_topk_ordered<K>(d, e_idx[t], e_val[t], lane);
        }
    }
}

template <int K, bool UPDATE>
__global__ __launch_bounds__(256) void fanin_topk_kernel(
    float* __restrict__ dst, FaninSrcs srcs, int nsrc, long n, long nblk,
    FaninUpd u)
{
    // wave index in an SGPR: the block loop is provably wave-uniform
    int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    long blk = (long)blockIdx.x * 4 + wave;
    long stride = (long)gridDim.x * 4;
    int lane = threadIdx.x & 63;
    // one tag map per wave, private to it (no workgroup barrier anywhere);
    // fanin_topk_group leaves it zero
    __shared__ unsigned tag_map[4][FANIN_BLOCK];
    unsigned* tags = tag_map[wave];
    *(uint4*)(tags + lane * 4) = make_uint4(0u, 0u, 0u, 0u);
    fanin_wave_sync();
    for (; blk < nblk; blk += stride) {
        long i = blk * (FANIN_BLOCK / 4) + lane;   // quad index
        bool live = i * 4 < n;                     // n % 4 == 0: whole quads
        float4_t wv = {0.f, 0.f, 0.f, 0.f}, mv = {0.f, 0.f, 0.f, 0.f};
        if constexpr (UPDATE) {
            if (live) {
                wv = ((const float4_t*)u.w)[i];
                mv = ((const float4_t*)u.m)[i];
            }
        }
        float4_t s = {0.f, 0.f, 0.f, 0.f};
        int j = 0;
        for (; j + 4 <= nsrc; j += 4)
            fanin_topk_group<K, 4>(s, srcs, j, blk, nblk, lane, tags);
        switch (nsrc - j) {
        case 3: fanin_topk_group<K, 3>(s, srcs, j, blk, nblk, lane, tags); break;
        case 2: fanin_topk_group<K, 2>(s, srcs, j, blk, nblk, lane, tags); break;
        case 1: fanin_topk_group<K, 1>(s, srcs, j, blk, nblk, lane, tags); break;
        default: break;
        }
        if (live) fanin_finish<UPDATE>(dst, i, s, wv, mv, u);
    }
}

template <bool UPDATE>
static int fanin_launch(float* dst, const void* const* srcs, int nsrc,
                        int codec, int k, long n, const FaninUpd& u,
                        hipStream_t stream) {
    if (nsrc < 0 || nsrc > FANIN_MAX_SRCS) return -1;
    if (codec < FANIN_F32 || codec > FANIN_TOPK) return -2;
    if (codec == FANIN_TOPK && k != 4 && k != 8 && k != 16 && k != 32)
        return -3;
    if (n < 0 || (n & 3)) return -4;
    if (n == 0) return 0;
    FaninSrcs S;
    for (int j = 0; j < FANIN_MAX_SRCS; ++j) S.p[j] = j < nsrc ? srcs[j] : nullptr;
    dim3 block(256);
    if (codec == FANIN_TOPK) {
        long nblk = (n + FANIN_BLOCK - 1) / FANIN_BLOCK;
        int blocks; ew_grid(nblk * 64, 256, &blocks);
#define FI_TK(KK) hipLaunchKernelGGL((fanin_topk_kernel<KK, UPDATE>),          \
        dim3(blocks), block, 0, stream, dst, S, nsrc, n, nblk, u)
        switch (k) {
        case 4:  FI_TK(4); break;
        case 8:  FI_TK(8); break;
        case 16: FI_TK(16); break;
        default: FI_TK(32); break;
        }
#undef FI_TK
        return 0;
    }
    long nvec = n / 4;
    long qbytes = n;                       // n % 4 == 0: no quant padding
    int blocks; ew_grid(nvec, 256, &blocks);
#define FI_EW(C) hipLaunchKernelGGL((fanin_ew_kernel<C, UPDATE>),              \
        dim3(blocks), block, 0, stream, dst, S, nsrc, nvec, qbytes, u)
    switch (codec) {
    case FANIN_F32:  FI_EW(FANIN_F32); break;
    case FANIN_BF16: FI_EW(FANIN_BF16); break;
    default:         FI_EW(FANIN_Q8); break;
    }
#undef FI_EW
    return 0;
}

// dst[n] (f32) = the rank-ordered sum of srcs[0 .. nsrc-1] (a host array of
// device pointers, nsrc <= 16). Returns 0, or nonzero without launching
// anything: -1 nsrc outside 0..16, -2 unknown codec, -3 a top-k k outside
// {4, 8, 16, 32}, -4 n negative or not a multiple of 4.
extern "C" int ps_fanin_reduce(void* dst, const void* const* srcs, int nsrc,
                               int codec, int k, long n, void* stream) {
    FaninUpd u = {};
    return fanin_launch<false>((float*)dst, srcs, nsrc, codec, k, n, u,
                               (hipStream_t)stream);
}

// The same sum, consumed in registers by the SGD/momentum update of w and m
// (f32[n]) and the re-pack of wire (f32 or bf16 by wire_dtype; null for
// none). Same return codes.
extern "C" int ps_fanin_sgd(void* w, void* m, void* wire, int wire_dtype,
                            const void* const* srcs, int nsrc, int codec,
                            int k, long n, float lr, float mu, float wd,
                            float scale, int nesterov, void* stream) {
    FaninUpd u;
    u.w = (float*)w; u.m = (float*)m; u.wire = wire;
    u.lr = lr; u.mu = mu; u.wd = wd; u.scale = scale;
    u.wire_bf16 = wire_dtype == PS_BF16;
    u.nesterov = nesterov != 0;
    u.has_wd = wd != 0.0f;
    return fanin_launch<true>(nullptr, srcs, nsrc, codec, k, n, u,
                              (hipStream_t)stream);
}
