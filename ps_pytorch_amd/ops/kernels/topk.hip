// Block top-k sparsifying gradient codec on the error-feedback path.
//
// The fixed-rate sparse companion of quant.hip's int8 codec (Deep Gradient
// Compression / EF-SGD with top-k): of every 256-element block exactly K
// elements (K in {4, 8, 16, 32}) go on the wire, everything else stays in
// the worker's f32 residual and is re-injected next step. Payload size is
// deterministic (RCCL needs sized buffers) and the PS decode needs no
// atomics.
//
// With c = f32(src) + residual (one f32 add, contraction off):
//   key(i)  = (bits(|c_i|) << 8) | (255 - i),  i = position in the block;
//             the K largest keys are sent: larger magnitude first, ties to
//             the lower index, +-Inf/NaN above every finite value. Positions
//             at or past n in the tail block count as c = +0.
//   payload = [u8 idx : nblk*K][bf16 val : nblk*K], one contiguous byte
//             buffer; a block's K entries in ascending index order,
//             val = bf16(c_i) (round to nearest even).
//   residual (in place) = c - f32(val) at sent positions (exact in f32 for
//             finite c), c elsewhere; nothing is written at or past n.
//   decode  = for j = 0..K-1 in payload order: dst[blk*256 + idx_j] +=
//             f32(val_j) where that position is < n. An all-zero payload (a
//             killed worker's) adds +0 to element 0 of each block K times,
//             so indices may repeat.
//
// pack: one wave (64 lanes x 4 elems) per 256-block, 4 waves per workgroup,
// as quant.hip. The select is a threshold search, no LDS and no atomics: up
// to 31 rounds build the K-th largest magnitude T bit by bit from ballot
// popcounts (4 compares + 4 scalar popcounts per round, the same for every
// K), stopping at the first threshold that exactly K elements reach;
// everything above T is sent, and of the elements equal to T the first
// K - count(> T) in index order. Positions are lane-major, so both that
// rank and the payload slot are prefix popcounts of ballots (v_mbcnt) plus
// the count inside the lane's own quad.
// unpack: same mapping; each lane keeps its 4 dst values in registers, the
// block's K entries are loaded once by lanes 0..K-1 and read lane by lane
// (wave-uniform), and the quad is stored once: coalesced, no atomics, a
// fixed add order, safe with repeated indices.
#include "common.h"

#define TOPK_BLOCK 256

static inline long topk_nblk(long n) { return (n + TOPK_BLOCK - 1) / TOPK_BLOCK; }

// number of set bits of `mask` below this lane
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi(
        (unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// this wave's index in its workgroup, in an SGPR: the block index and with
// it the grid-stride loop, the threshold search and its early stop are
// provably wave-uniform (scalar branches, T in an SGPR)
__device__ __forceinline__ int wave_in_block() {
    return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// The threshold search of the pack: the K-th largest magnitude of the
// block is the largest t with count(m >= t) >= K (count(m >= 0) = 256 >= K),
// built from bit B = 30 down, one round per bit: 4 compares into ballots, 4
// scalar popcounts. A t that exactly K elements reach already separates the
// selection from the rest, so the search stops there: about half the rounds
// on gradients without ties, all 31 on a block whose K-th and (K+1)-th
// magnitudes are equal. Recursion on B instead of a loop: the rounds come
// out as straight-line scalar code (T in an SGPR, one scalar branch each).
template <int K, int B>
__device__ __forceinline__ unsigned topk_threshold(const unsigned (&m)[4],
                                                   unsigned T) {
    unsigned t = T | (1u << B);
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt += __popcll(__ballot(m[k] >= t));
    if (cnt == K) return t;
    if (cnt > K) T = t;
    if constexpr (B > 0) return topk_threshold<K, B - 1>(m, T);
    else return T;
}

template <int K, bool BF16>
__global__ __launch_bounds__(256) void pack_topk_ef_kernel(
    unsigned char* __restrict__ idxs, unsigned short* __restrict__ vals,
    const void* __restrict__ src_, float* __restrict__ residual,
    long n, long nblk)
{
#pragma clang fp contract(off)
    const float* __restrict__ srcf = (const float*)src_;
    const unsigned short* __restrict__ srcb = (const unsigned short*)src_;
    long blk = (long)blockIdx.x * 4 + wave_in_block();
    long stride = (long)gridDim.x * 4;
    for (; blk < nblk; blk += stride) {
        int lane = threadIdx.x & 63;
        long idx = blk * TOPK_BLOCK + (long)lane * 4;
        bool full = idx + 4 <= n;
        float c[4];
        if (full) {
            float4_t e = *(const float4_t*)(residual + idx);
            if constexpr (BF16) {
                unsigned long long u = *(const unsigned long long*)(srcb + idx);
                ushort4_t s = *(ushort4_t*)&u;
                c[0] = bf16_to_f32(s.x) + e.x; c[1] = bf16_to_f32(s.y) + e.y;
                c[2] = bf16_to_f32(s.z) + e.z; c[3] = bf16_to_f32(s.w) + e.w;
            } else {
                float4_t x = *(const float4_t*)(srcf + idx);
                c[0] = x.x + e.x; c[1] = x.y + e.y;
                c[2] = x.z + e.z; c[3] = x.w + e.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                c[k] = (idx + k < n)
                    ? (BF16 ? bf16_to_f32(srcb[idx + k]) : srcf[idx + k])
                          + residual[idx + k]
                    : 0.f;
        }
        unsigned m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = __float_as_uint(c[k]) & 0x7fffffffu;

        unsigned T = topk_threshold<K, 30>(m, 0u);
        // count(m > T) <= K <= count(m >= T): everything above T goes, and
        // the first `need` of the elements equal to T in index order (after
        // an early stop that is all of them, possibly none)
        int above = 0, rank = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            above += __popcll(__ballot(m[k] > T));
            rank += lanes_below(__ballot(m[k] == T));
        }
        int need = K - above;
        bool sel[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bool eq = m[k] == T;
            sel[k] = m[k] > T || (eq && rank < need);
            rank += eq;
        }
        int slot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) slot += lanes_below(__ballot(sel[k]));

        long base = blk * K;
        float4_t en;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            en[k] = c[k];
            // exactly K elements are selected; the slot bound only keeps a
            // wrong count from ever leaving the block's payload entries
            if (sel[k] && slot < K) {
                unsigned short v = f32_to_bf16(c[k]);
                idxs[base + slot] = (unsigned char)(lane * 4 + k);
                vals[base + slot] = v;
                en[k] = c[k] - bf16_to_f32(v);
                ++slot;
            }
        }
        if (full) {
            *(float4_t*)(residual + idx) = en;
        } else {
            for (int k = 0; k < 4 && idx + k < n; ++k) residual[idx + k] = en[k];
        }
    }
}

template <int K, bool ACC>
__global__ __launch_bounds__(256) void unpack_topk_kernel(
    float* __restrict__ dst, const unsigned char* __restrict__ idxs,
    const unsigned short* __restrict__ vals, long n, long nblk)
{
    long blk = (long)blockIdx.x * 4 + wave_in_block();
    long stride = (long)gridDim.x * 4;
    for (; blk < nblk; blk += stride) {
        int lane = threadIdx.x & 63;
        long idx = blk * TOPK_BLOCK + (long)lane * 4;
        bool full = idx + 4 <= n;
        float4_t d = {0.f, 0.f, 0.f, 0.f};
        if constexpr (ACC) {
            if (full) {
                d = *(const float4_t*)(dst + idx);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (idx + k < n) d[k] = dst[idx + k];
            }
        }
        // lanes 0..K-1 fetch the block's entries (K <= 32 < 64)
        int e_idx = 0, e_val = 0;
        if (lane < K) {
            e_idx = idxs[blk * K + lane];
            e_val = (int)((unsigned)vals[blk * K + lane] << 16);
        }
        int pos = lane * 4;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            int i = __builtin_amdgcn_readlane(e_idx, j);
            float v = __int_as_float(__builtin_amdgcn_readlane(e_val, j));
            // entries at or past n land in lanes that store nothing there
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = (i == pos + k) ? d[k] + v : d[k];
        }
        if (full) {
            *(float4_t*)(dst + idx) = d;
        } else {
            for (int k = 0; k < 4 && idx + k < n; ++k) dst[idx + k] = d[k];
        }
    }
}

template <int K>
static void launch_pack_topk(void* payload, const void* src, void* residual,
                             long n, int src_dtype, hipStream_t stream) {
    long nblk = topk_nblk(n);
    unsigned char* idxs = (unsigned char*)payload;
    unsigned short* vals = (unsigned short*)(idxs + nblk * K);
    int blocks; ew_grid(nblk * 64, 256, &blocks);
    if (src_dtype == PS_BF16)
        hipLaunchKernelGGL((pack_topk_ef_kernel<K, true>), dim3(blocks),
                           dim3(256), 0, stream, idxs, vals, src,
                           (float*)residual, n, nblk);
    else
        hipLaunchKernelGGL((pack_topk_ef_kernel<K, false>), dim3(blocks),
                           dim3(256), 0, stream, idxs, vals, src,
                           (float*)residual, n, nblk);
}

template <int K>
static void launch_unpack_topk(void* dst, const void* payload, long n,
                               int accumulate, hipStream_t stream) {
    long nblk = topk_nblk(n);
    const unsigned char* idxs = (const unsigned char*)payload;
    const unsigned short* vals = (const unsigned short*)(idxs + nblk * K);
    int blocks; ew_grid(nblk * 64, 256, &blocks);
    if (accumulate)
        hipLaunchKernelGGL((unpack_topk_kernel<K, true>), dim3(blocks),
                           dim3(256), 0, stream, (float*)dst, idxs, vals, n,
                           nblk);
    else
        hipLaunchKernelGGL((unpack_topk_kernel<K, false>), dim3(blocks),
                           dim3(256), 0, stream, (float*)dst, idxs, vals, n,
                           nblk);
}

// payload: 3*k*ceil(n/256) bytes, 2-B aligned. residual: f32[n], 16-B
// aligned (a bucket slice), read and rewritten in place; it must not alias
// src or payload. Returns 0, or -1 for a k outside {4, 8, 16, 32} (nothing
// is launched).
extern "C" int ps_pack_topk_ef(void* payload, const void* src, void* residual,
                               long n, int k, int src_dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    switch (k) {
    case 4:  launch_pack_topk<4>(payload, src, residual, n, src_dtype, s); break;
    case 8:  launch_pack_topk<8>(payload, src, residual, n, src_dtype, s); break;
    case 16: launch_pack_topk<16>(payload, src, residual, n, src_dtype, s); break;
    case 32: launch_pack_topk<32>(payload, src, residual, n, src_dtype, s); break;
    default: return -1;
    }
    return 0;
}

extern "C" int ps_unpack_topk(void* dst, const void* payload, long n, int k,
                              int accumulate, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    switch (k) {
    case 4:  launch_unpack_topk<4>(dst, payload, n, accumulate, s); break;
    case 8:  launch_unpack_topk<8>(dst, payload, n, accumulate, s); break;
    case 16: launch_unpack_topk<16>(dst, payload, n, accumulate, s); break;
    case 32: launch_unpack_topk<32>(dst, payload, n, accumulate, s); break;
    default: return -1;
    }
    return 0;
}
