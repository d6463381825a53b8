// group.hip.h -- dense group ids over (contig, on_col codes...) for joins keyed on extra columns (on_cols).
//
// The join kernels partition by one int32 id per row and ignore rows whose id lies outside [0, n_contigs).  A dense id over the
// composite key (chrom, code_1, ..., code_K) stands in for the chrom id, and every existing kernel then joins within groups.
//
// key = ((chrom * card_1 + code_1) * card_2 + code_2) ...   in [0, D), D = n_contigs * prod(card_i) <= 2^31
// gid = rank of the row's key among the keys the BUILD side holds (ascending key order); -1 for a null component (< 0) or a key
//       the build side lacks.
//
// Four passes (ivj_group_ids_dev, host_group.hip.h):
//   mark    one bit per build key in a D-bit bitmap.  Most marks repeat a bit already set (strand only: ~75 hot words), so the
//           bitmap is privatized in LDS when it fits (D <= 2^18 bits = 32 KiB) and only non-zero words are OR-ed out; larger
//           domains test the word before the global atomicOr.
//   rank    popcount per word + exclusive scan of the D / 32 counts (device_scan).
//   remap   both sides: gid = rank[key >> 5] + popc(word & below).
//   table   one row (chrom, code_1, ..., code_K) per gid out of the set bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan.hip.h"

namespace ivj {

constexpr int GRP_MAX_COLS = 8;                      // on_cols one call takes
constexpr int GRP_THREADS = 256;
constexpr int64_t GRP_LDS_BITS = 1ll << 18;          // bitmaps up to this size are privatized in LDS (32 KiB)
constexpr int64_t GRP_MAX_DOMAIN = 1ll << 31;

// The key columns of one side.  Passed by value; every access to code / card uses a compile-time index (the loops below are
// fully unrolled and guarded by j < k), so the struct stays in kernel-argument registers and nothing spills to scratch.
struct GroupCols {
    const int32_t* contig;
    const int32_t* code[GRP_MAX_COLS];
    int32_t card[GRP_MAX_COLS];
    int32_t k;
    int32_t n_contigs;
    int64_t n;
};

// the row's key, or -1 for a null / out-of-range component (every prefix product is < D <= 2^31: uint32 arithmetic is exact)
__device__ __forceinline__ int64_t group_key(const GroupCols& c, int64_t i) {
    const int32_t ch = c.contig[i];
    if ((uint32_t)ch >= (uint32_t)c.n_contigs) return -1;
    uint32_t key = (uint32_t)ch;
#pragma unroll
    for (int j = 0; j < GRP_MAX_COLS; ++j) {
        if (j < c.k) {
            const int32_t v = c.code[j][i];
            if ((uint32_t)v >= (uint32_t)c.card[j]) return -1;
            key = key * (uint32_t)c.card[j] + (uint32_t)v;
        }
    }
    return (int64_t)key;
}

// mark, LDS-privatized: every workgroup sets bits in its own copy of the bitmap (words * 4 bytes of dynamic LDS), then ORs its
// non-zero words into the global bitmap (testing the global word first: hot words are shared by every workgroup)
__global__ __launch_bounds__(GRP_THREADS) void k_group_mark_lds(GroupCols c, uint32_t words, uint32_t* __restrict__ bitmap) {
    extern __shared__ uint32_t s_bits[];
    for (uint32_t w = threadIdx.x; w < words; w += GRP_THREADS) s_bits[w] = 0u;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * GRP_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x; i < c.n; i += stride) {
        const int64_t key = group_key(c, i);
        if (key >= 0) {
            const uint32_t m = 1u << (key & 31);
            uint32_t* w = &s_bits[key >> 5];
            if (!(*w & m)) atomicOr(w, m);
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < words; w += GRP_THREADS) {
        const uint32_t v = s_bits[w];
        if (v && (bitmap[w] & v) != v) atomicOr(&bitmap[w], v);
    }
}

// mark, global bitmap (zeroed by the caller): test before the atomic (a repeated key costs one cached load)
__global__ __launch_bounds__(GRP_THREADS) void k_group_mark_global(GroupCols c, uint32_t* __restrict__ bitmap) {
    const int64_t stride = (int64_t)gridDim.x * GRP_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x; i < c.n; i += stride) {
        const int64_t key = group_key(c, i);
        if (key >= 0) {
            const uint32_t m = 1u << (key & 31);
            uint32_t* w = &bitmap[key >> 5];
            if (!(*w & m)) atomicOr(w, m);
        }
    }
}

__global__ __launch_bounds__(GRP_THREADS) void k_group_popc(const uint32_t* __restrict__ bitmap, int64_t words, uint32_t* __restrict__ cnt) {
    const int64_t w = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x;
    if (w < words) cnt[w] = (uint32_t)__popc(bitmap[w]);
}

// remap: gid of every row of one side, GRP_REMAP_ITEMS consecutive rows per thread (16-byte loads and store when every column is
// 16-byte aligned).  gid may alias c.contig: each thread reads its rows before it writes them.
constexpr int GRP_REMAP_ITEMS = 4;

__device__ __forceinline__ int32_t group_gid(int64_t key, const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ rank) {
    if (key < 0) return -1;
    const uint32_t word = bitmap[key >> 5];
    const uint32_t m = 1u << (key & 31);
    return (word & m) ? (int32_t)(rank[key >> 5] + (uint32_t)__popc(word & (m - 1u))) : -1;
}

__global__ __launch_bounds__(GRP_THREADS) void k_group_remap(GroupCols c, const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ rank,
                                                             int32_t* gid, int vec) {
    const int64_t i0 = ((int64_t)blockIdx.x * GRP_THREADS + threadIdx.x) * GRP_REMAP_ITEMS;
    if (i0 >= c.n) return;
    if (vec && i0 + GRP_REMAP_ITEMS <= c.n) {
        const int4 ch = *reinterpret_cast<const int4*>(c.contig + i0);
        int32_t v0[4] = {ch.x, ch.y, ch.z, ch.w};
        uint32_t key[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { ok[u] = (uint32_t)v0[u] < (uint32_t)c.n_contigs; key[u] = (uint32_t)v0[u]; }
#pragma unroll
        for (int j = 0; j < GRP_MAX_COLS; ++j) {
            if (j < c.k) {
                const int4 cv = *reinterpret_cast<const int4*>(c.code[j] + i0);
                const int32_t v[4] = {cv.x, cv.y, cv.z, cv.w};
                const uint32_t card = (uint32_t)c.card[j];
#pragma unroll
                for (int u = 0; u < 4; ++u) { ok[u] = ok[u] && (uint32_t)v[u] < card; key[u] = key[u] * card + (uint32_t)v[u]; }
            }
        }
        int4 o;
        o.x = group_gid(ok[0] ? (int64_t)key[0] : -1, bitmap, rank);
        o.y = group_gid(ok[1] ? (int64_t)key[1] : -1, bitmap, rank);
        o.z = group_gid(ok[2] ? (int64_t)key[2] : -1, bitmap, rank);
        o.w = group_gid(ok[3] ? (int64_t)key[3] : -1, bitmap, rank);
        *reinterpret_cast<int4*>(gid + i0) = o;
        return;
    }
    const int64_t hi = i0 + GRP_REMAP_ITEMS < c.n ? i0 + GRP_REMAP_ITEMS : c.n;
    for (int64_t i = i0; i < hi; ++i) gid[i] = group_gid(group_key(c, i), bitmap, rank);
}

// table: row g = (chrom, code_1, ..., code_K) of the g-th present key; rows at or past `cap` are not written
__global__ __launch_bounds__(GRP_THREADS) void k_group_table(const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ rank, int64_t words,
                                                             GroupCols c, int32_t* __restrict__ keys, int64_t cap) {
    const int64_t w = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x;
    if (w >= words) return;
    uint32_t bits = bitmap[w];
    int64_t g = rank[w];
    const int stride = 1 + c.k;
    while (bits) {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1u;
        if (g >= cap) return;
        uint32_t rem = (uint32_t)(w * 32 + b);
        int32_t* row = keys + g * stride;
#pragma unroll
        for (int j = GRP_MAX_COLS - 1; j >= 0; --j) {
            if (j < c.k) {
                const uint32_t card = (uint32_t)c.card[j];
                row[1 + j] = (int32_t)(rem % card);
                rem /= card;
            }
        }
        row[0] = (int32_t)rem;
        ++g;
    }
}

}  // namespace ivj
