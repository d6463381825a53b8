// select.hip.h -- join kinds of pb.overlap other than inner (how = "semi" / "anti" / "left"): ordered stream compaction of the
// probe rows over their per-probe match counts.
//
// The counts are what count_overlaps returns for the very same call -- int32 from k_count_overlaps (count_nearest.hip.h), int64
// from the count form of k_overlap_thresh (thresh.hip.h) -- written by those kernels, unchanged, into a scratch column of the
// context, indexed by the probe's position in the caller's columns.  They never leave the device and no pair is enumerated.
//     keep[i] = (counts[i] > 0) != anti                      semi: anti = 0, anti: anti = 1
// A tile of SELECT_TILE consecutive probes is one workgroup; a thread owns SELECT_ITEMS consecutive probes (blocked, so that
// thread order = row order).  Two launches around one device-wide scan (host_core.hip.h: device_scan, the single-launch look-back
// scan):
//   k_select_count   tile_tot[tile] = kept rows of the tile
//   (scan)           tile_tot -> exclusive tile bases, the slot behind the last tile = the number of selected rows (one 8-byte D2H)
//   k_select_emit    flags again, block_exclusive_scan of the per-thread kept counts, row ids at base + prefix: ascending, no atomics,
//                    identical from run to run.  The id is row_id[position] when the side has row ids, else the position.
//                    pad (optional) receives -1 at the same output positions: the (row, -1) tail of the left outer join goes
//                    straight behind the inner pairs in the caller's two pair columns.
// The output pointers may be only 4-byte aligned (a base plus an odd pair count): every output store is a 4-byte scalar.  The
// count column is the context's own (256-byte aligned), so full tiles read it with 16-byte loads.
// What bounds it: bytes.  Per probe the two passes read the count twice (2 x 4 bytes plain, 2 x 8 thresholded) and write 4 bytes
// (8 with pad) per SELECTED row; the count kernel before it reads the 12 bytes of the probe and writes the 4 (8) of the count.
#pragma once
#include "scan.hip.h"

namespace ivj {

constexpr int SELECT_THREADS = 256;
constexpr int SELECT_ITEMS = 8;
constexpr int SELECT_TILE = SELECT_THREADS * SELECT_ITEMS;   // probes per workgroup
static_assert(SELECT_THREADS == SCAN_THREADS, "block_exclusive_scan is written for SCAN_THREADS");
static_assert(SELECT_ITEMS == 8, "select_keep loads eight counts per thread");

// bit k = probe i0 + k is kept; probes at or beyond n are never kept.  counts is 16-byte aligned, i0 a multiple of SELECT_ITEMS.
template <class CT>
__device__ __forceinline__ unsigned select_keep(const CT* __restrict__ counts, int64_t i0, int64_t n, bool anti) {
    unsigned keep = 0u;
    if (i0 + SELECT_ITEMS <= n) {
        if (sizeof(CT) == 4) {
            const int4* p = reinterpret_cast<const int4*>(counts + i0);
            const int4 a = p[0], b = p[1];
            const int v[SELECT_ITEMS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int k = 0; k < SELECT_ITEMS; ++k) keep |= ((v[k] > 0) != anti ? 1u : 0u) << k;
        } else {
            typedef long long v2ll __attribute__((ext_vector_type(2)));
            const v2ll* p = reinterpret_cast<const v2ll*>(counts + i0);
#pragma unroll
            for (int k = 0; k < SELECT_ITEMS; k += 2) {
                const v2ll v = p[k / 2];
                keep |= ((v.x > 0) != anti ? 1u : 0u) << k;
                keep |= ((v.y > 0) != anti ? 1u : 0u) << (k + 1);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < SELECT_ITEMS; ++k)
            if (i0 + k < n) keep |= ((counts[i0 + k] > 0) != anti ? 1u : 0u) << k;
    }
    return keep;
}

template <class CT>
__global__ __launch_bounds__(SELECT_THREADS) void k_select_count(const CT* __restrict__ counts, int64_t n, int anti,
                                                                 long long* __restrict__ tile_tot) {
    __shared__ int lds[SELECT_THREADS / kWave];
    const int64_t i0 = (int64_t)blockIdx.x * SELECT_TILE + (int64_t)threadIdx.x * SELECT_ITEMS;
    const unsigned keep = select_keep(counts, i0, n, anti != 0);
    int tot;
    block_exclusive_scan((int)__popc(keep), SumOp(), 0, lds, &tot);
    if (threadIdx.x == 0) tile_tot[blockIdx.x] = (long long)tot;
}

// tile_base = the exclusive scan of k_select_count's totals.  rows (and pad, when given) hold at least the scan's total.
template <class CT>
__global__ __launch_bounds__(SELECT_THREADS) void k_select_emit(const CT* __restrict__ counts, int64_t n, int anti,
                                                                const int32_t* __restrict__ row_id, const long long* __restrict__ tile_base,
                                                                int32_t* __restrict__ rows, int32_t* __restrict__ pad) {
    __shared__ int lds[SELECT_THREADS / kWave];
    const int64_t i0 = (int64_t)blockIdx.x * SELECT_TILE + (int64_t)threadIdx.x * SELECT_ITEMS;
    const unsigned keep = select_keep(counts, i0, n, anti != 0);
    int tot;
    const int pre = block_exclusive_scan((int)__popc(keep), SumOp(), 0, lds, &tot);
    if (tot == 0) return;                                  // uniform
    long long o = tile_base[blockIdx.x] + pre;
#pragma unroll
    for (int k = 0; k < SELECT_ITEMS; ++k) {
        if (!((keep >> k) & 1u)) continue;
        rows[o] = row_id ? row_id[i0 + k] : (int32_t)(i0 + k);
        if (pad) pad[o] = -1;
        ++o;
    }
}

}  // namespace ivj
