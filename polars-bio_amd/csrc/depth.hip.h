// depth.hip.h -- pb.depth: run-length coverage blocks (chrom, start, end, depth) of ONE interval frame, on the sorted index.
//
// The index already holds both event streams of a sweep, sorted per contig and sharing the segment offsets:
//   A = (contig, start)   b_contig / b_start      one "+1" per row
//   B = (contig, end')    b_contig / e_end        one "-1" per row      end' = end (Strict, half-open) or end + 1 (Weak, closed)
// After i events of A and j events of B of the merged sequence the depth is i - j, so no +-1 scan is needed: a merge
// path over the two sequences gives every event its (i, j), and only the LAST event of a group of equal (contig, position)
// is looked at -- events at one position are netted before anything is emitted (a read that ends where the next one starts
// does not split a block, Weak [1,5] + [6,9] is one block).  With
//   d_before(K) = #A < K - #B < K        d_after(K) = #A <= K - #B <= K
// a group K is a boundary iff d_after != d_before; it OPENS a block when d_after != 0 and CLOSES the block the previous
// boundary opened when d_before != 0.  Opens and closes pair up one to one (the depth is 0 at the end of every contig), so one
// exclusive count of the opens places both: an open writes (contig, start, depth) at its rank r, a close writes end at r - 1.
//
// Keys are 64 bits: contig << 33 | position, position = flip(x) (+ 1 for a Weak end: 33 bits, the "+1" never wraps -- the
// form count_nearest.hip.h uses for its targets).  Rows outside the dictionary carry contig = n_contigs in the index: they
// sort behind every dictionary row, take part in the merge and are dropped when a block would be emitted.
//
// Launches: k_depth_partition (one merge-path search per tile edge), k_depth_tile<.., false> (open count per tile), a scan of
// the tile counts, k_depth_tile<.., true> (the same walk, writing).  A tile is DP_TILE merged events: both runs are staged in
// LDS with one element before and one behind each, so that "same key as the event before / after the tile" needs no global
// read; only a group that reaches back over a tile edge pays a global bound search (dp_lower_bound) for its d_before.
//
// The walk assumes end' >= start for every dictionary row.  Rows with start > end (flags[0] of the index) would make the
// depth negative between end' and start: the host driver (host_depth.hip.h) re-indexes such a frame without its empty rows.
#pragma once
#include "index_view.hip.h"
#include "scan.hip.h"

namespace ivj {

constexpr int DP_THREADS = 256;
static_assert(DP_THREADS == SCAN_THREADS, "block_exclusive_scan of scan.hip.h is shared");
constexpr int DP_ITEMS = 8;
constexpr int DP_TILE = DP_THREADS * DP_ITEMS;       // merged events per workgroup (starts + ends)
constexpr int DP_LDS = DP_TILE + 4;                  // both runs + {before, behind} of each
constexpr unsigned long long DP_NONE = ~0ull;        // no element: larger than every key (position <= 2^32, contig < 2^31)

__device__ __forceinline__ unsigned long long dp_key(int32_t contig, unsigned long long pos) {
    return ((unsigned long long)(uint32_t)contig << 33) | pos;
}
template <bool STRICT, bool ENDS>
__device__ __forceinline__ unsigned long long dp_load(const int32_t* __restrict__ contig, const int32_t* __restrict__ x, int64_t p, int64_t n) {
    if (p < 0 || p >= n) return DP_NONE;
    return dp_key(contig[p], (unsigned long long)flip(x[p]) + ((ENDS && !STRICT) ? 1ull : 0ull));
}

// first position of [0, hi) whose key is >= K
template <bool STRICT, bool ENDS>
__device__ __forceinline__ int64_t dp_lower_bound(const int32_t* __restrict__ contig, const int32_t* __restrict__ x, int64_t hi, int64_t n,
                                                  unsigned long long K) {
    int64_t lo = 0;
    while (lo < hi) {
        const int64_t m = lo + ((hi - lo) >> 1);
        if (dp_load<STRICT, ENDS>(contig, x, m, n) < K) lo = m + 1; else hi = m;
    }
    return lo;
}

// part[t] = number of starts among the first min(t * DP_TILE, 2 n) merged events (a start goes first among equal keys)
template <bool STRICT>
__global__ __launch_bounds__(DP_THREADS) void k_depth_partition(const int32_t* __restrict__ b_contig, const int32_t* __restrict__ b_start,
                                                               const int32_t* __restrict__ e_end, int64_t n, int64_t n_tiles,
                                                               uint32_t* __restrict__ part) {
    const int64_t t = (int64_t)blockIdx.x * DP_THREADS + threadIdx.x;
    if (t > n_tiles) return;
    int64_t d = t * DP_TILE;
    if (d > 2 * n) d = 2 * n;
    int64_t lo = d > n ? d - n : 0, hi = d < n ? d : n;
    while (lo < hi) {
        const int64_t m = lo + ((hi - lo) >> 1);
        const unsigned long long a = dp_load<STRICT, false>(b_contig, b_start, m, n);
        const unsigned long long b = dp_load<STRICT, true>(b_contig, e_end, d - 1 - m, n);
        if (a <= b) lo = m + 1; else hi = m;
    }
    part[t] = (uint32_t)lo;
}

// One tile of the merged sequence.  FILL = false: tile_count[tile] = blocks opened in the tile.  FILL = true: the blocks are
// written, tile_off[tile] = blocks opened before the tile, n_out = blocks in all (no store goes past it).
// RUNS (setop.hip.h: the union runs of a frame): only the transitions between depth 0 and depth >= 1 are boundaries -- a group
// opens iff d_before == 0 && d_after != 0 and closes iff d_before != 0 && d_after == 0; o_depth is not written.
template <bool STRICT, bool FILL, bool RUNS = false>
__global__ __launch_bounds__(DP_THREADS) void k_depth_tile(const int32_t* __restrict__ b_contig, const int32_t* __restrict__ b_start,
                                                          const int32_t* __restrict__ e_end, int64_t n, int32_t n_contigs,
                                                          const uint32_t* __restrict__ part, uint32_t* __restrict__ tile_count,
                                                          const uint32_t* __restrict__ tile_off, uint32_t n_out, int32_t* __restrict__ o_contig,
                                                          int32_t* __restrict__ o_start, int32_t* __restrict__ o_end, int32_t* __restrict__ o_depth) {
    __shared__ unsigned long long keys[DP_LDS];
    __shared__ uint32_t l_scan[DP_THREADS / kWave];
    const int64_t tile = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t d0 = tile * DP_TILE;
    const int64_t d1 = d0 + DP_TILE < 2 * n ? d0 + DP_TILE : 2 * n;
    const int64_t i0 = part[tile], i1 = part[tile + 1];
    const int64_t j0 = d0 - i0, j1 = d1 - i1;
    const int na = (int)(i1 - i0), nb = (int)(j1 - j0), cnt = na + nb;       // cnt <= DP_TILE
    // slot 0 = the element before the run, 1 .. len the run, len + 1 the element behind it
    unsigned long long* sA = keys;
    unsigned long long* sB = keys + na + 2;
    for (int k = tid; k < na + 2; k += DP_THREADS) sA[k] = dp_load<STRICT, false>(b_contig, b_start, i0 - 1 + k, n);
    for (int k = tid; k < nb + 2; k += DP_THREADS) sB[k] = dp_load<STRICT, true>(b_contig, e_end, j0 - 1 + k, n);
    __syncthreads();

    const int diag = tid * DP_ITEMS < cnt ? tid * DP_ITEMS : cnt;
    int i, j;
    {
        int lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (sA[1 + m] <= sB[diag - m]) lo = m + 1; else hi = m;          // sB[1 + (diag - 1 - m)]
        }
        i = lo; j = diag - lo;
    }
    unsigned long long a = sA[1 + i], b = sB[1 + j];
    int32_t db = 0;                                                          // depth before the group the walk stands in
    if (diag < cnt) {
        const unsigned long long K0 = a <= b ? a : b;
        if (sA[i] != K0 && sB[j] != K0) {
            db = (int32_t)((i0 + i) - (j0 + j));
        } else {
            // the group began before this thread: count the elements below K0 of both runs
            int64_t la, lb;
            {
                int lo = 1, hi = i + 1;
                while (lo < hi) { const int m = (lo + hi) >> 1; if (sA[m] < K0) lo = m + 1; else hi = m; }
                la = (lo == 1 && sA[0] == K0) ? dp_lower_bound<STRICT, false>(b_contig, b_start, i0 - 1, n, K0) : i0 + lo - 1;
            }
            {
                int lo = 1, hi = j + 1;
                while (lo < hi) { const int m = (lo + hi) >> 1; if (sB[m] < K0) lo = m + 1; else hi = m; }
                lb = (lo == 1 && sB[0] == K0) ? dp_lower_bound<STRICT, true>(b_contig, e_end, j0 - 1, n, K0) : j0 + lo - 1;
            }
            db = (int32_t)(la - lb);
        }
    }

    unsigned long long gk[DP_ITEMS];                 // key of the group that ends at item k
    int32_t gd[DP_ITEMS];                            // depth behind it
    uint32_t open_mask = 0, close_mask = 0;
#pragma unroll
    for (int k = 0; k < DP_ITEMS; ++k) {
        gk[k] = 0; gd[k] = 0;
        if (diag + k < cnt) {
            unsigned long long K;
            if (a <= b) { K = a; ++i; a = sA[1 + i]; } else { K = b; ++j; b = sB[1 + j]; }
            const unsigned long long next = a <= b ? a : b;
            if (next != K) {
                const int32_t da = (int32_t)((i0 + i) - (j0 + j));
                const bool live = da != db && (uint32_t)(K >> 33) < (uint32_t)n_contigs;
                if constexpr (RUNS) {
                    if (live && db == 0) open_mask |= 1u << k;
                    if (live && da == 0) close_mask |= 1u << k;
                } else {
                    if (live && da != 0) open_mask |= 1u << k;
                    if (live && db != 0) close_mask |= 1u << k;
                }
                gk[k] = K; gd[k] = da;
                db = da;
            }
        }
    }
    uint32_t total = 0;
    uint32_t r = block_exclusive_scan((uint32_t)__popc(open_mask), SumOp(), 0u, l_scan, &total);
    if constexpr (!FILL) {
        if (tid == 0) tile_count[tile] = total;
    } else {
        r += tile_off[tile];
#pragma unroll
        for (int k = 0; k < DP_ITEMS; ++k) {
            const unsigned long long pos = gk[k] & ((1ull << 33) - 1ull);
            if ((close_mask & (1u << k)) && r >= 1u && r <= n_out) {       // r >= 1: a close follows the open of the boundary before it
                __builtin_nontemporal_store(unflip((uint32_t)(pos - (STRICT ? 0ull : 1ull))), o_end + (r - 1));
            }
            if ((open_mask & (1u << k)) && r < n_out) {
                __builtin_nontemporal_store((int32_t)(gk[k] >> 33), o_contig + r);
                __builtin_nontemporal_store(unflip((uint32_t)pos), o_start + r);
                if constexpr (!RUNS) __builtin_nontemporal_store(gd[k], o_depth + r);
                ++r;
            }
        }
    }
}

// the slow path's input: the index's own rows in start order, rows that cover nothing (and rows outside the dictionary) marked -1
template <bool STRICT>
__global__ void k_depth_sanitize(const int32_t* __restrict__ b_contig, const int32_t* __restrict__ b_start, const int2* __restrict__ ep,
                                 int64_t n, int32_t n_contigs, int32_t* __restrict__ c, int32_t* __restrict__ s, int32_t* __restrict__ e) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int32_t ct = b_contig[p], st = b_start[p], en = ep[p].x;
    const bool covers = STRICT ? st < en : st <= en;
    c[p] = (covers && (uint32_t)ct < (uint32_t)n_contigs) ? ct : -1;
    s[p] = st; e[p] = en;
}

}  // namespace ivj
