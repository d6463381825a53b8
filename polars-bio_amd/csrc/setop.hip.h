// setop.hip.h -- set algebra on the positions two interval frames cover: intersection, union, difference, symmetric
// difference as maximal runs (chrom, start, end), and the three class totals (only df1, only df2, both) behind pb.jaccard.
//
// Step 1 (depth.hip.h, k_depth_tile<.., RUNS = true>) turns each frame into its union runs: the depth walk keeping only the
// transitions between depth 0 and depth >= 1.  Per contig a run list is strictly increasing, s0 < e0' < s1 < e1' < ...
// (e' = the half-open end: end for Strict, end + 1 for Weak), so read as a BOUNDARY STREAM -- element 2 r = the start of
// run r, element 2 r + 1 = its end' -- it is a strictly increasing sequence of depth's keys, contig << 33 | flip(pos).
//
// Step 2, here: a merge path over the two boundary streams.  After i events of stream 1 and j of stream 2 the walk stands
// inside U(df1) iff i is odd and inside U(df2) iff j is odd: the state is the pair of parities, (i & 1) | (j & 1) << 1, and
// no scan is needed.  Events at one position are netted before anything is emitted, as depth does; because each stream is
// strictly increasing a group of equal keys holds at most ONE event of each stream, so one element of look-back and
// look-ahead decides it (no global search): stream 1 goes first among equals, a stream-1 event whose key equals stream 2's
// next element leaves the group to that event, a stream-2 event whose key equals stream 1's previous element owns a group
// of two.  The operation is a 4-bit truth table f over the state (bit s = "state s belongs to the result"): a group is a
// boundary iff f(before) != f(after), it opens a region when f(after) and closes one otherwise.  f(0) = 0 for every
// operation and the state is 0 at the end of every contig, so opens and closes pair up: one exclusive count of the opens
// places both -- an open writes (contig, start) at its rank r, a close writes end at r - 1.
//
// Launches: k_so_partition (one merge-path search per tile edge), k_so_tile<.., SO_COUNT>, a scan of the tile counts,
// k_so_tile<.., SO_FILL>.  A tile is SO_TILE merged events, both stream pieces staged in LDS with one element before and
// one behind each.  SO_STATS replaces count / scan / fill: per tile, for each class, sum(close positions) - sum(open
// positions) in uint64 with wrap-around (no tile needs its neighbour), and the opens of the class "both"; k_so_reduce adds
// the per-tile words in one workgroup (integers only, no atomics).
#pragma once
#include "depth.hip.h"

namespace ivj {

constexpr int SO_THREADS = 256;
static_assert(SO_THREADS == SCAN_THREADS, "block_exclusive_scan of scan.hip.h is shared");
constexpr int SO_ITEMS = 8;
constexpr int SO_TILE = SO_THREADS * SO_ITEMS;       // merged boundary events per workgroup
constexpr int SO_LDS = SO_TILE + 4;                  // both pieces + {before, behind} of each
constexpr int SO_COUNT = 0, SO_FILL = 1, SO_STATS = 2;
constexpr int SO_STAT_WORDS = 4;                     // only df1, only df2, both, regions of "both"

// the union runs of one frame; n = boundary events = 2 * runs
struct SoStream {
    const int32_t* contig;
    const int32_t* start;
    const int32_t* end;
    int64_t n;
};

template <bool STRICT>
__device__ __forceinline__ unsigned long long so_load(const SoStream& s, int64_t p) {
    if (p < 0 || p >= s.n) return DP_NONE;
    const int64_t r = p >> 1;
    if (p & 1) return dp_key(s.contig[r], (unsigned long long)flip(s.end[r]) + (STRICT ? 0ull : 1ull));
    return dp_key(s.contig[r], (unsigned long long)flip(s.start[r]));
}

// part[t] = events of stream 1 among the first min(t * SO_TILE, a.n + b.n) merged events (stream 1 goes first among equal keys)
template <bool STRICT>
__global__ __launch_bounds__(SO_THREADS) void k_so_partition(SoStream a, SoStream b, int64_t n_tiles, uint32_t* __restrict__ part) {
    const int64_t t = (int64_t)blockIdx.x * SO_THREADS + threadIdx.x;
    if (t > n_tiles) return;
    int64_t d = t * SO_TILE;
    if (d > a.n + b.n) d = a.n + b.n;
    int64_t lo = d > b.n ? d - b.n : 0, hi = d < a.n ? d : a.n;
    while (lo < hi) {
        const int64_t m = lo + ((hi - lo) >> 1);
        if (so_load<STRICT>(a, m) <= so_load<STRICT>(b, d - 1 - m)) lo = m + 1; else hi = m;
    }
    part[t] = (uint32_t)lo;
}

// One tile of the merged boundary sequence.  table: bit s = state s belongs to the result (s = in-U1 | in-U2 << 1).
// SO_COUNT: tile_count[tile] = regions opened in the tile.  SO_FILL: the regions are written, tile_off[tile] = regions opened
// before the tile, n_out = regions in all (no store goes past it).  SO_STATS: tile_stats[4 tile ..] = the tile's share of the
// three class totals and the regions of "both" it opens; table is not read.
template <bool STRICT, int MODE>
__global__ __launch_bounds__(SO_THREADS) void k_so_tile(SoStream sa, SoStream sb, uint32_t table, const uint32_t* __restrict__ part,
                                                       uint32_t* __restrict__ tile_count, const uint32_t* __restrict__ tile_off, uint32_t n_out,
                                                       int32_t* __restrict__ o_contig, int32_t* __restrict__ o_start, int32_t* __restrict__ o_end,
                                                       unsigned long long* __restrict__ tile_stats) {
    __shared__ unsigned long long keys[SO_LDS];
    __shared__ uint32_t l_scan[SO_THREADS / kWave];
    __shared__ unsigned long long l_scan64[SO_THREADS / kWave];
    const int64_t tile = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t total = sa.n + sb.n;
    const int64_t d0 = tile * SO_TILE;
    const int64_t d1 = d0 + SO_TILE < total ? d0 + SO_TILE : total;
    const int64_t i0 = part[tile], i1 = part[tile + 1];
    const int64_t j0 = d0 - i0, j1 = d1 - i1;
    const int na = (int)(i1 - i0), nb = (int)(j1 - j0), cnt = na + nb;       // cnt <= SO_TILE
    // slot 0 = the element before the piece, 1 .. len the piece, len + 1 the element behind it
    unsigned long long* sA = keys;
    unsigned long long* sB = keys + na + 2;
    for (int k = tid; k < na + 2; k += SO_THREADS) sA[k] = so_load<STRICT>(sa, i0 - 1 + k);
    for (int k = tid; k < nb + 2; k += SO_THREADS) sB[k] = so_load<STRICT>(sb, j0 - 1 + k);
    __syncthreads();

    const int diag = tid * SO_ITEMS < cnt ? tid * SO_ITEMS : cnt;
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
    const uint32_t pi = (uint32_t)i0, pj = (uint32_t)j0;                     // only the parities are used

    unsigned long long gk[SO_ITEMS];                 // key of the group that ends at item k
    uint32_t open_mask = 0, close_mask = 0;
    unsigned long long acc1 = 0, acc2 = 0, acc3 = 0, opens3 = 0;
#pragma unroll
    for (int k = 0; k < SO_ITEMS; ++k) {
        gk[k] = 0;
        if (diag + k < cnt) {
            unsigned long long K;
            bool owns;
            uint32_t before;
            if (a <= b) {
                K = a;
                before = ((pi + i) & 1u) | (((pj + j) & 1u) << 1);
                ++i; a = sA[1 + i];
                owns = b != K;                        // an equal key of stream 2 follows: the group is that event's
            } else {
                K = b;
                const uint32_t tie = sA[i] == K ? 1u : 0u;                   // stream 1's event before it, at the same position
                before = ((pi + i - tie) & 1u) | (((pj + j) & 1u) << 1);
                ++j; b = sB[1 + j];
                owns = true;
            }
            const uint32_t after = ((pi + i) & 1u) | (((pj + j) & 1u) << 1);
            if (owns) {
                if constexpr (MODE == SO_STATS) {
                    const unsigned long long pos = K & ((1ull << 33) - 1ull);
                    acc1 += (before == 1u ? pos : 0ull) - (after == 1u ? pos : 0ull);
                    acc2 += (before == 2u ? pos : 0ull) - (after == 2u ? pos : 0ull);
                    acc3 += (before == 3u ? pos : 0ull) - (after == 3u ? pos : 0ull);
                    opens3 += (after == 3u && before != 3u) ? 1ull : 0ull;
                } else {
                    const uint32_t fb = (table >> before) & 1u, fa = (table >> after) & 1u;
                    if (fb != fa) {
                        if (fa) open_mask |= 1u << k; else close_mask |= 1u << k;
                        gk[k] = K;
                    }
                }
            }
        }
    }
    if constexpr (MODE == SO_STATS) {
        unsigned long long t1, t2, t3, t4;
        block_exclusive_scan(acc1, SumOp(), 0ull, l_scan64, &t1);
        block_exclusive_scan(acc2, SumOp(), 0ull, l_scan64, &t2);
        block_exclusive_scan(acc3, SumOp(), 0ull, l_scan64, &t3);
        block_exclusive_scan(opens3, SumOp(), 0ull, l_scan64, &t4);
        if (tid == 0) {
            unsigned long long* w = tile_stats + tile * SO_STAT_WORDS;
            w[0] = t1; w[1] = t2; w[2] = t3; w[3] = t4;
        }
    } else {
        uint32_t total_open = 0;
        uint32_t r = block_exclusive_scan((uint32_t)__popc(open_mask), SumOp(), 0u, l_scan, &total_open);
        if constexpr (MODE == SO_COUNT) {
            if (tid == 0) tile_count[tile] = total_open;
        } else {
            r += tile_off[tile];
#pragma unroll
            for (int k = 0; k < SO_ITEMS; ++k) {
                const unsigned long long pos = gk[k] & ((1ull << 33) - 1ull);
                if ((close_mask & (1u << k)) && r >= 1u && r <= n_out) {   // r >= 1: a close follows the open of the boundary before it
                    __builtin_nontemporal_store(unflip((uint32_t)(pos - (STRICT ? 0ull : 1ull))), o_end + (r - 1));
                }
                if ((open_mask & (1u << k)) && r < n_out) {
                    __builtin_nontemporal_store((int32_t)(gk[k] >> 33), o_contig + r);
                    __builtin_nontemporal_store(unflip((uint32_t)pos), o_start + r);
                    ++r;
                }
            }
        }
    }
}

// out[w] = sum over the tiles of tile_stats[4 t + w], modulo 2^64: one workgroup, every thread a fixed stride of tiles
__global__ __launch_bounds__(SO_THREADS) void k_so_reduce(const unsigned long long* __restrict__ tile_stats, int64_t n_tiles,
                                                         unsigned long long* __restrict__ out) {
    __shared__ unsigned long long l_scan64[SO_THREADS / kWave];
    unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    for (int64_t t = threadIdx.x; t < n_tiles; t += SO_THREADS) {
        const unsigned long long* w = tile_stats + t * SO_STAT_WORDS;
        w0 += w[0]; w1 += w[1]; w2 += w[2]; w3 += w[3];
    }
    unsigned long long t0, t1, t2, t3;
    block_exclusive_scan(w0, SumOp(), 0ull, l_scan64, &t0);
    block_exclusive_scan(w1, SumOp(), 0ull, l_scan64, &t1);
    block_exclusive_scan(w2, SumOp(), 0ull, l_scan64, &t2);
    block_exclusive_scan(w3, SumOp(), 0ull, l_scan64, &t3);
    if (threadIdx.x == 0) { out[0] = t0; out[1] = t1; out[2] = t2; out[3] = t3; }
}

}  // namespace ivj
