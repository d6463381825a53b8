// multi.hip.h -- N interval frames as position sets: pb.multi_intersect (the maximal runs of positions covered by the same
// non-empty set of frames, bedtools multiinter) and pb.consensus (the maximal runs covered by at least k of the N frames).
//
// Step 1 (depth.hip.h, k_depth_tile<.., RUNS = true>) turns every frame into its union runs; the run lists are concatenated and
// indexed once (host_multi.hip.h), which gives the two event streams of depth.hip.h over ALL runs:
//   A = (contig, start)   one event per run          B = (contig, end')   one event per run      (end' = the half-open end)
// Every event carries the TAG of its run's frame (k_multi_tags: the run's row in the concatenation against the F + 1 run
// offsets; the end order reaches its row through e_pos).  A frame's runs are disjoint and do not touch, so an event of frame f
// toggles bit f of the membership mask whichever stream it comes from: after any prefix of the merged sequence
//   mask = XOR over the events of the prefix of 1 << tag
// and one position holds at most ONE event of a frame (s0 < e0' < s1 < ... per frame and contig): a group of equal keys has
// at most F <= 64 events.
//
// Step 2, here: the merge-path walk of k_depth_tile with that mask as its state.  k_multi_tile_xor reduces every tile's events to
// one 64-bit word, an exclusive XOR scan of the words gives the mask in front of every tile, and inside the tile a block-wide
// exclusive XOR scan of the threads' words gives the mask in front of every thread.  Events at one position are netted first:
// only the LAST event of a group is looked at, with m_after = the mask behind it and m_before = the mask in front of the
// group's first event.  A group that began before the thread (or the tile) is repaired by walking both streams back while the
// key stays the same -- at most F steps a stream, from LDS inside the tile and from HBM in front of it.  With the class function
//   segments:  c(m) = popcount(m) >= k ? m : 0          consensus:  c(m) = popcount(m) >= k
// a group is a boundary iff c(m_after) != c(m_before); it opens a run iff c(m_after) != 0 and closes the previous one iff
// c(m_before) != 0.  The mask is 0 at the end of every contig, so opens and closes pair up and one exclusive count of the opens
// places both, as in k_depth_tile: an open writes (contig, start, mask) at its rank r, a close writes end at r - 1.
//
// Launches: k_multi_tags, k_depth_partition, k_multi_tile_xor, the XOR scan, k_multi_tile<.., FILL = false>, the scan of the
// counts, k_multi_tile<.., FILL = true>.
#pragma once
#include "depth.hip.h"

namespace ivj {

constexpr int MI_THREADS = DP_THREADS;
constexpr int MI_ITEMS = DP_ITEMS;
constexpr int MI_TILE = DP_TILE;                     // merged events per workgroup: k_depth_partition cuts the tiles
constexpr int MI_LDS = MI_TILE + 4;                  // both pieces + {before, behind} of each
constexpr int MI_MAX_FRAMES = IVJ_MAX_FRAMES;
static_assert(MI_MAX_FRAMES == 64, "the membership mask is one 64-bit word");

// tag_a[p] = frame of the run at start-order slot p, tag_e[p] = frame of the run at end-order slot p.
// run_off: F + 1 ascending offsets of the frames' runs in the concatenation (run_off[F] = n).
__global__ __launch_bounds__(256) void k_multi_tags(const int32_t* __restrict__ b_row, const int32_t* __restrict__ e_pos, int64_t n,
                                                    const uint32_t* __restrict__ run_off, int32_t n_frames, uint8_t* __restrict__ tag_a,
                                                    uint8_t* __restrict__ tag_e) {
    __shared__ uint32_t l_off[MI_MAX_FRAMES + 1];
    for (int k = threadIdx.x; k <= n_frames; k += blockDim.x) l_off[k] = run_off[k];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    auto frame_of = [&](uint32_t row) {              // the last f with run_off[f] <= row (empty frames repeat an offset)
        int lo = 0, hi = n_frames;
        while (hi - lo > 1) {
            const int m = (lo + hi) >> 1;
            if (l_off[m] <= row) lo = m; else hi = m;
        }
        return (uint8_t)lo;
    };
    tag_a[p] = frame_of((uint32_t)b_row[p]);
    const int32_t q = e_pos[p];
    tag_e[p] = ((uint32_t)q < (uint64_t)n) ? frame_of((uint32_t)b_row[q]) : (uint8_t)0;
}

// tile_x[t] = XOR of 1 << tag over the events of tile t (part: k_depth_partition's table)
__global__ __launch_bounds__(MI_THREADS) void k_multi_tile_xor(const uint8_t* __restrict__ tag_a, const uint8_t* __restrict__ tag_e, int64_t n,
                                                              const uint32_t* __restrict__ part, unsigned long long* __restrict__ tile_x) {
    __shared__ unsigned long long l_scan64[MI_THREADS / kWave];
    const int64_t tile = blockIdx.x;
    const int64_t d0 = tile * MI_TILE;
    const int64_t d1 = d0 + MI_TILE < 2 * n ? d0 + MI_TILE : 2 * n;
    const int64_t i0 = part[tile], i1 = part[tile + 1];
    const int64_t j0 = d0 - i0, j1 = d1 - i1;
    unsigned long long x = 0;
    for (int64_t k = i0 + threadIdx.x; k < i1; k += MI_THREADS) x ^= 1ull << (tag_a[k] & 63);
    for (int64_t k = j0 + threadIdx.x; k < j1; k += MI_THREADS) x ^= 1ull << (tag_e[k] & 63);
    unsigned long long tot;
    block_exclusive_scan(x, XorOp(), 0ull, l_scan64, &tot);
    if (threadIdx.x == 0) tile_x[tile] = tot;
}

template <bool CONSENSUS>
__device__ __forceinline__ unsigned long long mi_class(unsigned long long m, int32_t min_frames) {
    const bool in = __popcll(m) >= min_frames;
    if constexpr (CONSENSUS) return in ? 1ull : 0ull;
    return in ? m : 0ull;
}

// One tile of the merged sequence.  tile_mask[tile] = the membership mask in front of the tile.  FILL = false: tile_count[tile] =
// runs opened in the tile.  FILL = true: the runs are written, tile_off[tile] = runs opened before the tile, n_out = runs in all
// (no store goes past it); o_mask is written for segments only.
template <bool STRICT, bool FILL, bool CONSENSUS>
__global__ __launch_bounds__(MI_THREADS) void k_multi_tile(const int32_t* __restrict__ b_contig, const int32_t* __restrict__ b_start,
                                                          const int32_t* __restrict__ e_end, const uint8_t* __restrict__ tag_a,
                                                          const uint8_t* __restrict__ tag_e, int64_t n, int32_t n_contigs, int32_t min_frames,
                                                          const uint32_t* __restrict__ part, const unsigned long long* __restrict__ tile_mask,
                                                          uint32_t* __restrict__ tile_count, const uint32_t* __restrict__ tile_off, uint32_t n_out,
                                                          int32_t* __restrict__ o_contig, int32_t* __restrict__ o_start, int32_t* __restrict__ o_end,
                                                          unsigned long long* __restrict__ o_mask) {
    __shared__ unsigned long long keys[MI_LDS];
    __shared__ uint8_t tags[MI_LDS];
    __shared__ uint32_t l_scan[MI_THREADS / kWave];
    __shared__ unsigned long long l_scan64[MI_THREADS / kWave];
    const int64_t tile = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t d0 = tile * MI_TILE;
    const int64_t d1 = d0 + MI_TILE < 2 * n ? d0 + MI_TILE : 2 * n;
    const int64_t i0 = part[tile], i1 = part[tile + 1];
    const int64_t j0 = d0 - i0, j1 = d1 - i1;
    const int na = (int)(i1 - i0), nb = (int)(j1 - j0), cnt = na + nb;       // cnt <= MI_TILE
    // slot 0 = the element before the piece, 1 .. len the piece, len + 1 the element behind it
    unsigned long long* sA = keys;
    unsigned long long* sB = keys + na + 2;
    uint8_t* tA = tags;
    uint8_t* tB = tags + na + 2;
    for (int k = tid; k < na + 2; k += MI_THREADS) {
        const int64_t p = i0 - 1 + k;
        sA[k] = dp_load<STRICT, false>(b_contig, b_start, p, n);
        tA[k] = (p >= 0 && p < n) ? (uint8_t)(tag_a[p] & 63) : (uint8_t)0;
    }
    for (int k = tid; k < nb + 2; k += MI_THREADS) {
        const int64_t p = j0 - 1 + k;
        sB[k] = dp_load<STRICT, true>(b_contig, e_end, p, n);
        tB[k] = (p >= 0 && p < n) ? (uint8_t)(tag_e[p] & 63) : (uint8_t)0;
    }
    __syncthreads();

    const int diag = tid * MI_ITEMS < cnt ? tid * MI_ITEMS : cnt;
    int i, j;
    {
        int lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (sA[1 + m] <= sB[diag - m]) lo = m + 1; else hi = m;          // sB[1 + (diag - 1 - m)]
        }
        i = lo; j = diag - lo;
    }
    const int is = i, js = j;                                               // where this thread's piece begins
    unsigned long long a = sA[1 + i], b = sB[1 + j];
    const unsigned long long K0 = a <= b ? a : b;                           // key of the thread's first event

    unsigned long long gk[MI_ITEMS];                 // key of the group that ends at item k
    unsigned long long rel[MI_ITEMS];                // XOR of the thread's events up to and including item k
    uint32_t ends = 0;                               // bit k: item k is the last event of its group
    unsigned long long x = 0;
#pragma unroll
    for (int k = 0; k < MI_ITEMS; ++k) {
        gk[k] = 0; rel[k] = 0;
        if (diag + k < cnt) {
            unsigned long long K;
            if (a <= b) { K = a; x ^= 1ull << tA[1 + i]; ++i; a = sA[1 + i]; }
            else { K = b; x ^= 1ull << tB[1 + j]; ++j; b = sB[1 + j]; }
            const unsigned long long next = a <= b ? a : b;
            if (next != K) ends |= 1u << k;
            gk[k] = K; rel[k] = x;
        }
    }
    unsigned long long tile_x;
    const unsigned long long prefix = tile_mask[tile] ^ block_exclusive_scan(x, XorOp(), 0ull, l_scan64, &tile_x);

    // the mask in front of the group the thread's first event belongs to: the events of that group before the thread are taken
    // out again, stream by stream (each holds at most one event of a frame at a key: at most MI_MAX_FRAMES steps)
    unsigned long long mb = prefix;
    if (diag < cnt) {
        int64_t p = i0 + is - 1;
        for (int step = 0; step < MI_MAX_FRAMES && p >= 0; ++step, --p) {
            const bool in_lds = p >= i0 - 1;
            const unsigned long long K = in_lds ? sA[p - i0 + 1] : dp_load<STRICT, false>(b_contig, b_start, p, n);
            if (K != K0) break;
            mb ^= 1ull << (in_lds ? tA[p - i0 + 1] : (uint8_t)(tag_a[p] & 63));
        }
        p = j0 + js - 1;
        for (int step = 0; step < MI_MAX_FRAMES && p >= 0; ++step, --p) {
            const bool in_lds = p >= j0 - 1;
            const unsigned long long K = in_lds ? sB[p - j0 + 1] : dp_load<STRICT, true>(b_contig, e_end, p, n);
            if (K != K0) break;
            mb ^= 1ull << (in_lds ? tB[p - j0 + 1] : (uint8_t)(tag_e[p] & 63));
        }
    }

    uint32_t open_mask = 0, close_mask = 0;
#pragma unroll
    for (int k = 0; k < MI_ITEMS; ++k) {
        if (ends & (1u << k)) {
            const unsigned long long ma = prefix ^ rel[k];
            const unsigned long long cb = mi_class<CONSENSUS>(mb, min_frames), ca = mi_class<CONSENSUS>(ma, min_frames);
            const bool live = ca != cb && (uint32_t)(gk[k] >> 33) < (uint32_t)n_contigs;
            if (live && ca != 0) open_mask |= 1u << k;
            if (live && cb != 0) close_mask |= 1u << k;
            mb = ma;
        }
    }
    uint32_t total = 0;
    uint32_t r = block_exclusive_scan((uint32_t)__popc(open_mask), SumOp(), 0u, l_scan, &total);
    if constexpr (!FILL) {
        if (tid == 0) tile_count[tile] = total;
    } else {
        r += tile_off[tile];
#pragma unroll
        for (int k = 0; k < MI_ITEMS; ++k) {
            const unsigned long long pos = gk[k] & ((1ull << 33) - 1ull);
            if ((close_mask & (1u << k)) && r >= 1u && r <= n_out) {       // r >= 1: a close follows the open of the boundary before it
                __builtin_nontemporal_store(unflip((uint32_t)(pos - (STRICT ? 0ull : 1ull))), o_end + (r - 1));
            }
            if ((open_mask & (1u << k)) && r < n_out) {
                __builtin_nontemporal_store((int32_t)(gk[k] >> 33), o_contig + r);
                __builtin_nontemporal_store(unflip((uint32_t)pos), o_start + r);
                if constexpr (!CONSENSUS) __builtin_nontemporal_store(prefix ^ rel[k], o_mask + r);
                ++r;
            }
        }
    }
}

}  // namespace ivj
