// signal.hip.h -- pb.signal_summary / pb.signal_profile: the build side (df2) read as a SIGNAL TRACK, (contig, start, end, value)
// rows as in a bedGraph, where a row weighs its value on every position it covers.  Per probe, over the build rows b of its contig,
//     ov(b)  = min(q.end, b.end) - max(q.start, b.start)   (+ 1 for closed frames), 64-bit
//     b contributes  iff  ov(b) >= max(1, min_overlap, probe_min, build_min[b])  and its value is valid
//     bases  = sum of ov(b)            uint64, wrapping
//     sum    = sum of value(b) * ov(b) int64 columns: the product and the sum modulo 2^64; double columns: one rounding per
//                                      product ((double)ov is exact up to 2^32), then the additions of the walk
//     min / max over the contributing values, unweighted; mean = sum / bases
// -- bigWigAverageOverBed's covered / sum / mean, deepTools computeMatrix per bin.  Rows of either side that cover no position
// share nothing (ov <= 0): this is the thresholded predicate of thresh.hip.h with an effective minimum of 1, NOT the plain
// count_overlaps predicate of the unthresholded map_overlaps.
//
// Both kernels are oagg_tile<.., WEIGHTED = true> of overlap_agg.hip.h: the same candidate walk, segmented scan, edge parts folded
// in candidate order after the chunk barrier, chunking, LDS block (OaggLds) and k_oagg_gather; no atomics, integer results
// identical from run to run, a double sum bit for bit for the same rows in the same order.  They differ in the probe source:
//
//   k_overlap_wagg     OaggRows: the caller's probe columns (bucketed or not), as k_overlap_agg.
//   k_signal_profile   OaggBins: probe g of the grid is bin j = g % n_bins of window row = g / n_bins, made in registers from the
//                      12 bytes of the window (+ its reverse byte) exactly as depth_profile.hip.h derives bin edges: flipped 33-bit
//                      positions, xs = flip(start), L = flip(end) + w - xs (w = 0 Strict / 1 Weak; none when <= 0),
//                      x_j = xs + floor(j L / n_bins) in 64 bits, bin j = [x_j, x_{j+1}).  The bin reaches flat_range and the
//                      predicate as an int32 interval in the frame's own convention -- (unflip(x_j), unflip(x_{j+1})) Strict,
//                      (unflip(x_j), unflip(x_{j+1} - 1)) Weak, both representable whenever the bin is non-empty -- and an empty
//                      bin as a probe without a contig, which has no candidates.  Its result goes to row n_bins + (reverse[row] ?
//                      n_bins - 1 - j : j).  No bin frame exists in HBM.
//
// What bounds them: one 16-byte record, 8 value bytes, 1 validity byte, one predicate and one scan step per CANDIDATE -- per
// candidate of every BIN for the profile, so a build row that spans k bins is visited k times (and the loose range of flat_range
// adds about one row per bin).  That suits signal tracks of short rows; a track of contig-wide rows makes every bin walk them all.
#pragma once
#include "overlap_agg.hip.h"
#include "depth_profile.hip.h"

namespace ivj {

// The bins of n windows as probes.  n_total = n * n_bins; a tile's first probe is split into (row, bin) with one 64-bit division,
// uniform, and the lanes go on in 32 bits (bin + tile offset < 4096 + 512).
template <bool STRICT>
struct OaggBins {
    using At = int64_t;
    const int32_t *wc, *ws, *we;
    const uint8_t* reverse;
    int64_t n_total;
    uint32_t n_bins;
    __device__ __forceinline__ int64_t count() const { return n_total; }
    __device__ __forceinline__ void load(int64_t i0, int32_t (&c)[THRESH_ITEMS], int32_t (&s)[THRESH_ITEMS], int32_t (&e)[THRESH_ITEMS],
                                         At (&at)[THRESH_ITEMS]) const {
        const uint32_t B = n_bins;
        const int64_t g0 = i0 - (int64_t)threadIdx.x * THRESH_ITEMS;                 // the tile's first probe
        const int64_t row0 = g0 / (int64_t)B;
        const uint32_t j0 = (uint32_t)(g0 % (int64_t)B);
#pragma unroll
        for (int k = 0; k < THRESH_ITEMS; ++k) {
            c[k] = -1; s[k] = 0; e[k] = 0; at[k] = 0;
            if (i0 + k >= n_total) continue;
            const uint32_t o = j0 + (uint32_t)threadIdx.x * THRESH_ITEMS + (uint32_t)k;
            const int64_t row = row0 + (int64_t)(o / B);
            const uint32_t j = o % B;
            const bool rev = reverse != nullptr && reverse[row] != 0;
            at[k] = row * (int64_t)B + (int64_t)(rev ? B - 1u - j : j);
            const unsigned long long xs = (unsigned long long)flip(ws[row]);
            const unsigned long long xe = (unsigned long long)flip(we[row]) + (STRICT ? 0ull : 1ull);
            const unsigned long long len = xe > xs ? xe - xs : 0ull;
            const unsigned long long x0 = xs + (unsigned long long)j * len / B;          // j L < 2^13 x 2^32
            const unsigned long long x1 = xs + (unsigned long long)(j + 1u) * len / B;   // <= xe
            if (x0 >= x1) continue;                                                      // an empty bin: no contig, no candidates
            c[k] = wc[row];
            s[k] = unflip((uint32_t)x0);
            e[k] = unflip((uint32_t)(STRICT ? x1 : x1 - 1ull));
        }
    }
};

template <bool STRICT, int DTYPE>
__global__ __launch_bounds__(THRESH_THREADS, 3) void k_overlap_wagg(IndexView ix, const int32_t* __restrict__ pc, const int32_t* __restrict__ ps,
                                                                    const int32_t* __restrict__ pe, const int32_t* __restrict__ pos, int64_t n,
                                                                    bool vec_ok, uint32_t min_overlap, const uint32_t* __restrict__ probe_min,
                                                                    const uint32_t* __restrict__ bm_sorted,
                                                                    const typename std::conditional<DTYPE == 0, long long, double>::type* __restrict__ vals_sorted,
                                                                    const uint8_t* __restrict__ ok_sorted,
                                                                    AggOut<typename std::conditional<DTYPE == 0, long long, double>::type> out) {
    using V = typename std::conditional<DTYPE == 0, long long, double>::type;
    __shared__ OaggLds<V> L;
    const OaggRows src{pc, ps, pe, pos, n, vec_ok};
    oagg_tile<STRICT, true, true, V>(ix, src, min_overlap, probe_min, bm_sorted, vals_sorted, ok_sorted, out, L);
}

// out.* hold n * n_bins elements, row-major; 1 <= n_bins <= DPROF_MAX_BINS (the host checks it)
template <bool STRICT, int DTYPE>
__global__ __launch_bounds__(THRESH_THREADS, 3) void k_signal_profile(IndexView ix, const int32_t* __restrict__ wc, const int32_t* __restrict__ ws,
                                                                      const int32_t* __restrict__ we, const uint8_t* __restrict__ reverse,
                                                                      int64_t n, int n_bins,
                                                                      const typename std::conditional<DTYPE == 0, long long, double>::type* __restrict__ vals_sorted,
                                                                      const uint8_t* __restrict__ ok_sorted,
                                                                      AggOut<typename std::conditional<DTYPE == 0, long long, double>::type> out) {
    using V = typename std::conditional<DTYPE == 0, long long, double>::type;
    __shared__ OaggLds<V> L;
    const OaggBins<STRICT> src{wc, ws, we, reverse, n * (int64_t)n_bins, (uint32_t)n_bins};
    oagg_tile<STRICT, true, true, V>(ix, src, 0u, nullptr, nullptr, vals_sorted, ok_sorted, out, L);
}

}  // namespace ivj
