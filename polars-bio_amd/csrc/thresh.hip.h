// thresh.hip.h -- pb.overlap / pb.count_overlaps with overlap thresholds (min_overlap, min_frac1, min_frac2): a candidate-test
// join on the plan of flat.hip.h.
//
// For a probe row a and a build row b of one contig
//     ov(a, b) = min(a.end, b.end) - max(a.start, b.start)   (+ 1 for 1-based closed frames, WEAK)
// and the pair is kept iff
//     ov >= max(1, min_overlap, probe_min[a], build_min[b])                      (64-bit; 0 = no requirement, 0xffffffff = never)
// The fractions never reach the device: the front door turns min_frac1 / min_frac2 into the per-row minimum base counts
// probe_min / build_min (include/ivjoin.h).
//
// Every kept pair has ov >= 1, hence passes the plain predicate b.start (<) a.end && a.start (<) b.end, hence lies inside the
// LOOSE candidate range [lo', hi') that flat_range reads from tab2 with two table reads (flat.hip.h; the tables of build_flat,
// read-only).  The range is that of the UNSHRUNK probe: it is NOT tightened by the minima (a probe shrunk by m > len / 2 inverts,
// and the range of the plain probe is a superset whatever the minima are).  The only candidates left out are those of probes that
// cannot match at all: rows that cover no position and rows whose own minimum is "never".  Every lane tests one candidate on its
// 16-byte rec4 record plus -- when build minima were given -- the 4-byte minimum of the same sorted position (build_min permuted into index order once per call by
// k_thresh_gather: nothing is gathered by row per candidate).
//
// Ranges of any length: the tile's candidates are walked as cand_walk.hip.h describes, with the sub-range test loop; a probe's range
// may span any number of chunks (a contig-wide build row keeps the range of every probe of the contig open down to that row:
// there is no second path to fall back to, the chunks simply go on).
//
// Two forms of one kernel:
//   count (EMIT = false)  per-tile totals (the exclusive scan of which places the tiles' output ranges) and, when asked, per-probe
//                         counts (int64, written at the probe's position in the caller's columns = count_overlaps with thresholds);
//   emit  (EMIT = true)   the matches of a tile in flat candidate order at the tile's base: the pairs of one probe are contiguous
//                         and ordered by (build.start, build row), the tiles follow each other in launch order -- the output is
//                         identical from run to run.
// What bounds it: one 16-byte (20 with build minima) read and one predicate per candidate, i.e. the number of candidates, not of
// matches; a threshold removes pairs from the output, never candidates from the test.
#pragma once
#include "flat.hip.h"

namespace ivj {

// The geometry of this kernel and of those built on ThreshLds (overlap_agg, overlap_quant, signal) under the family's own names,
// by value: the tests size their cases by them.  It is the shared walk's, which holds the asserts on it.
constexpr int THRESH_THREADS = 256;
constexpr int THRESH_ITEMS = 2;
constexpr int THRESH_TILE = THRESH_THREADS * THRESH_ITEMS;   // probes per workgroup
constexpr int THRESH_CH = 2048;                              // candidates per chunk
constexpr uint32_t THRESH_NEVER = 0xffffffffu;
static_assert(THRESH_THREADS == WALK_THREADS && THRESH_ITEMS == WALK_ITEMS && THRESH_CH == WALK_CH, "the geometry of cand_walk.hip.h");

// m_sorted[p] = m[b_row[p]]: the build-side minima in index order
__global__ void k_thresh_gather(const int32_t* __restrict__ b_row, const uint32_t* __restrict__ m, int64_t n_index, int64_t n_rows,
                                uint32_t* __restrict__ m_sorted) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_index) return;
    const int32_t r = b_row[p];
    m_sorted[p] = (r >= 0 && (int64_t)r < n_rows) ? m[r] : THRESH_NEVER;
}

// the predicate, as written in the header comment
template <bool STRICT>
__device__ __forceinline__ bool thresh_match(int32_t as, int32_t ae, int32_t bs, int32_t be, uint32_t thr) {
    const long long lo = as > bs ? as : bs, hi = ae < be ? ae : be;
    const long long ov = hi - lo + (STRICT ? 0ll : 1ll);
    const long long need = thr > 1u ? (long long)thr : 1ll;
    return thr != THRESH_NEVER && ov >= need;
}

// a probe's minimum raised to the build row's (bm_sorted NULL: no build minima), and the predicate of a candidate-test kernel
// with and without thresholds: the plain form is b.start (<) q.end && q.start (<) b.end as written.  qq = the probe's {start, end},
// v = the candidate's rec4 record at sorted position p.
__device__ __forceinline__ uint32_t cand_thr(uint32_t thr, const uint32_t* __restrict__ bm_sorted, int p) {
    if (bm_sorted) { const uint32_t bm = bm_sorted[p]; thr = thr > bm ? thr : bm; }
    return thr;
}
template <bool STRICT, bool THRESH>
__device__ __forceinline__ bool cand_match(const int2 qq, const int4 v, uint32_t thr, const uint32_t* __restrict__ bm_sorted, int p) {
    if (THRESH) return thresh_match<STRICT>(qq.x, qq.y, v.x, v.y, cand_thr(thr, bm_sorted, p));
    return lt_op<STRICT>(v.x, qq.y) && lt_op<STRICT>(qq.x, v.y);
}

struct ThreshLds {
    int lo[THRESH_TILE];              // first candidate position of the probe
    uint32_t off[THRESH_TILE];        // tile-local offset of its first candidate, modulo 2^32
    int2 q[THRESH_TILE];              // {start, end}
    uint32_t thr[THRESH_TILE];        // max(min_overlap, probe_min[row])
    uint32_t cnt[THRESH_TILE];        // count form: matches of the probe
    int32_t row[THRESH_TILE];         // emit form: the row id to report
    __align__(16) uint16_t marks[THRESH_CH];
    int32_t st_b[THRESH_CH];
    int scan_i[WALK_WAVES];
    long long scan_ll[WALK_WAVES];
    long long wtot[WALK_WAVES];
};

// One chunk of nC <= THRESH_CH candidates starting at tile-local candidate offset c0: the candidate -> probe map (walk_marks), then
// wavefront w tests the candidates of its sub-range (walk_sub).  EMIT: the matches of a wavefront are staged at st_b / marks[wb + rank]
// for walk_emit_chunk.  COUNTS: per-probe counts into L.cnt (walk_count_heads).  Returns the number of matches of this wavefront.
template <bool STRICT, bool EMIT, bool COUNTS>
__device__ __forceinline__ int thresh_chunk(const IndexView& ix, const uint32_t* __restrict__ bm_sorted, long long c0, int nC,
                                            const long long (&off)[THRESH_ITEMS], const int (&cn)[THRESH_ITEMS], ThreshLds& L) {
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned long long lt_lanes = (1ull << lane) - 1ull;
    walk_marks(L.marks, L.scan_i, c0, nC, off, cn);
    const WalkSub sub = walk_sub(nC);
    const uint32_t c0lo = (uint32_t)c0;
    int cnt = 0;
    for (int i0 = sub.wb; i0 < sub.we; i0 += kWave) {
        const int i = i0 + lane;
        const bool valid = i < sub.we;
        const WalkAt at = walk_probe(L.lo, L.off, L.marks, i, c0lo, valid);
        const int2 qq = L.q[at.q];
        const uint32_t thr = L.thr[at.q];
        int4 v = make_int4(0, 0, 0, 0);                    // {start, end, build row, -}
        if (valid) v = ix.rec4[at.p];
        const bool m = valid && cand_match<STRICT, true>(qq, v, thr, bm_sorted, at.p);
        const unsigned long long mm = __ballot(m);
        if (COUNTS) walk_count_heads(L.cnt, at.q, valid, mm);
        if (EMIT && m) {
            const int r = sub.wb + cnt + (int)__popcll(mm & lt_lanes);
            L.st_b[r] = v.z;
            L.marks[r] = (uint16_t)at.q;
        }
        cnt += (int)__popcll(mm);
    }
    return cnt;
}

// pos (NULL: identity) = the probe's position in the caller's columns when the probes were bucketed: probe_min and the per-probe
// counts are indexed by it; row_id (NULL: the position) = the id the emit form reports.
// count form: tile_tot[tile] = matches of the tile (NULL: not wanted), counts[position] = matches of the probe (NULL: not wanted).
// emit form: tile_tot = the exclusive scan of the count form's totals; the tile's pairs go to out_*[tile_tot[tile] ...].
template <bool STRICT, bool EMIT>
__global__ __launch_bounds__(THRESH_THREADS, 4) void k_overlap_thresh(IndexView ix, const int32_t* __restrict__ pc, const int32_t* __restrict__ ps,
                                                                      const int32_t* __restrict__ pe, const int32_t* __restrict__ pos,
                                                                      const int32_t* __restrict__ row_id, int64_t n, bool vec_ok,
                                                                      uint32_t min_overlap, const uint32_t* __restrict__ probe_min,
                                                                      const uint32_t* __restrict__ bm_sorted, long long* __restrict__ tile_tot,
                                                                      long long* __restrict__ counts, int32_t* __restrict__ out_probe,
                                                                      int32_t* __restrict__ out_build) {
    __shared__ ThreshLds L;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const long long ntiles = (n + THRESH_TILE - 1) / THRESH_TILE;
    const long long tile = xcd_tile64(blockIdx.x, ntiles);
    if (tile >= ntiles) return;                            // uniform
    const int64_t i0 = (int64_t)tile * THRESH_TILE + (int64_t)threadIdx.x * THRESH_ITEMS;
    int32_t c[THRESH_ITEMS], s[THRESH_ITEMS], e[THRESH_ITEMS], at[THRESH_ITEMS];
    load_probe_items(pc, ps, pe, pos, i0, n, vec_ok, c, s, e, at);
    int lo[THRESH_ITEMS], cn[THRESH_ITEMS];
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k) {
        const bool valid = i0 + k < n;
        uint32_t thr = min_overlap;
        if (valid && probe_min) { const uint32_t pm = probe_min[at[k]]; thr = thr > pm ? thr : pm; }
        // a probe that covers no position, or whose own minimum is "never", has no candidates
        const bool can = valid && thr != THRESH_NEVER && (STRICT ? s[k] < e[k] : s[k] <= e[k]);
        flat_range<STRICT>(ix, c[k], s[k], e[k], can, lo[k], cn[k]);
        const int q = threadIdx.x * THRESH_ITEMS + k;
        L.lo[q] = lo[k]; L.q[q] = make_int2(s[k], e[k]); L.thr[q] = thr;
        if (!EMIT) L.cnt[q] = 0u;
        if (EMIT) L.row[q] = (valid && row_id) ? row_id[at[k]] : at[k];
    }
    long long T;
    long long off[THRESH_ITEMS];
    walk_offsets(cn, L.scan_ll, off, T);
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k) L.off[threadIdx.x * THRESH_ITEMS + k] = (uint32_t)off[k];
    // (the first barrier of walk_marks publishes the LDS arrays)
    if (EMIT) {
        if (T == 0) return;                                // uniform
        long long running = tile_tot[tile];
        for (long long c0 = 0; c0 < T; c0 += THRESH_CH) {
            const int nC = walk_chunk_len(T, c0);
            const int cnt = thresh_chunk<STRICT, true, false>(ix, bm_sorted, c0, nC, off, cn, L);
            running += walk_emit_chunk(L.wtot, cnt, nC, [&](int slot, long long o) {
                __builtin_nontemporal_store(L.row[L.marks[slot]], out_probe + running + o);
                __builtin_nontemporal_store(L.st_b[slot], out_build + running + o);
            });
        }
        return;
    }
    long long wcnt = 0;                                    // matches of this wavefront over the whole tile
    for (long long c0 = 0; c0 < T; c0 += THRESH_CH) {
        const int nC = walk_chunk_len(T, c0);
        if (counts) wcnt += thresh_chunk<STRICT, false, true>(ix, bm_sorted, c0, nC, off, cn, L);
        else wcnt += thresh_chunk<STRICT, false, false>(ix, bm_sorted, c0, nC, off, cn, L);
    }
    if (lane == 0) L.wtot[w] = wcnt;
    __syncthreads();                                       // ... and the LDS counters are complete
    if (tile_tot && threadIdx.x == 0) {
        long long tot = 0;
#pragma unroll
        for (int k = 0; k < WALK_WAVES; ++k) tot += L.wtot[k];
        tile_tot[tile] = tot;
    }
    if (counts) {
#pragma unroll
        for (int k = 0; k < THRESH_ITEMS; ++k)
            if (i0 + k < n) counts[at[k]] = (long long)L.cnt[threadIdx.x * THRESH_ITEMS + k];
    }
}

}  // namespace ivj
