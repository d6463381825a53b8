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
// cannot match at all: rows that cover no position and rows whose own minimum is "never".  The candidates of a tile of probes are
// laid out flat (exclusive scan of the range lengths) and every lane tests one candidate on its 16-byte rec4 record plus -- when
// build minima were given -- the 4-byte minimum of the same sorted position (build_min permuted into index order once per call by
// k_thresh_gather: nothing is gathered by row per candidate).
//
// Ranges of any length: a tile walks its flat candidate space in chunks of THRESH_CH; a probe's range may span any number of
// chunks (a contig-wide build row keeps the range of every probe of the contig open down to that row: there is no second path to
// fall back to, the chunks simply go on).  Tile-local candidate offsets are kept modulo 2^32 in LDS: the index of a candidate
// inside its probe's range (< 2^30 build rows) is exact under that arithmetic however many candidates the tile has.
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

constexpr int THRESH_THREADS = 256;
constexpr int THRESH_ITEMS = 2;
constexpr int THRESH_TILE = THRESH_THREADS * THRESH_ITEMS;   // probes per workgroup
constexpr int THRESH_CH = 2048;                              // candidates per chunk (one 16-byte mark vector per thread)
constexpr uint32_t THRESH_NEVER = 0xffffffffu;
static_assert(THRESH_CH * 2 == THRESH_THREADS * 16, "one uint4 of marks per thread");
static_assert(THRESH_TILE < 65535, "probe index + 1 must fit the 16-bit marks");
static_assert(THRESH_THREADS == SCAN_THREADS, "block_exclusive_scan is written for SCAN_THREADS");

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

struct ThreshLds {
    int lo[THRESH_TILE];              // first candidate position of the probe
    uint32_t off[THRESH_TILE];        // tile-local offset of its first candidate, modulo 2^32
    int2 q[THRESH_TILE];              // {start, end}
    uint32_t thr[THRESH_TILE];        // max(min_overlap, probe_min[row])
    uint32_t cnt[THRESH_TILE];        // count form: matches of the probe
    int32_t row[THRESH_TILE];         // emit form: the row id to report
    __align__(16) uint16_t marks[THRESH_CH];
    int32_t st_b[THRESH_CH];
    int scan_i[THRESH_THREADS / kWave];
    long long scan_ll[THRESH_THREADS / kWave];
    long long wtot[THRESH_THREADS / kWave];
};

// One chunk of nC <= THRESH_CH candidates starting at tile-local candidate offset c0.  Builds the candidate -> probe map (marks:
// probe index + 1 at the probe's first candidate of the chunk, max-scanned), then wavefront w tests the candidates
// [w * per, (w + 1) * per).  EMIT: the matches of a wavefront are staged at st_b / marks[w * per + rank] (marks recycled as the probe
// index of the staged pair: rank <= index, and the lanes of a step have read their marks before any of them writes).  COUNTS: the
// matches of one probe inside a step are consecutive lanes; the first of them adds their number to the probe's LDS counter.
// Returns the number of matches of this wavefront.
template <bool STRICT, bool EMIT, bool COUNTS>
__device__ __forceinline__ int thresh_chunk(const IndexView& ix, const uint32_t* __restrict__ bm_sorted, long long c0, int nC,
                                            const long long (&off)[THRESH_ITEMS], const int (&cn)[THRESH_ITEMS], ThreshLds& L) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const unsigned long long lt_lanes = (1ull << lane) - 1ull;
    const int per = ((nC + THRESH_THREADS - 1) / THRESH_THREADS) * kWave;
    uint4* marks4 = reinterpret_cast<uint4*>(L.marks);
    __syncthreads();                                       // the previous chunk is done with marks / st_b
    marks4[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k) {
        if (cn[k] == 0) continue;
        const long long rel = off[k] - c0;
        if (rel >= 0 && rel < (long long)nC) L.marks[rel] = (uint16_t)(threadIdx.x * THRESH_ITEMS + k + 1);
        else if (rel < 0 && rel + cn[k] > 0) L.marks[0] = (uint16_t)(threadIdx.x * THRESH_ITEMS + k + 1);
    }
    __syncthreads();
    {
        uint4 v = marks4[threadIdx.x];
        uint32_t wd[4] = {v.x, v.y, v.z, v.w};
        uint32_t tmax = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = wd[j] & 0xffffu, b = wd[j] >> 16;
            tmax = tmax > a ? tmax : a;
            tmax = tmax > b ? tmax : b;
        }
        int tot;
        uint32_t run = (uint32_t)block_exclusive_scan((int)tmax, MaxOp(), 0, L.scan_i, &tot);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = wd[j] & 0xffffu, b = wd[j] >> 16;
            run = run > a ? run : a;
            const uint32_t na = run;
            run = run > b ? run : b;
            wd[j] = na | (run << 16);
        }
        marks4[threadIdx.x] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
    __syncthreads();
    const int wb = w * per;
    const int we = (wb + per) < nC ? (wb + per) : nC;
    const uint32_t c0lo = (uint32_t)c0;
    int cnt = 0;
    for (int i0 = wb; i0 < we; i0 += kWave) {
        const int i = i0 + lane;
        const bool valid = i < we;
        int q = valid ? (int)L.marks[i] - 1 : 0;
        q = q < 0 ? 0 : q;                                 // (every candidate of a chunk lies at or after a mark)
        const int lo = L.lo[q];
        const uint32_t of = L.off[q];
        const int2 qq = L.q[q];
        uint32_t thr = L.thr[q];
        const int p = lo + (int)(c0lo + (uint32_t)i - of);
        int4 v = make_int4(0, 0, 0, 0);                    // {start, end, build row, -}
        if (valid) {
            v = ix.rec4[p];
            if (bm_sorted) { const uint32_t bm = bm_sorted[p]; thr = thr > bm ? thr : bm; }
        }
        const bool m = valid && thresh_match<STRICT>(qq.x, qq.y, v.x, v.y, thr);
        const unsigned long long mm = __ballot(m);
        if (COUNTS && mm != 0ull) {                        // uniform
            const int qseg = valid ? q : -1;
            const int qprev = __shfl_up(qseg, 1, kWave);
            const bool head = lane == 0 || qprev != qseg;
            const unsigned long long hb = __ballot(head);
            if (head && valid) {
                const unsigned long long above = hb & ~((2ull << lane) - 1ull);   // the heads after this one
                const unsigned long long upto = above ? ((above & (0ull - above)) - 1ull) : ~0ull;
                const int c = (int)__popcll(mm & upto & ~lt_lanes);
                if (c) atomicAdd(&L.cnt[q], (uint32_t)c);
            }
        }
        if (EMIT && m) {
            const int r = wb + cnt + (int)__popcll(mm & lt_lanes);
            L.st_b[r] = v.z;
            L.marks[r] = (uint16_t)q;
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
    load_items_nt(pc, i0, n, vec_ok, -1, c);
    load_items_nt(ps, i0, n, vec_ok, 0, s);
    load_items_nt(pe, i0, n, vec_ok, 0, e);
    if (pos) load_items(pos, i0, n, vec_ok, 0, at);
    else {
#pragma unroll
        for (int k = 0; k < THRESH_ITEMS; ++k) at[k] = (int32_t)(i0 + k);
    }
    int lo[THRESH_ITEMS], cn[THRESH_ITEMS];
    long long tsum = 0;
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k) {
        const bool valid = i0 + k < n;
        uint32_t thr = min_overlap;
        if (valid && probe_min) { const uint32_t pm = probe_min[at[k]]; thr = thr > pm ? thr : pm; }
        // a probe that covers no position, or whose own minimum is "never", has no candidates
        const bool can = valid && thr != THRESH_NEVER && (STRICT ? s[k] < e[k] : s[k] <= e[k]);
        flat_range<STRICT>(ix, c[k], s[k], e[k], can, lo[k], cn[k]);
        tsum += cn[k];
        const int q = threadIdx.x * THRESH_ITEMS + k;
        L.lo[q] = lo[k]; L.q[q] = make_int2(s[k], e[k]); L.thr[q] = thr;
        if (!EMIT) L.cnt[q] = 0u;
        if (EMIT) L.row[q] = (valid && row_id) ? row_id[at[k]] : at[k];
    }
    long long T;
    long long off[THRESH_ITEMS];
    off[0] = block_exclusive_scan(tsum, SumOp(), 0ll, L.scan_ll, &T);
#pragma unroll
    for (int k = 1; k < THRESH_ITEMS; ++k) off[k] = off[k - 1] + cn[k - 1];
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k) L.off[threadIdx.x * THRESH_ITEMS + k] = (uint32_t)off[k];
    // (the first barrier inside thresh_chunk publishes the LDS arrays)
    if (EMIT) {
        if (T == 0) return;                                // uniform
        long long running = tile_tot[tile];
        for (long long c0 = 0; c0 < T; c0 += THRESH_CH) {
            const int nC = (int)((T - c0) < (long long)THRESH_CH ? (T - c0) : (long long)THRESH_CH);
            const int cnt = thresh_chunk<STRICT, true, false>(ix, bm_sorted, c0, nC, off, cn, L);
            if (lane == 0) L.wtot[w] = cnt;                // (readers of the previous values have passed a barrier inside thresh_chunk)
            __syncthreads();
            long long cpre = 0, ctot = 0;
#pragma unroll
            for (int k = 0; k < THRESH_THREADS / kWave; ++k) { const long long x = L.wtot[k]; if (k < w) cpre += x; ctot += x; }
            const int wb = w * (((nC + THRESH_THREADS - 1) / THRESH_THREADS) * kWave);
            for (int j = lane; j < cnt; j += kWave) {
                __builtin_nontemporal_store(L.row[L.marks[wb + j]], out_probe + running + cpre + j);
                __builtin_nontemporal_store(L.st_b[wb + j], out_build + running + cpre + j);
            }
            running += ctot;
        }
        return;
    }
    long long wcnt = 0;                                    // matches of this wavefront over the whole tile
    for (long long c0 = 0; c0 < T; c0 += THRESH_CH) {
        const int nC = (int)((T - c0) < (long long)THRESH_CH ? (T - c0) : (long long)THRESH_CH);
        if (counts) wcnt += thresh_chunk<STRICT, false, true>(ix, bm_sorted, c0, nC, off, cn, L);
        else wcnt += thresh_chunk<STRICT, false, false>(ix, bm_sorted, c0, nC, off, cn, L);
    }
    if (lane == 0) L.wtot[w] = wcnt;
    __syncthreads();                                       // ... and the LDS counters are complete
    if (tile_tot && threadIdx.x == 0) {
        long long tot = 0;
#pragma unroll
        for (int k = 0; k < THRESH_THREADS / kWave; ++k) tot += L.wtot[k];
        tile_tot[tile] = tot;
    }
    if (counts) {
#pragma unroll
        for (int k = 0; k < THRESH_ITEMS; ++k)
            if (i0 + k < n) counts[at[k]] = (long long)L.cnt[threadIdx.x * THRESH_ITEMS + k];
    }
}

}  // namespace ivj
