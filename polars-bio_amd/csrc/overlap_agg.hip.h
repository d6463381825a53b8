// overlap_agg.hip.h -- pb.map_overlaps: count / sum / min / max / mean of a build-side (df2) value column over the build rows that
// match each probe (df1) row (bedtools map -c/-o).  The candidate walk of thresh.hip.h with the reduction of merge_agg.hip.h in place
// of the population count: no pair is written anywhere.
//
//   k_oagg_gather   once per call and column: vals_sorted[p] = values[b_row[p]] and one validity byte per sorted position (a row
//                   outside [0, n_values) is invalid).  A candidate then costs its 16-byte rec4 record, 8 consecutive value bytes and
//                   1 validity byte (+ 4 bytes with build minima): nothing is gathered by row per candidate.
//   k_overlap_agg   the tile geometry of k_overlap_thresh: THRESH_TILE probes per workgroup, their loose candidate ranges (flat_range,
//                   never tightened, no FLAT_MAX_CAND hand-over) laid out flat and walked in chunks of THRESH_CH; wavefront w tests the
//                   sub-range [w * per, (w + 1) * per) of a chunk in ascending steps of 64, one candidate per lane.
//
// The reduction.  A lane's state is that of its candidate when it matches and its value is valid, the identity otherwise.  A
// segmented inclusive scan over the wavefront, keyed on the candidate's probe, gives every segment's fold for the step; the segment
// open at the end of a step is carried into the next step in registers (the wavefront walks ascending).  A segment that begins and
// ends strictly inside the wavefront's sub-range has that wavefront as its only writer in this chunk: the lane that ends it folds it
// into the probe's LDS accumulator acc[q] with a plain read-modify-write.  The at most two segments that contain the sub-range's
// first or last candidate go to edge[w][0 / 1] with their probe index; after the chunk's barrier one thread folds these <= 8 parts
// into acc in ascending (wavefront, slot) order, which is candidate order.  A probe that spans chunks accumulates chunk by chunk.
// No atomics, no thread loops over one probe's candidates.  Given the index's sorted order every fold has one fixed shape, so
// integer results are identical from run to run and a double sum repeats bit for bit for the same rows in the same order on the
// same library build (the ABI comment of ivj_overlap_agg).
//
// Which probes get an empty range: with thresholds (THRESH) rows that cover no position or whose own minimum is "never", as in
// k_overlap_thresh; without, none but the rows flat_range itself rejects (outside the dictionary, empty contig) -- the plain
// predicate is evaluated as written, so a row that covers no position counts what count_overlaps counts for it.
// What bounds it: one record, one predicate and one scan step per CANDIDATE, not per match, and one sweep per value column.
//
// Two template arguments serve signal.hip.h (pb.signal_summary / pb.signal_profile) and leave the forms above as they were:
// WEIGHTED makes a candidate contribute its value times the positions it shares with the probe (oagg_add_w) instead of its value
// once, and the probe source Src (OaggRows here: the caller's probe columns) says where a tile's probes come from and where
// their results go.
#pragma once
#include "thresh.hip.h"
#include "merge_agg.hip.h"

namespace ivj {

constexpr int OAGG_WAVES = THRESH_THREADS / kWave;

// vals_sorted[p] = values[b_row[p]] (8-byte elements of either type), ok_sorted[p] = the value may be used
__global__ void k_oagg_gather(const int32_t* __restrict__ b_row, const unsigned long long* __restrict__ values,
                              const uint8_t* __restrict__ valid, int64_t n_index, int64_t n_values,
                              unsigned long long* __restrict__ vals_sorted, uint8_t* __restrict__ ok_sorted) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_index) return;
    const int64_t r = (int64_t)b_row[p];
    const bool ok = (uint64_t)r < (uint64_t)n_values && (!valid || valid[r]);
    vals_sorted[p] = ok ? values[r] : 0ull;
    ok_sorted[p] = ok ? 1 : 0;
}

template <class S>
__device__ __forceinline__ S oagg_bcast(const S& s, int src) {
    S o;
    o.cnt = __shfl(s.cnt, src, kWave); o.sum = __shfl(s.sum, src, kWave);
    o.mn = __shfl(s.mn, src, kWave); o.mx = __shfl(s.mx, src, kWave);
    return o;
}

// positions a probe (qs, qe) shares with a build row (bs, be), as thresh_match computes them: <= 0 = none
template <bool STRICT>
__device__ __forceinline__ long long oagg_ov(int32_t qs, int32_t qe, int32_t bs, int32_t be) {
    const long long lo = qs > bs ? qs : bs, hi = qe < be ? qe : be;
    return hi - lo + (STRICT ? 0ll : 1ll);
}

// the weighted contribution of one candidate, 1 <= ov <= 2^32: cnt holds the shared positions (uint64 arithmetic, wrapping), sum
// the value times ov -- int64 columns as a uint64 product, i.e. modulo 2^64; double columns as one correctly rounded product
// ((double)ov is exact; __dmul_rn keeps it from being contracted into the additions that follow) -- min / max the bare value
__device__ __forceinline__ void oagg_add_w(AggState<long long>& s, long long v, unsigned long long ov) {
    s.cnt = (long long)((unsigned long long)s.cnt + ov);
    s.sum += (unsigned long long)v * ov;
    s.mn = v < s.mn ? v : s.mn; s.mx = v > s.mx ? v : s.mx;
}
__device__ __forceinline__ void oagg_add_w(AggState<double>& s, double v, unsigned long long ov) {
    s.cnt = (long long)((unsigned long long)s.cnt + ov);
    s.sum += __dmul_rn(v, (double)ov);
    s.mn = fmin(s.mn, v); s.mx = fmax(s.mx, v);
}

template <class V> struct OaggLds {
    ThreshLds T;
    AggState<V> acc[THRESH_TILE];
    AggState<V> edge[OAGG_WAVES][2];
    int edge_q[OAGG_WAVES][2];                             // probe index of the part, -1 = none
};

// One chunk of nC <= THRESH_CH candidates starting at tile-local candidate offset c0: the candidate -> probe map of thresh_chunk
// (marks: probe index + 1 at the probe's first candidate of the chunk, max-scanned), then the walk described above.
template <bool STRICT, bool THRESH, bool WEIGHTED, class V>
__device__ __forceinline__ void oagg_chunk(const IndexView& ix, const uint32_t* __restrict__ bm_sorted, const V* __restrict__ vals_sorted,
                                           const uint8_t* __restrict__ ok_sorted, long long c0, int nC, const long long (&off)[THRESH_ITEMS],
                                           const int (&cn)[THRESH_ITEMS], OaggLds<V>& L) {
    using S = AggState<V>;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const int per = ((nC + THRESH_THREADS - 1) / THRESH_THREADS) * kWave;
    uint16_t* marks = L.T.marks;
    uint4* marks4 = reinterpret_cast<uint4*>(marks);
    __syncthreads();                                       // the previous chunk is done with marks, acc and edge
    marks4[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    if (lane < 2) L.edge_q[w][lane] = -1;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k) {
        if (cn[k] == 0) continue;
        const long long rel = off[k] - c0;
        if (rel >= 0 && rel < (long long)nC) marks[rel] = (uint16_t)(threadIdx.x * THRESH_ITEMS + k + 1);
        else if (rel < 0 && rel + cn[k] > 0) marks[0] = (uint16_t)(threadIdx.x * THRESH_ITEMS + k + 1);
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
        uint32_t run = (uint32_t)block_exclusive_scan((int)tmax, MaxOp(), 0, L.T.scan_i, &tot);
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
    if (wb < we) {                                         // uniform per wavefront (no barrier inside)
        const uint32_t c0lo = (uint32_t)c0;
        // (every candidate of a chunk lies at or after a mark: marks[i] >= 1 for i < nC)
        const int q_first = (int)marks[wb] - 1, q_last = (int)marks[we - 1] - 1;
        S carry = S::identity();                           // the segment open at the end of the previous step, from its start in this sub-range
        bool carry_live = false;
        for (int i0 = wb; i0 < we; i0 += kWave) {
            const int i = i0 + lane;
            const bool valid = i < we;
            int q = valid ? (int)marks[i] - 1 : 0;
            q = q < 0 ? 0 : q;
            const int q_prev = (valid && i > wb) ? (int)marks[i - 1] - 1 : -1;
            const int q_next = (valid && i + 1 < we) ? (int)marks[i + 1] - 1 : -1;
            const bool starts = valid && q_prev != q;      // the probe's first candidate inside this sub-range
            const bool ends = valid && q_next != q;        // ... and its last
            const int lo = L.T.lo[q];
            const uint32_t of = L.T.off[q];
            const int2 qq = L.T.q[q];
            const int p = lo + (int)(c0lo + (uint32_t)i - of);
            bool m = false;
            unsigned long long ov = 0ull;                  // WEIGHTED: the positions shared with the probe
            if (valid) {
                const int4 v = ix.rec4[p];                 // {start, end, build row, -}
                if (WEIGHTED) {                            // the thresholded predicate with its ov kept: contributes iff ov >= max(1, minima)
                    uint32_t thr = L.T.thr[q];
                    if (bm_sorted) { const uint32_t bm = bm_sorted[p]; thr = thr > bm ? thr : bm; }
                    const long long o = oagg_ov<STRICT>(qq.x, qq.y, v.x, v.y);
                    m = thr != THRESH_NEVER && o >= (thr > 1u ? (long long)thr : 1ll);
                    ov = (unsigned long long)o;
                } else if (THRESH) {
                    uint32_t thr = L.T.thr[q];
                    if (bm_sorted) { const uint32_t bm = bm_sorted[p]; thr = thr > bm ? thr : bm; }
                    m = thresh_match<STRICT>(qq.x, qq.y, v.x, v.y, thr);
                } else {
                    m = lt_op<STRICT>(v.x, qq.y) && lt_op<STRICT>(qq.x, v.y);
                }
                if (m) m = ok_sorted[p] != 0;
            }
            if (__ballot(m) == 0ull && !carry_live) continue;  // uniform: every state of the step is the identity and nothing is carried
            S inc = S::identity();
            if (m) {
                if (WEIGHTED) oagg_add_w(inc, vals_sorted[p], ov);
                else inc.add(vals_sorted[p]);
            }
            // inclusive segmented scan: (a, b) -> (b.head ? b : a + b, a.head | b.head); a lane before the step's first start keeps
            // head == 0 and holds the fold from lane 0 on, which continues the carried segment
            int inc_head = starts ? 1 : 0;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const S o = magg_shfl_up(inc, d);
                const int oh = __shfl_up(inc_head, d, kWave);
                if (lane >= d) {
                    if (!inc_head) inc = S::merge(o, inc);
                    inc_head |= oh;
                }
            }
            if (!inc_head) inc = S::merge(carry, inc);
            if (ends) {
                if (q == q_first) { L.edge[w][0] = inc; L.edge_q[w][0] = q; }
                else if (q == q_last) { L.edge[w][1] = inc; L.edge_q[w][1] = q; }
                else L.acc[q] = S::merge(L.acc[q], inc);   // this wavefront is the segment's only writer in this chunk
            }
            const S last = oagg_bcast(inc, kWave - 1);
            carry_live = __shfl((valid && !ends) ? 1 : 0, kWave - 1, kWave) != 0;   // (the sub-range's last candidate always ends)
            carry = carry_live ? last : S::identity();
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < OAGG_WAVES; ++k) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int q = L.edge_q[k][s];
                if (q >= 0) L.acc[q] = S::merge(L.acc[q], L.edge[k][s]);
            }
        }
    }
    // (the barrier that opens the next chunk, or the one before the outputs are written, publishes acc)
}

// Probe source of k_overlap_agg: the caller's probe columns.  pos (NULL: identity) = the probe's position in the caller's columns
// when the probes were bucketed: probe_min is read and the results are written there.  A source hands a thread its THRESH_ITEMS
// consecutive probes from i0 on as (contig, start, end) in the frame's own convention -- contig -1 for a probe that has none or
// can match nothing -- and the output element of each.
struct OaggRows {
    using At = int32_t;
    const int32_t *pc, *ps, *pe, *pos;
    int64_t n;
    bool vec_ok;
    __device__ __forceinline__ int64_t count() const { return n; }
    __device__ __forceinline__ void load(int64_t i0, int32_t (&c)[THRESH_ITEMS], int32_t (&s)[THRESH_ITEMS], int32_t (&e)[THRESH_ITEMS],
                                         At (&at)[THRESH_ITEMS]) const {
        load_items_nt(pc, i0, n, vec_ok, -1, c);
        load_items_nt(ps, i0, n, vec_ok, 0, s);
        load_items_nt(pe, i0, n, vec_ok, 0, e);
        if (pos) load_items(pos, i0, n, vec_ok, 0, at);
        else {
#pragma unroll
            for (int k = 0; k < THRESH_ITEMS; ++k) at[k] = (int32_t)(i0 + k);
        }
    }
};

// One tile of THRESH_TILE probes of `src`: ranges, the chunk walk, the outputs.  min_overlap / probe_min / bm_sorted are read by the
// THRESH form only (WEIGHTED implies it: an effective minimum of 1).
template <bool STRICT, bool THRESH, bool WEIGHTED, class V, class Src>
__device__ __forceinline__ void oagg_tile(const IndexView& ix, const Src& src, uint32_t min_overlap, const uint32_t* __restrict__ probe_min,
                                          const uint32_t* __restrict__ bm_sorted, const V* __restrict__ vals_sorted,
                                          const uint8_t* __restrict__ ok_sorted, const AggOut<V>& out, OaggLds<V>& L) {
    static_assert(THRESH || !WEIGHTED, "the weighted form is a thresholded form");
    using S = AggState<V>;
    const int64_t n = src.count();
    const long long ntiles = (n + THRESH_TILE - 1) / THRESH_TILE;
    const long long tile = xcd_tile64(blockIdx.x, ntiles);
    if (tile >= ntiles) return;                            // uniform
    const int64_t i0 = (int64_t)tile * THRESH_TILE + (int64_t)threadIdx.x * THRESH_ITEMS;
    int32_t c[THRESH_ITEMS], s[THRESH_ITEMS], e[THRESH_ITEMS];
    typename Src::At at[THRESH_ITEMS];
    src.load(i0, c, s, e, at);
    int lo[THRESH_ITEMS], cn[THRESH_ITEMS];
    long long tsum = 0;
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k) {
        const bool valid = i0 + k < n;
        uint32_t thr = THRESH ? min_overlap : 0u;
        if (THRESH && valid && probe_min) { const uint32_t pm = probe_min[at[k]]; thr = thr > pm ? thr : pm; }
        const bool can = THRESH ? (valid && thr != THRESH_NEVER && (STRICT ? s[k] < e[k] : s[k] <= e[k])) : valid;
        flat_range<STRICT>(ix, c[k], s[k], e[k], can, lo[k], cn[k]);
        tsum += cn[k];
        const int q = threadIdx.x * THRESH_ITEMS + k;
        L.T.lo[q] = lo[k]; L.T.q[q] = make_int2(s[k], e[k]); L.T.thr[q] = thr;
        L.acc[q] = S::identity();
    }
    long long T;
    long long off[THRESH_ITEMS];
    off[0] = block_exclusive_scan(tsum, SumOp(), 0ll, L.T.scan_ll, &T);
#pragma unroll
    for (int k = 1; k < THRESH_ITEMS; ++k) off[k] = off[k - 1] + cn[k - 1];
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k) L.T.off[threadIdx.x * THRESH_ITEMS + k] = (uint32_t)off[k];
    // (the first barrier inside oagg_chunk publishes the LDS arrays)
    for (long long c0 = 0; c0 < T; c0 += THRESH_CH) {
        const int nC = (int)((T - c0) < (long long)THRESH_CH ? (T - c0) : (long long)THRESH_CH);
        oagg_chunk<STRICT, THRESH, WEIGHTED, V>(ix, bm_sorted, vals_sorted, ok_sorted, c0, nC, off, cn, L);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k)
        if (i0 + k < n) magg_write(out, (int64_t)at[k], L.acc[threadIdx.x * THRESH_ITEMS + k]);
}

template <bool STRICT, bool THRESH, int DTYPE>
__global__ __launch_bounds__(THRESH_THREADS, 3) void k_overlap_agg(IndexView ix, const int32_t* __restrict__ pc, const int32_t* __restrict__ ps,
                                                                   const int32_t* __restrict__ pe, const int32_t* __restrict__ pos, int64_t n,
                                                                   bool vec_ok, uint32_t min_overlap, const uint32_t* __restrict__ probe_min,
                                                                   const uint32_t* __restrict__ bm_sorted,
                                                                   const typename std::conditional<DTYPE == 0, long long, double>::type* __restrict__ vals_sorted,
                                                                   const uint8_t* __restrict__ ok_sorted,
                                                                   AggOut<typename std::conditional<DTYPE == 0, long long, double>::type> out) {
    using V = typename std::conditional<DTYPE == 0, long long, double>::type;
    __shared__ OaggLds<V> L;
    const OaggRows src{pc, ps, pe, pos, n, vec_ok};
    oagg_tile<STRICT, THRESH, false, V>(ix, src, min_overlap, probe_min, bm_sorted, vals_sorted, ok_sorted, out, L);
}

}  // namespace ivj
