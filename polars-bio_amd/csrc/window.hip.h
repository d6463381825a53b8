// window.hip.h -- pb.window / pb.count_window: every build (df2) row within a distance of every probe (df1) row, with the distance
// (bedtools window -w / -l / -r / -sw, pyranges join(slack=), bioframe pair_by_distance).  A candidate-test join on the plan of
// thresh.hip.h (the walk of cand_walk.hip.h); the tables of build_flat (flat.hip.h) are read-only here.
//
// For a probe row a and a build row b of one contig, everything in 64 bits ((<) is < for 0-based half-open frames, STRICT, and <=
// for 1-based closed ones, WEAK):
//     gap_right = b.start - a.end        gap_left = a.start - b.end
//     d(a, b)   = 0 if b.start (<) a.end && a.start (<) b.end (the rows overlap), else max(gap_right, gap_left)
// A row that does not overlap a lies AFTER it when !(b.start (<) a.end) and BEFORE it when !(a.start (<) b.end); two rows that both
// cover a position are never both.  With the probe's extents L(a), R(a) in [0, 2^32 - 1] the pair is kept iff
//     both rows cover a position  &&  d >= min_distance  &&  (overlap || (after && d <= R(a)) || (before && d <= L(a)))
// The reported distance is signed: negative when b lies before a, 0 on overlap; |d| <= 2^32 - 1 (int32 coordinates).
//
// THE RANGE.  A kept pair has
//     b.start <= a.end + R(a)       (overlap: b.start (<) a.end;  after: gap_right = d <= R;  before: b.start (<) a.end as the rows
//                                    of a non-overlapping pair lie on one side only)
//     b.end   >= a.start - L(a)     (the mirror)
// flat_range<STRICT>(qs, qe) returns a superset [lo', hi') of the rows with  b.start (<) qe  and  qs (<) prefix-max(b.end).  So the
// extended probe is
//     STRICT   qe = a.end + R + 1,  qs = a.start - L - 1          (b.start <= x  <=>  b.start < x + 1)
//     WEAK     qe = a.end + R,      qs = a.start - L
// formed in 64 bits and then CLAMPED to int32.  The clamp leaves a superset of the matches: qe only clamps down to INT32_MAX and qs
// only up to INT32_MIN (extents are >= 0).  WEAK: b.start <= INT32_MAX and INT32_MIN <= b.end hold for every int32 row, nothing is
// cut.  STRICT: the rows cut are those with b.start >= INT32_MAX, resp. with prefix-max(b.end) <= INT32_MIN, hence b.end =
// INT32_MIN; a half-open row with start = INT32_MAX or end = INT32_MIN has start >= end, covers no position and never pairs.
// The range is NOT narrowed by min_distance.  Probes that cover no position have no candidates.
//
// THE WALK is that of cand_walk.hip.h with the sub-range test loop, as in k_overlap_thresh: WIN_TILE probes per workgroup, one lane
// per candidate on its 16-byte rec4 record.  Ranges of any length: the chunks simply go on (a contig-wide build row keeps every
// range of its contig open); no hand-over to another kernel.
//
// Forms of one kernel (FORM):
//   WIN_COUNT  per-tile totals (their exclusive scan places the tiles' output ranges) and, when asked, per-probe int64 counts
//              written at the probe's position in the caller's columns;
//   WIN_PAIRS  the matches of a tile in flat candidate order at the tile's base: the pairs of one probe are contiguous and ordered
//              by (build.start, build row), tiles follow in launch order -- identical from run to run;
//   WIN_DIST   WIN_PAIRS plus the signed int64 distance of every pair.
// No global atomics on the result path.
//
// LDS.  Per probe: lo, off, {start, end}, L, R and one word that is the match counter (count form) or the row id to report (emit
// forms): 28 bytes x 512 = 14 KB.  Per chunk: the 16-bit marks (4 KB) and the staged build rows (8 KB), as in ThreshLds; WIN_DIST
// stages the 32-bit MAGNITUDE of the distance (8 KB) -- not the int64 (16 KB) -- and keeps the sign in bit 15 of the staged mark (a
// probe index needs 9 bits).  WIN_COUNT / WIN_PAIRS: 26 720 bytes, WIN_DIST: 34 896 bytes per workgroup; four resident workgroups
// of the largest form take 139 584 of the CU's 163 840 bytes, so __launch_bounds__(256, 4) holds for all three.
#pragma once
#include "flat.hip.h"

namespace ivj {

// The kernel's geometry under its own names, by value (the tests size their cases by them): the shared walk's.
constexpr int WIN_THREADS = 256;
constexpr int WIN_ITEMS = 2;
constexpr int WIN_TILE = WIN_THREADS * WIN_ITEMS;         // probes per workgroup
constexpr int WIN_CH = 2048;                              // candidates per chunk
static_assert(WIN_THREADS == WALK_THREADS && WIN_ITEMS == WALK_ITEMS && WIN_CH == WALK_CH, "the geometry of cand_walk.hip.h");
constexpr int WIN_COUNT = 0, WIN_PAIRS = 1, WIN_DIST = 2;
constexpr uint32_t WIN_SIGN = 0x8000u;                    // staged mark: the build row lies before the probe
static_assert(WIN_TILE < (int)WIN_SIGN, "probe index + 1 must leave bit 15 of the 16-bit marks free");

// the extended probe of the header comment, clamped to int32
template <bool STRICT>
__device__ __forceinline__ void window_probe(int32_t s, int32_t e, uint32_t left, uint32_t right, int32_t& qs, int32_t& qe) {
    const long long lo = (long long)s - (long long)left - (STRICT ? 1ll : 0ll);
    const long long hi = (long long)e + (long long)right + (STRICT ? 1ll : 0ll);
    qs = lo < (long long)INT32_MIN ? INT32_MIN : (int32_t)lo;          // lo <= s: never above INT32_MAX
    qe = hi > (long long)INT32_MAX ? INT32_MAX : (int32_t)hi;          // hi >= e: never below INT32_MIN
}

// the predicate, as written in the header comment (the probe is known to cover a position); mag = |d|, before = its sign
template <bool STRICT>
__device__ __forceinline__ bool window_match(int32_t as, int32_t ae, int32_t bs, int32_t be, uint32_t left, uint32_t right,
                                             uint32_t min_distance, uint32_t& mag, bool& before) {
    const bool covers = STRICT ? bs < be : bs <= be;
    const bool not_after = lt_op<STRICT>(bs, ae), not_before = lt_op<STRICT>(as, be);
    const bool ov = not_after && not_before;
    const long long gr = (long long)bs - (long long)ae, gl = (long long)as - (long long)be;
    const long long d = ov ? 0ll : (gr > gl ? gr : gl);
    before = !ov && !not_before;
    mag = (uint32_t)d;                                    // 0 <= d <= 2^32 - 1 wherever the pair is kept
    const bool near = ov || (!not_after ? d <= (long long)right : (!not_before && d <= (long long)left));
    return covers && near && d >= (long long)min_distance;
}

template <int FORM>
struct WindowLds {
    int lo[WIN_TILE];                 // first candidate position of the probe
    uint32_t off[WIN_TILE];           // tile-local offset of its first candidate, modulo 2^32
    int2 q[WIN_TILE];                 // {start, end} of the probe itself (not the extended one)
    uint32_t left[WIN_TILE];          // L(a)
    uint32_t right[WIN_TILE];         // R(a)
    uint32_t cr[WIN_TILE];            // count form: matches of the probe; emit forms: the row id to report
    __align__(16) uint16_t marks[WIN_CH];
    int32_t st_b[WIN_CH];
    uint32_t st_d[FORM == WIN_DIST ? WIN_CH : 1];
    int scan_i[WALK_WAVES];
    long long scan_ll[WALK_WAVES];
    long long wtot[WALK_WAVES];
};
static_assert(sizeof(WindowLds<WIN_DIST>) * 4 <= 160 * 1024, "four resident workgroups per CU");

// One chunk of nC <= WIN_CH candidates starting at tile-local candidate offset c0: the candidate -> probe map (walk_marks), then
// wavefront w tests the candidates of its sub-range (walk_sub) with the distance predicate.  Emit forms: the matches of a wavefront
// are staged at st_b / st_d / marks[wb + rank] for walk_emit_chunk; bit 15 of the staged mark = the sign of the distance.  COUNTS:
// per-probe counts into L.cr (walk_count_heads).  Returns the number of matches of this wavefront.
template <bool STRICT, int FORM, bool COUNTS>
__device__ __forceinline__ int window_chunk(const IndexView& ix, uint32_t min_distance, long long c0, int nC,
                                            const long long (&off)[WIN_ITEMS], const int (&cn)[WIN_ITEMS], WindowLds<FORM>& L) {
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
        const uint32_t el = L.left[at.q], er = L.right[at.q];
        int4 v = make_int4(0, 0, 0, 0);                    // {start, end, build row, -}
        if (valid) v = ix.rec4[at.p];
        uint32_t mag = 0;
        bool before = false;
        const bool m = valid && window_match<STRICT>(qq.x, qq.y, v.x, v.y, el, er, min_distance, mag, before);
        const unsigned long long mm = __ballot(m);
        if (COUNTS) walk_count_heads(L.cr, at.q, valid, mm);
        if (FORM != WIN_COUNT && m) {
            const int r = sub.wb + cnt + (int)__popcll(mm & lt_lanes);
            L.st_b[r] = v.z;
            if (FORM == WIN_DIST) L.st_d[r] = mag;
            L.marks[r] = (uint16_t)((uint32_t)at.q | (before ? WIN_SIGN : 0u));
        }
        cnt += (int)__popcll(mm);
    }
    return cnt;
}

// pos (NULL: identity) = the probe's position in the caller's columns when the probes were bucketed: probe_left / probe_right and
// the per-probe counts are indexed by it; row_id (NULL: the position) = the id the emit forms report.  probe_left / probe_right
// (NULL: the scalar left / right) = the extents of every probe row.
// count form: tile_tot[tile] = matches of the tile (NULL: not wanted), counts[position] = matches of the probe (NULL: not wanted).
// emit forms: tile_tot = the exclusive scan of the count form's totals; the tile's pairs go to out_*[tile_tot[tile] ...].
template <bool STRICT, int FORM>
__global__ __launch_bounds__(WIN_THREADS, 4) void k_window(IndexView ix, const int32_t* __restrict__ pc, const int32_t* __restrict__ ps,
                                                          const int32_t* __restrict__ pe, const int32_t* __restrict__ pos,
                                                          const int32_t* __restrict__ row_id, int64_t n, bool vec_ok, uint32_t left,
                                                          uint32_t right, const uint32_t* __restrict__ probe_left,
                                                          const uint32_t* __restrict__ probe_right, uint32_t min_distance,
                                                          long long* __restrict__ tile_tot, long long* __restrict__ counts,
                                                          int32_t* __restrict__ out_probe, int32_t* __restrict__ out_build,
                                                          long long* __restrict__ out_dist) {
    __shared__ WindowLds<FORM> L;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const long long ntiles = (n + WIN_TILE - 1) / WIN_TILE;
    const long long tile = xcd_tile64(blockIdx.x, ntiles);
    if (tile >= ntiles) return;                            // uniform
    const int64_t i0 = (int64_t)tile * WIN_TILE + (int64_t)threadIdx.x * WIN_ITEMS;
    int32_t c[WIN_ITEMS], s[WIN_ITEMS], e[WIN_ITEMS], at[WIN_ITEMS];
    load_probe_items(pc, ps, pe, pos, i0, n, vec_ok, c, s, e, at);
    int lo[WIN_ITEMS], cn[WIN_ITEMS];
#pragma unroll
    for (int k = 0; k < WIN_ITEMS; ++k) {
        const bool valid = i0 + k < n;
        uint32_t el = left, er = right;
        if (valid && probe_left) el = probe_left[at[k]];
        if (valid && probe_right) er = probe_right[at[k]];
        // a probe that covers no position has no candidates
        const bool can = valid && (STRICT ? s[k] < e[k] : s[k] <= e[k]);
        int32_t qs, qe;
        window_probe<STRICT>(s[k], e[k], el, er, qs, qe);
        flat_range<STRICT>(ix, c[k], qs, qe, can, lo[k], cn[k]);
        const int q = threadIdx.x * WIN_ITEMS + k;
        L.lo[q] = lo[k]; L.q[q] = make_int2(s[k], e[k]); L.left[q] = el; L.right[q] = er;
        if (FORM == WIN_COUNT) L.cr[q] = 0u;
        else L.cr[q] = (uint32_t)((valid && row_id) ? row_id[at[k]] : at[k]);
    }
    long long T;
    long long off[WIN_ITEMS];
    walk_offsets(cn, L.scan_ll, off, T);
#pragma unroll
    for (int k = 0; k < WIN_ITEMS; ++k) L.off[threadIdx.x * WIN_ITEMS + k] = (uint32_t)off[k];
    // (the first barrier of walk_marks publishes the LDS arrays)
    if constexpr (FORM != WIN_COUNT) {
        if (T == 0) return;                                // uniform
        long long running = tile_tot[tile];
        for (long long c0 = 0; c0 < T; c0 += WIN_CH) {
            const int nC = walk_chunk_len(T, c0);
            const int cnt = window_chunk<STRICT, FORM, false>(ix, min_distance, c0, nC, off, cn, L);
            running += walk_emit_chunk(L.wtot, cnt, nC, [&](int slot, long long o) {
                const uint32_t mk = L.marks[slot];
                __builtin_nontemporal_store((int32_t)L.cr[mk & (WIN_SIGN - 1u)], out_probe + running + o);
                __builtin_nontemporal_store(L.st_b[slot], out_build + running + o);
                if constexpr (FORM == WIN_DIST) {
                    const long long d = (long long)L.st_d[slot];
                    __builtin_nontemporal_store((mk & WIN_SIGN) ? -d : d, out_dist + running + o);
                }
            });
        }
        return;
    } else {
        long long wcnt = 0;                                // matches of this wavefront over the whole tile
        for (long long c0 = 0; c0 < T; c0 += WIN_CH) {
            const int nC = walk_chunk_len(T, c0);
            if (counts) wcnt += window_chunk<STRICT, WIN_COUNT, true>(ix, min_distance, c0, nC, off, cn, L);
            else wcnt += window_chunk<STRICT, WIN_COUNT, false>(ix, min_distance, c0, nC, off, cn, L);
        }
        if (lane == 0) L.wtot[w] = wcnt;
        __syncthreads();                                   // ... and the LDS counters are complete
        if (tile_tot && threadIdx.x == 0) {
            long long tot = 0;
#pragma unroll
            for (int k = 0; k < WALK_WAVES; ++k) tot += L.wtot[k];
            tile_tot[tile] = tot;
        }
        if (counts) {
#pragma unroll
            for (int k = 0; k < WIN_ITEMS; ++k)
                if (i0 + k < n) counts[at[k]] = (long long)L.cr[threadIdx.x * WIN_ITEMS + k];
        }
    }
}

}  // namespace ivj
