// permute.hip.h -- pb.permutation_test: overlap statistics of df1 under many circular shifts, nothing per row leaves the registers.
//
// Semantics (include/ivjoin.h, DESIGN.md "Permutation test").  Half-open coordinates: hs = start - (closed ? 1 : 0), he = end; a
// contig c covers [0, L[c]).  A probe row is eligible iff its contig is in the dictionary and 0 <= hs < he <= L[c].  In permutation p
//     s' = (hs + off[p][c]) mod L,  e' = s' + (he - hs)
// and the row is the piece [s', e') when e' <= L, otherwise the two pieces [s', L) and [0, e' - L).  A piece matches a build row iff
// they share a position; build rows that cover no position never match.  Per permutation: n_pairs = matches summed over rows and
// pieces (a build row that reaches both pieces of a wrapped row counts twice), n_rows = rows with a match in any piece.
//
// The count of a piece [qs, qe) is the two-rank formula of k_count_overlaps on the joint grid,
//     #{b.start (<) qe} - #{b.end <= qs}         targets te = flip(qe) + (closed ? 1 : 0), ts = flip(qs) + 1, in 64 bits
// (e' reaches 2 L - 1 > 2^31 before it is split, and a piece's end reaches L = 2^31 - 1 plus one in the closed frame).  It is exact
// for every piece once the build rows that cover no position are kept out of both ranks: zpre_s[p] / zpre_e[p] = number of such rows
// before position p of the start / end order (k_perm_zmark + one exclusive scan each, once per call); both orders share the contig
// segments, so the counts at the segment start cancel and
//     count = (hi - zpre_s[hi]) - (r - zpre_e[r]).
// ztot[0] == 0 (no such row: the usual case) skips the two 4-byte gathers.
//
// Shape.  The probe rows arrive in (contig, start) order (the driver sorts them once per call): a circular shift keeps that order
// inside a contig up to one rotation, so the record gathers of a wavefront walk the joint grid almost sequentially in every
// permutation, and the lanes of a wavefront share their contig: the offset of a permutation is one broadcast load.
// A wavefront keeps PERM_ITEMS rows per lane in registers together with their contig's grid metadata (read once, not per
// permutation: no LDS copy of the metadata, whatever the dictionary size) and loops over the PERM_BLOCK = 64 permutations of its
// block; the wavefront's sums of permutation j end up in lane j (select, no LDS), the four wavefronts of the workgroup are folded
// through 4 KB of LDS behind one barrier and lane j writes ONE 16-byte partial {pairs, rows} for (tile, permutation).
// k_permute_fold sums the partials of a permutation over the tiles.  No atomics anywhere; the sums are integers, so the result does
// not depend on any order.  Grid = tiles x permutation blocks.
// Out-of-range values: off, L and the coordinates only ever form 64-bit targets that are compared against the grid's edges before a
// slot is computed, so no table is read out of bounds whatever they hold.
#pragma once
#include "count_nearest.hip.h"

namespace ivj {

constexpr int PERM_THREADS = 256;
constexpr int PERM_ITEMS = 4;                                    // probe rows per lane
constexpr int PERM_TILE = PERM_THREADS * PERM_ITEMS;             // probe rows per workgroup
constexpr int PERM_BLOCK = 64;                                   // permutations per workgroup: one per lane of the partial store
constexpr int PERM_CHUNK = 1024;                                 // permutations per launch at most (the driver chunks over them)
constexpr int PERM_FOLD_THREADS = 512;
static_assert(PERM_BLOCK == kWave, "lane j of a wavefront holds the sums of permutation j of the block");
static_assert(PERM_CHUNK % PERM_BLOCK == 0, "a launch is whole permutation blocks");

template <bool STRICT>
__device__ __forceinline__ bool perm_no_position(int32_t s, int32_t e) { return STRICT ? s >= e : s > e; }

// zs[p] = 1 iff the row at position p of the start order covers no position, ze[p] the same for the end order; entry n = 0
template <bool STRICT>
__global__ void k_perm_zmark(const int32_t* __restrict__ b_start, const int2* __restrict__ ep, const int32_t* __restrict__ e_end,
                             const int32_t* __restrict__ e_pos, int64_t n, uint32_t* __restrict__ zs, uint32_t* __restrict__ ze) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n) return;
    uint32_t fs = 0u, fe = 0u;
    if (p < n) {
        fs = perm_no_position<STRICT>(b_start[p], ep[p].x) ? 1u : 0u;
        const int32_t q = e_pos[p];
        fe = ((uint32_t)q < (uint32_t)n && perm_no_position<STRICT>(b_start[q], e_end[p])) ? 1u : 0u;
    }
    zs[p] = fs; ze[p] = fe;
}

// per-row constants of the permutation loop: the row and its contig's joint-grid metadata
struct PermRow {
    uint32_t hs, len, L;             // half-open start, length, contig length; len == 0: the row takes no part
    int32_t c;
    int a, b;                        // the contig's segment of the build index
    uint32_t ulo, uhi, tb;           // the grid's edges (flipped coordinates) and first slot
    int shift;
};

// matches of the piece [qs, qe) (half-open, 0 <= qs < qe <= L) among the build rows of R's contig
template <bool STRICT>
__device__ __forceinline__ long long perm_piece(const IndexView& ix, const uint32_t* __restrict__ zs, const uint32_t* __restrict__ ze,
                                                bool zany, const PermRow& R, unsigned long long qs, unsigned long long qe) {
    const unsigned long long te = qe + 0x80000000ull + (STRICT ? 0ull : 1ull);   // first start >= / > qe
    const unsigned long long ts = qs + 0x80000000ull + 1ull;                     // first end > qs
    const int he = (R.b <= R.a || te <= R.ulo) ? 0 : (te > R.uhi ? 1 : 2);
    const int hsel = (R.b <= R.a || ts <= R.ulo) ? 0 : (ts > R.uhi ? 1 : 2);
    const uint32_t de = (uint32_t)te - R.ulo, ds = (uint32_t)ts - R.ulo, bmask = (1u << R.shift) - 1u;   // shift <= 31
    const uint32_t se = he == 2 ? R.tb + (de >> R.shift) : 0u;
    const uint32_t ss = hsel == 2 ? R.tb + (ds >> R.shift) : 0u;
    const bool wide = R.shift > 16;
    int4 re = make_int4(0, 0, 0, 0), rs = make_int4(0, 0, 0, 0);
    if (he == 2) re = ix.crec[se];
    if (hsel == 2) rs = (he == 2 && se == ss) ? re : ix.crec[ss];
    const int hi = he == 0 ? R.a : (he == 1 ? R.b : joint_rank(ix.b_start, re.x, (uint32_t)re.z, de & bmask, wide, te, R.b));
    const int r = hsel == 0 ? R.a : (hsel == 1 ? R.b : joint_rank(ix.e_end, rs.y, (uint32_t)rs.w, ds & bmask, wide, ts, R.b));
    long long cnt = (long long)hi - (long long)r;
    if (zany) cnt -= (long long)zs[hi] - (long long)ze[r];
    return cnt;
}

__device__ __forceinline__ long long perm_wave_sum(long long v) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

// pc / ps / pep: the probe rows in (contig, start) order (contig, start, {end, -}); rows outside the dictionary carry a contig
// >= n_contigs.  off: the offsets of THIS launch's n_perm permutations, row-major n_perm x n_contigs.
// partial[tile * n_perm + p] = {pairs, rows} of tile `tile` in permutation p.
template <bool STRICT>
__global__ __launch_bounds__(PERM_THREADS) void k_permute(IndexView ix, const uint32_t* __restrict__ zs, const uint32_t* __restrict__ ze,
                                                          const uint32_t* __restrict__ ztot, const int32_t* __restrict__ pc,
                                                          const int32_t* __restrict__ ps, const int2* __restrict__ pep, int64_t n,
                                                          const int32_t* __restrict__ contig_len, const int32_t* __restrict__ off,
                                                          int n_perm, longlong2* __restrict__ partial) {
    __shared__ longlong2 s_part[PERM_THREADS / kWave][PERM_BLOCK];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const bool zany = ztot[0] != 0u;
    const int64_t tile = blockIdx.x;
    const int p0 = (int)blockIdx.y * PERM_BLOCK;
    const int np = (n_perm - p0) < PERM_BLOCK ? (n_perm - p0) : PERM_BLOCK;
    // row k of lane l of wavefront w: consecutive lanes hold consecutive rows (coalesced loads, neighbouring grid slots)
    PermRow R[PERM_ITEMS];
#pragma unroll
    for (int k = 0; k < PERM_ITEMS; ++k) {
        const int64_t i = tile * PERM_TILE + (int64_t)(w * PERM_ITEMS + k) * kWave + lane;
        PermRow r;
        r.hs = 0u; r.len = 0u; r.L = 1u; r.c = 0; r.a = 0; r.b = 0; r.ulo = 0u; r.uhi = 0u; r.tb = 0u; r.shift = 0;
        if (i < n) {
            const int32_t c = pc[i];
            if ((uint32_t)c < (uint32_t)ix.n_contigs) {
                const long long hs = (long long)ps[i] - (STRICT ? 0ll : 1ll), he = (long long)pep[i].x, L = (long long)contig_len[c];
                if (0ll <= hs && hs < he && he <= L) {
                    const int4 m0 = ix.cmeta_j[2 * c], m1 = ix.cmeta_j[2 * c + 1];
                    r.hs = (uint32_t)hs; r.len = (uint32_t)(he - hs); r.L = (uint32_t)L; r.c = c;
                    r.a = m0.x; r.b = m0.y; r.ulo = (uint32_t)m0.z; r.uhi = (uint32_t)m0.w; r.shift = m1.x; r.tb = (uint32_t)m1.y;
                }
            }
        }
        R[k] = r;
    }
    long long acc_pairs = 0, acc_rows = 0;                       // of permutation p0 + lane, over this wavefront's rows
#pragma unroll 1
    for (int j = 0; j < np; ++j) {
        const int32_t* offp = off + (size_t)(p0 + j) * (size_t)ix.n_contigs;
        long long pairs = 0;
        int rows = 0;
#pragma unroll
        for (int k = 0; k < PERM_ITEMS; ++k) {
            const bool live = R[k].len != 0u;
            const uint32_t o = live ? (uint32_t)offp[R[k].c] : 0u;
            unsigned long long s1 = (unsigned long long)R[k].hs + o;             // < 2 L when 0 <= off < L
            if (s1 >= R[k].L) s1 -= R[k].L;
            const unsigned long long e1 = s1 + R[k].len;
            const bool wrap = e1 > R[k].L;
            long long cnt = 0;
            if (live) cnt = perm_piece<STRICT>(ix, zs, ze, zany, R[k], s1, wrap ? (unsigned long long)R[k].L : e1);
            if (__ballot(live && wrap) != 0ull) {                                // uniform: rare, a fraction len / L of the rows
                if (live && wrap) cnt += perm_piece<STRICT>(ix, zs, ze, zany, R[k], 0ull, e1 - R[k].L);
            }
            pairs += cnt;
            rows += (int)__popcll(__ballot(cnt > 0));
        }
        pairs = perm_wave_sum(pairs);
        if (lane == j) { acc_pairs = pairs; acc_rows = rows; }
    }
    s_part[w][lane] = make_longlong2(acc_pairs, acc_rows);
    __syncthreads();
    if (w == 0 && lane < np) {
        longlong2 t = s_part[0][lane];
#pragma unroll
        for (int k = 1; k < PERM_THREADS / kWave; ++k) { const longlong2 x = s_part[k][lane]; t.x += x.x; t.y += x.y; }
        partial[(size_t)tile * (size_t)n_perm + (size_t)(p0 + lane)] = t;
    }
}

// n_pairs[p] / n_rows[p] = the partials of permutation p summed over the tiles
__global__ __launch_bounds__(PERM_FOLD_THREADS) void k_permute_fold(const longlong2* __restrict__ partial, int64_t tiles, int n_perm,
                                                                   long long* __restrict__ n_pairs, long long* __restrict__ n_rows) {
    constexpr int NW = PERM_FOLD_THREADS / kWave;
    __shared__ longlong2 s_part[NW][kWave];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const int p = (int)blockIdx.x * kWave + lane;
    longlong2 t = make_longlong2(0, 0);
    if (p < n_perm) {
#pragma unroll 4
        for (int64_t i = w; i < tiles; i += NW) { const longlong2 x = partial[(size_t)i * (size_t)n_perm + (size_t)p]; t.x += x.x; t.y += x.y; }
    }
    s_part[w][lane] = t;
    __syncthreads();
    if (w == 0 && p < n_perm) {
#pragma unroll
        for (int k = 1; k < NW; ++k) { const longlong2 x = s_part[k][lane]; t.x += x.x; t.y += x.y; }
        n_pairs[p] = t.x; n_rows[p] = t.y;
    }
}

}  // namespace ivj
