// depth_query.hip.h -- pb.depth_summary: per probe row the deepest pile of build rows under it (max_depth) and, per requested
// threshold T, the number of its positions that at least T build rows cover (bases_ge[T]) -- range queries over the depth blocks.
//
// The depth blocks of the build side (depth.hip.h) are disjoint and sorted per contig, so a block's position in the start order, its
// position in the end order and its block number coincide.  For a probe with first position s and last position e' (Strict [s, e):
// e' = e - 1, Weak [s, e]: e' = e) on contig segment [a, b) of the BLOCK index
//   i0 = a + blocks that end at or before s  (Strict: bend <= s, Weak: bend < s)  = rank of ts in e_end
//   i1 = a + blocks that start at or before e' (Strict: bstart < e, Weak: bstart <= e) = rank of te in b_start
// with the targets ts / te of k_count_overlaps: both ranks come from the joint grid (joint_rank), one or two 16-byte record gathers.
// The probe touches exactly the blocks [i0, i1) (none when i1 <= i0: a gap, an empty probe, a contig without blocks).
//
//   bases_ge[k] = P[i1][k] - P[i0][k] - (depth[i0] >= T_k ? max(0, s - bstart[i0]) : 0) - (depth[i1-1] >= T_k ? max(0, bend[i1-1] - e) : 0)
//   max_depth   = max depth over [i0, i1)
// P = exclusive 64-bit prefix sums over the blocks of (depth >= T_k ? length : 0), blocks + 1 entries, INTERLEAVED: KPAD uint64 per
// entry (KPAD = the threshold count rounded up to 1, 2, 4 or 8), so one endpoint reads all its values from one aligned fetch of at
// most 64 bytes.  A block's length is end - start (Strict) / end - start + 1 (Weak) in 64 bits; the two clips have the same form in
// both modes (the positions of block i0 below s, the positions of block i1 - 1 above e').  brec = one 16-byte record per block
// {start, end, depth, 0}: each clip is one gather.  The sums are uint64 with wrap-around; the true values are below 2^63.
//
// The maximum is a range maximum over a 16-ary tree of block maxima in the layout of hier_shape (index_view.hip.h): level 0 = the
// depths, level l entry i = max over the blocks [i << 4l, (i + 1) << 4l), pads = 0 (a depth is >= 1).  range_max16 takes the
// canonical decomposition: per level the partial 16-block at either end (at most 15 entries each, one 64-byte line each), the rest
// one level up.  [i0, i1) lies inside one contig by construction: the walk carries no contig test.  A probe that touches at most two
// blocks -- the usual case -- has both depths in the two block records it gathered for the clips and reads no tree line at all.
//
// Requests per probe (thresholds given): the probe's three column loads, one or two joint-grid records, two prefix rows, two block
// records; a probe over three or more blocks adds one or two tree lines per level it crosses.
#pragma once
#include "count_nearest.hip.h"

namespace ivj {

constexpr int DQ_MAX_T = 8;                       // = IVJ_MAX_THRESHOLDS
constexpr int DQ_TILES_PER_WG = 4;
struct DqThresholds { int32_t t[DQ_MAX_T]; };     // entries past the given ones: INT32_MAX (their columns are never stored)

// block records and level 0 of the tree (padded to whole 16-blocks with 0)
__global__ __launch_bounds__(256) void k_dq_records(const int32_t* __restrict__ bs, const int32_t* __restrict__ be, const int32_t* __restrict__ bd,
                                                    int64_t nb, int64_t padded, int4* __restrict__ rec, int32_t* __restrict__ level0) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= padded) return;
    const int32_t d = i < nb ? bd[i] : 0;
    level0[i] = d;
    if (i < nb) rec[i] = make_int4(bs[i], be[i], d, 0);
}

// one level of the tree from the level below: dst[i] = max of src[16 i .. 16 i + 15], entries at or past n_src count 0
__global__ __launch_bounds__(256) void k_dq_tree_level(const int32_t* __restrict__ src, int64_t n_src, int32_t* __restrict__ dst, int64_t padded) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= padded) return;
    int32_t m = 0;
    for (int t = 0; t < 16; ++t) {
        if (i * 16 + t < n_src) { const int32_t x = src[i * 16 + t]; m = x > m ? x : m; }
    }
    dst[i] = m;
}

// planar[k * stride + i] = depth[i] >= T_k ? length of block i : 0, entry nb = 0 (the exclusive scan leaves the grand total there)
template <bool STRICT>
__global__ __launch_bounds__(256) void k_dq_lengths(const int32_t* __restrict__ bs, const int32_t* __restrict__ be, const int32_t* __restrict__ bd,
                                                    int64_t nb, DqThresholds thr, int n_thr, size_t stride, long long* __restrict__ planar) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > nb) return;
    long long len = 0;
    int32_t d = 0;
    if (i < nb) { len = (long long)be[i] - (long long)bs[i] + (STRICT ? 0ll : 1ll); d = bd[i]; }
#pragma unroll
    for (int k = 0; k < DQ_MAX_T; ++k)
        if (k < n_thr) planar[(size_t)k * stride + (size_t)i] = d >= thr.t[k] ? len : 0ll;
}

// the scanned planar columns -> one row of KPAD uint64 per entry (columns past the given ones: 0)
template <int KPAD>
__global__ __launch_bounds__(256) void k_dq_interleave(const long long* __restrict__ planar, size_t stride, int n_thr, int64_t m,
                                                       unsigned long long* __restrict__ tab) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
#pragma unroll
    for (int k = 0; k < KPAD; ++k)
        tab[(size_t)i * KPAD + k] = k < n_thr ? (unsigned long long)planar[(size_t)k * stride + (size_t)i] : 0ull;
}

// max of the entries [j0, j1) of one 16-entry block (one 64-byte line, four 16-byte loads).  The entries outside the range are
// cleared with an arithmetic mask (depths are >= 0), so the sixteen steps are plain vector instructions: no lane masks to keep
__device__ __forceinline__ int32_t dq_block_max(const int32_t* __restrict__ block, int j0, int j1) {
    const int4* bp = reinterpret_cast<const int4*>(block);
    const int4 w0 = bp[0], w1 = bp[1], w2 = bp[2], w3 = bp[3];
    const int32_t v[16] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
    const uint32_t in = ((1u << j1) - 1u) & ~((1u << j0) - 1u);                // j1 <= 16
    int32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) m = max(m, v[j] & -(int32_t)((in >> j) & 1u));
    return m;
}

// max over the blocks [i0, i1), i0 < i1 <= nb = number of blocks: per level the partial 16-block at either end, the whole
// 16-blocks in between one level up; ends when what is left lies inside one 16-block (at the latest on the highest level, which
// is one block).  The level offsets of hier_shape are carried along (each level is padded to whole 16-blocks), so the walk needs
// the tree's base and nb only.  One 16-block per step: `right` holds the right-hand partial block of a level for the next step.
__device__ __forceinline__ int32_t range_max16(const int32_t* __restrict__ tree, int nb, int i0, int i1) {
    int32_t m = 0;
    int lo = i0, hi = i1, len = nb;
    uint32_t off = 0;
    bool right = false;
    while (lo < hi) {
        const int bl = lo & ~15, bh = (hi - 1) & ~15;
        const bool last = bl == bh;
        int base, j0, j1;
        if (right) { base = bh; j0 = 0; j1 = hi - bh; }
        else { base = bl; j0 = lo - bl; j1 = last ? hi - bl : 16; }
        // a level whose left end is aligned has no left partial block; one whose right end is aligned has no right one
        const bool skip = !last && (right ? (hi & 15) == 0 : lo == bl);
        if (!skip) m = max(m, dq_block_max(tree + (size_t)off + (size_t)base, j0, j1));
        if (last) break;
        if (!right) { right = true; continue; }
        right = false;
        lo = (lo + 15) >> 4;
        hi >>= 4;
        off += (uint32_t)((len + 15) & ~15);
        len = (len + 15) >> 4;
    }
    return m;
}

// what the probe kernel reads of the index of the blocks
struct DqIndex {
    const int4* cmeta_j;      // joint grid: per-contig metadata (two int4)
    const int4* crec;         //             16-byte bin records
    const int32_t* b_start;   // block starts = the start order
    const int32_t* e_end;     // block ends = the end order
    int32_t n_contigs;
};

template <int KPAD>
__device__ __forceinline__ void dq_load_row(const unsigned long long* __restrict__ tab, int i, unsigned long long (&out)[KPAD > 0 ? KPAD : 1]) {
    if constexpr (KPAD == 1) out[0] = tab[i];
    else if constexpr (KPAD >= 2) {
        typedef unsigned long long v2u __attribute__((ext_vector_type(2)));
        const v2u* p = reinterpret_cast<const v2u*>(tab + (size_t)i * KPAD);
#pragma unroll
        for (int k = 0; k < KPAD / 2; ++k) { const v2u v = p[k]; out[2 * k] = v.x; out[2 * k + 1] = v.y; }
    }
}

// ix = the index of the BLOCKS (joint grid, b_start, e_end); tree (nb blocks) / brec / tab as above.  KPAD = 0: no thresholds (max_depth only).
// max_depth == nullptr: thresholds only.  bases_ge is column-major, n rows per column, n_thr columns.
template <bool STRICT, int KPAD, bool LM>
__global__ __launch_bounds__(PROBE_THREADS) void k_depth_query(DqIndex ix, const int32_t* __restrict__ tree, int nb, const int4* __restrict__ brec,
                                                               const unsigned long long* __restrict__ tab, DqThresholds thr, int n_thr,
                                                               const int32_t* __restrict__ pc, const int32_t* __restrict__ ps,
                                                               const int32_t* __restrict__ pe, int64_t n, int vec,
                                                               int32_t* __restrict__ max_depth, long long* __restrict__ bases_ge) {
    constexpr int N = PROBE_ITEMS_LAT;
    static_assert(N == 2, "the vector stores below write the two results of a lane");
    constexpr int KR = KPAD > 0 ? KPAD : 1;
    const bool vec_ok = vec & 1, vec_out = vec & 2, vec_md = vec & 4;      // probe columns / bases_ge columns / max_depth take vector access
    __shared__ int4 l_cm[LM ? 2 * CM_LDS : 1];
    if (LM) {
        for (int i = threadIdx.x; i < 2 * ix.n_contigs; i += PROBE_THREADS) l_cm[i] = ix.cmeta_j[i];
        __syncthreads();
    }
#pragma unroll 1
  for (int t = 0; t < DQ_TILES_PER_WG; ++t) {
    const int64_t r0 = ((int64_t)blockIdx.x * DQ_TILES_PER_WG + t) * (PROBE_THREADS * N) + (int64_t)threadIdx.x * N;
    if (r0 - (int64_t)threadIdx.x * N >= n) break;
    int32_t c[N], s[N], e[N];
    load_items_nt(pc, r0, n, vec_ok, -1, c);
    load_items_nt(ps, r0, n, vec_ok, 0, s);
    load_items_nt(pe, r0, n, vec_ok, 0, e);
    // phase 1: metadata and the (usually single) joint-grid record of every probe, issued together
    int a[N], b[N];
    unsigned long long te[N], ts[N];
    int he[N], hs[N];          // 0: rank = a, 1: rank = b, 2: table
    bool same[N], wide[N];
    uint32_t oe[N], os[N];
    int4 re[N], rs[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const bool ok = r0 + k < n && (uint32_t)c[k] < (uint32_t)ix.n_contigs;
        int4 m0 = make_int4(0, 0, 0, 0), m1 = make_int4(0, 0, 0, 0);
        if (ok) {
            if (LM) { m0 = l_cm[2 * c[k]]; m1 = l_cm[2 * c[k] + 1]; }
            else { m0 = ix.cmeta_j[2 * c[k]]; m1 = ix.cmeta_j[2 * c[k] + 1]; }
        }
        a[k] = m0.x; b[k] = m0.y;
        const uint32_t ulo = (uint32_t)m0.z, uhi = (uint32_t)m0.w;
        te[k] = (unsigned long long)flip(e[k]) + (STRICT ? 0ull : 1ull);   // blocks that start below it touch the probe's last position
        ts[k] = (unsigned long long)flip(s[k]) + (STRICT ? 1ull : 0ull);   // blocks that end below it lie before the probe's first position
        he[k] = (b[k] <= a[k] || te[k] <= ulo) ? 0 : (te[k] > uhi ? 1 : 2);
        hs[k] = (b[k] <= a[k] || ts[k] <= ulo) ? 0 : (ts[k] > uhi ? 1 : 2);
        const uint32_t de = (uint32_t)te[k] - ulo, ds = (uint32_t)ts[k] - ulo, bmask = (1u << m1.x) - 1u;   // shift <= 31
        const uint32_t se = he[k] == 2 ? (uint32_t)m1.y + (de >> m1.x) : 0u;
        const uint32_t ss = hs[k] == 2 ? (uint32_t)m1.y + (ds >> m1.x) : 0u;
        oe[k] = de & bmask; os[k] = ds & bmask; wide[k] = m1.x > 16;
        same[k] = he[k] == 2 && hs[k] == 2 && se == ss;
        re[k] = make_int4(0, 0, 0, 0); rs[k] = make_int4(0, 0, 0, 0);
        if (he[k] == 2) re[k] = ix.crec[se];
        if (hs[k] == 2 && !same[k]) rs[k] = ix.crec[ss];
    }
    // phase 2: the block range [i0, i1) of every probe
    int i0[N], i1[N];
    bool live[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (same[k]) rs[k] = re[k];
        i1[k] = he[k] == 0 ? a[k] : (he[k] == 1 ? b[k] : joint_rank(ix.b_start, re[k].x, (uint32_t)re[k].z, oe[k], wide[k], te[k], b[k]));
        i0[k] = hs[k] == 0 ? a[k] : (hs[k] == 1 ? b[k] : joint_rank(ix.e_end, rs[k].y, (uint32_t)rs[k].w, os[k], wide[k], ts[k], b[k]));
        const bool empty = STRICT ? (s[k] >= e[k]) : (s[k] > e[k]);
        live[k] = !empty && i1[k] > i0[k];
    }
    // phase 3: both prefix rows and both block records of every probe, issued together
    unsigned long long p0[N][KR], p1[N][KR];
    int4 q0[N], q1[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int j = 0; j < KR; ++j) { p0[k][j] = 0; p1[k][j] = 0; }
        q0[k] = make_int4(0, 0, 0, 0); q1[k] = make_int4(0, 0, 0, 0);
        if (KPAD > 0 && live[k]) {
            dq_load_row<KPAD>(tab, i0[k], p0[k]);
            dq_load_row<KPAD>(tab, i1[k], p1[k]);
            q0[k] = brec[i0[k]];
            q1[k] = brec[i1[k] - 1];
        }
    }
    long long out[N][KR];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const long long lc = (long long)s[k] - (long long)q0[k].x, rc = (long long)q1[k].y - (long long)e[k];
        const unsigned long long lclip = lc > 0 ? (unsigned long long)lc : 0ull, rclip = rc > 0 ? (unsigned long long)rc : 0ull;
#pragma unroll
        for (int j = 0; j < KR; ++j) {
            // depth >= T as an all-ones word (T - 1 - depth < 0, no overflow: T >= 1, depth >= 0): selects without lane masks
            const unsigned long long ge0 = (unsigned long long)(long long)(((thr.t[j] - 1) - q0[k].z) >> 31);
            const unsigned long long ge1 = (unsigned long long)(long long)(((thr.t[j] - 1) - q1[k].z) >> 31);
            const unsigned long long v = p1[k][j] - p0[k][j] - (lclip & ge0) - (rclip & ge1);
            out[k][j] = (KPAD > 0 && live[k]) ? (long long)v : 0ll;
        }
    }
    // the range maximum: from the two records when they are all the probe touches, over the tree otherwise
    int32_t md[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        md[k] = 0;
        if (max_depth && live[k]) {
            if (KPAD > 0 && i1[k] - i0[k] <= 2) md[k] = q0[k].z > q1[k].z ? q0[k].z : q1[k].z;
            else md[k] = range_max16(tree, nb, i0[k], i1[k]);
        }
    }
    // one store stream per column.  vec_out / vec_md (host): every column of bases_ge is 16-byte aligned / max_depth is 8-byte
    // aligned, so a lane's two results go out as one store.  KPAD is the threshold count rounded up, so the columns below
    // KPAD / 2 + 1 always exist and only the ones above are tested against n_thr.
    const bool full = r0 + N <= n;
    if (KPAD > 0) {
        long long* at = bases_ge + r0;                                         // the lane's place in column j: one add of n per column
#pragma unroll
        for (int j = 0; j < KR; ++j, at += n) {
            if (j > KPAD / 2 && j >= n_thr) continue;
            if (full && vec_out) {
                typedef long long v2ll __attribute__((ext_vector_type(2)));
                v2ll v; v.x = out[0][j]; v.y = out[N - 1][j];
                __builtin_nontemporal_store(v, reinterpret_cast<v2ll*>(at));
            } else {
#pragma unroll
                for (int k = 0; k < N; ++k) if (r0 + k < n) at[k] = out[k][j];
            }
        }
    }
    if (max_depth) {
        if (full && vec_md) {
            typedef int v2i __attribute__((ext_vector_type(2)));
            v2i v; v.x = md[0]; v.y = md[N - 1];
            __builtin_nontemporal_store(v, reinterpret_cast<v2i*>(max_depth + r0));
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) if (r0 + k < n) max_depth[r0 + k] = md[k];
        }
    }
  }
}

}  // namespace ivj
