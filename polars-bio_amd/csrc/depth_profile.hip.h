// depth_profile.hip.h -- pb.depth_profile: every window row cut into n_bins bins, per bin the positions it shares with EVERY build
// row of the window's contig, summed (overlap_bases of the bin as a probe row) -- a rows x bins matrix made on the device from the
// 12 bytes of each window.
//
// Positions are the 33-bit u = flip(x) of depth_sum.hip.h: a window covers [xs, xe), xs = flip(start), xe = flip(end) + w (w = 0
// Strict / 1 Weak), L = xe - xs positions (none when xe <= xs), and the B + 1 bin edges are x_j = xs + floor(j L / B), j = 0 .. B
// (64-bit: j L reaches 2^44).  Bin j = [x_j, x_{j+1}): lengths differ by at most one and sum to L.
//
// bases of bin j = G(x_{j+1}) - G(x_j) with the G of depth_sum.hip.h, so G is evaluated ONCE PER EDGE -- B + 1 times per row, not 2 B.
// One joint-grid target t per edge answers both ranks.  A key equal to x contributes x - key = 0, so a rank may count ties or not:
//   ra over A = flip(b_start):      every A < x counted, no A > x        <=>  t in {x, x + 1}
//   rb over flip(e_end), B = . + w: every B < x counted, no B > x        <=>  t in {x, x + 1} Strict,  t in {x - 1, x} Weak
// hence t = x in both modes (for an edge that is a window's end this is depth_sum's te, for its start a tie-counting variant of ts).
// Per edge: one 16-byte record gather (joint_rank: a crowded bin gallops over the key array as in k_count_overlaps) and two 8-byte
// prefix gathers,
//   G'(x) = x (ra - rb) - PA[ra] + PE[rb] + w rb
// -- depth_sum's G less the terms PA[a], PE[a], w a of the contig segment, which are the same for every edge of a row and cancel
// in the difference.  uint64 with wrap-around, exact as there.
//
// Layout: the n (B + 1) edges of all rows are ONE flat sequence laid over the lanes, consecutive edges on consecutive lanes, so that
// neighbouring lanes gather the same or the next grid record.  A workgroup evaluates DPROF_WG_SLOTS consecutive edges (DPROF_ITEMS
// per thread, each item a run of PROBE_THREADS consecutive edges: the gathers of all items are in flight together), parks the G'
// values in LDS and forms a bin from two neighbouring slots.  Rows straddle wavefronts, items and workgroups freely: the workgroups
// advance by DPROF_WG_EDGES = DPROF_WG_SLOTS - 1, i.e. the last edge of a workgroup is evaluated again as the first of the next
// (one edge in 1024), and a row's own last edge (j = B) forms no bin.  No atomics; every output word is written once by one lane:
// the result is identical from run to run.  The B values of a row are contiguous in the output and so are the lanes that write them
// (descending addresses inside the row when its reverse flag is set): the stores coalesce.
//
// An index that holds a row with start > end (flags[0] != 0) takes the bounded scan of depth_sum.hip.h (scan_bases) per bin, from
// the rank of the bin's upper edge in the start order -- decided on the device from the flag.
#pragma once
#include "depth_sum.hip.h"

namespace ivj {

constexpr int DPROF_ITEMS = 4;                                   // edges per thread
constexpr int DPROF_TILE = PROBE_THREADS;                        // consecutive edges of one item across the workgroup's lanes
constexpr int DPROF_WG_SLOTS = DPROF_TILE * DPROF_ITEMS;         // edges a workgroup evaluates
constexpr int DPROF_WG_EDGES = DPROF_WG_SLOTS - 1;               // edges a workgroup advances by: its last slot is the next one's first
constexpr int DPROF_MAX_BINS = 4096;

template <bool STRICT, bool LM>
__global__ __launch_bounds__(PROBE_THREADS) void k_depth_profile(IndexView ix, const unsigned long long* __restrict__ pa,
                                                                 const unsigned long long* __restrict__ pe_sum,
                                                                 const int32_t* __restrict__ wc, const int32_t* __restrict__ ws,
                                                                 const int32_t* __restrict__ we, const uint8_t* __restrict__ reverse,
                                                                 int64_t n, int n_bins, long long* __restrict__ bases) {
    constexpr int N = DPROF_ITEMS;
    __shared__ int4 l_cm[LM ? 2 * CM_LDS : 1];
    __shared__ unsigned long long l_g[DPROF_WG_SLOTS];
    __shared__ int l_ra[DPROF_WG_SLOTS];
    if (LM) {
        for (int i = threadIdx.x; i < 2 * ix.n_contigs; i += PROBE_THREADS) l_cm[i] = ix.cmeta_j[i];
        __syncthreads();
    }
    const bool inv = ix.flags[0] != 0;
    const uint32_t B = (uint32_t)n_bins, B1 = B + 1u;
    // the workgroup's first edge as (row, edge of the row): one 64-bit division, uniform; the lanes go on in 32 bits
    const unsigned long long g0 = (unsigned long long)blockIdx.x * DPROF_WG_EDGES;
    const int64_t row0 = (int64_t)(g0 / B1);
    const uint32_t j0 = (uint32_t)(g0 % B1);

    // phase 1: the window, the edge, the contig's metadata and the (single) record gather of every edge, issued together
    int64_t row[N];
    uint32_t j[N];
    int a[N], b[N], h[N];          // h: 0 ranks = a, 1 ranks = b, 2 table
    bool live[N], wide[N];         // live: the edge belongs to a window that has positions on a contig that has build rows
    unsigned long long x[N], xs[N], len[N];
    uint32_t off[N];
    int4 rec[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const uint32_t o = j0 + (uint32_t)(k * DPROF_TILE) + threadIdx.x;        // < 4097 + 1024
        row[k] = row0 + (int64_t)(o / B1);
        j[k] = o % B1;
        const bool in = row[k] < n;
        int32_t c = -1, s = 0, e = 0;
        if (in) { c = wc[row[k]]; s = ws[row[k]]; e = we[row[k]]; }
        const bool ok = in && (uint32_t)c < (uint32_t)ix.n_contigs;
        int4 m0 = make_int4(0, 0, 0, 0), m1 = make_int4(0, 0, 0, 0);
        if (ok) {
            if (LM) { m0 = l_cm[2 * c]; m1 = l_cm[2 * c + 1]; }
            else { m0 = ix.cmeta_j[2 * c]; m1 = ix.cmeta_j[2 * c + 1]; }
        }
        a[k] = m0.x; b[k] = m0.y;
        const uint32_t ulo = (uint32_t)m0.z, uhi = (uint32_t)m0.w;
        xs[k] = (unsigned long long)flip(s);
        const unsigned long long xe = (unsigned long long)flip(e) + (STRICT ? 0ull : 1ull);
        len[k] = xe > xs[k] ? xe - xs[k] : 0ull;
        x[k] = xs[k] + (unsigned long long)j[k] * len[k] / B;                    // j L < 2^13 x 2^32
        live[k] = ok && b[k] > a[k] && len[k] != 0;
        h[k] = (!live[k] || x[k] <= ulo) ? 0 : (x[k] > uhi ? 1 : 2);
        const uint32_t d = (uint32_t)x[k] - ulo, bmask = (1u << m1.x) - 1u;      // shift <= 31
        off[k] = d & bmask; wide[k] = m1.x > 16;
        rec[k] = make_int4(0, 0, 0, 0);
        if (h[k] == 2) rec[k] = ix.crec[(uint32_t)m1.y + (d >> m1.x)];
    }
    // phase 2: both ranks of every edge from its record
    int ra[N], rb[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        ra[k] = h[k] == 0 ? a[k] : (h[k] == 1 ? b[k] : joint_rank(ix.b_start, rec[k].x, (uint32_t)rec[k].z, off[k], wide[k], x[k], b[k]));
        rb[k] = a[k];
        if (live[k] && !inv)
            rb[k] = h[k] == 0 ? a[k] : (h[k] == 1 ? b[k] : joint_rank(ix.e_end, rec[k].y, (uint32_t)rec[k].w, off[k], wide[k], x[k], b[k]));
    }
    // phase 3: the two prefix gathers of every edge, issued together
    unsigned long long ga[N], gb[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        ga[k] = 0; gb[k] = 0;
        if (live[k] && !inv) { ga[k] = pa[ra[k]]; gb[k] = pe_sum[rb[k]]; }
    }
    unsigned long long g[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        g[k] = 0;
        if (live[k] && !inv) {
            g[k] = x[k] * (unsigned long long)(long long)(ra[k] - rb[k]) - ga[k] + gb[k];
            if (!STRICT) g[k] += (unsigned long long)(long long)rb[k];
        }
        l_g[k * DPROF_TILE + threadIdx.x] = g[k];
        l_ra[k * DPROF_TILE + threadIdx.x] = ra[k];
    }
    __syncthreads();
    // a bin = this slot's edge and the next slot's: the same row whenever j < B.  The workgroup's last slot forms none (the next
    // workgroup starts on it).
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int slot = k * DPROF_TILE + (int)threadIdx.x;
        if (slot >= DPROF_WG_EDGES || row[k] >= n || j[k] >= B) continue;
        unsigned long long v = l_g[slot + 1] - g[k];
        if (inv) {
            v = 0;
            const unsigned long long x1 = xs[k] + (unsigned long long)(j[k] + 1u) * len[k] / B;
            if (live[k] && x[k] < x1) v = scan_bases<STRICT>(ix, a[k], l_ra[slot + 1], unflip((uint32_t)x[k]), x[k], x1);
        }
        const bool rev = reverse != nullptr && reverse[row[k]] != 0;
        __builtin_nontemporal_store((long long)v, bases + row[k] * (int64_t)B + (rev ? B - 1u - j[k] : j[k]));
    }
}

}  // namespace ivj
