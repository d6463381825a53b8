// depth_sum.hip.h -- pb.mean_depth: per probe row the positions it shares with EVERY build row of its contig, summed (the integral of
// the build side's depth over the probe row), from weighted ranks on the joint grid of count_overlaps.
//
// 33-bit positions u = flip(x); a build row covers [A, B) with A = flip(start), B = flip(end) + w, w = 0 Strict / 1 Weak (a closed
// [s, e] is the half-open [s, e + 1): never wraps at INT32_MAX).  For one contig segment [a, b) of the index, A = b_start and
// flip(e_end) are sorted and share the segment offsets; PA / PE are exclusive 64-bit prefix sums of flip(b_start) / flip(e_end) over
// the whole array (n + 1 entries each, build_position_sums).  With ra / rb = ranks of x in A / B inside the segment
//   G(x) = sum_{A[k] < x} (x - A[k]) - sum_{B[k] < x} (x - B[k])
//        = x (ra - rb) - (PA[ra] - PA[a]) + (PE[rb] - PE[a]) + w (rb - a)
// is the number of covered (row, position) pairs below x, and bases = G(e'_q) - G(s_q) for a probe [s_q, e'_q), 0 when it is empty.
// A key equal to x contributes x - key = 0, so a rank may count ties or not: BOTH ranks of an endpoint come from the one target the
// count kernel already looks up (te for the end, ts for the start), i.e. from the one joint-grid record of that target -- the same
// two (usually one) 16-byte record gathers per probe as k_count_overlaps, then four 8-byte prefix gathers; PA[a] and PE[a] cancel.
// All sums are uint64 with wrap-around; the true value is below 2^63 (at most 2^31 rows x 2^32 positions), so the result is exact.
//
// An index that holds a row with start > end (flags[0] != 0) would count that row's length negative.  Such an index takes the bounded
// scan instead (the analogue of scan_count): from the probe's hi-bound down the start order while the prefix max of the ends is still
// above the probe's start, summing clipped lengths from ep -- one dependent 8-byte + one 4-byte read per row of the window, i.e.
// O(window) per probe instead of O(1), decided on the device from the flag: no host synchronisation, no re-index.
#pragma once
#include "count_nearest.hip.h"

namespace ivj {

// positions of a key column as uint64 (entry n = 0: the exclusive scan over n + 1 entries leaves the grand total there)
__global__ __launch_bounds__(256) void k_position_map(const int32_t* __restrict__ keys, int64_t n, unsigned long long* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= n) out[i] = i < n ? (unsigned long long)flip(keys[i]) : 0ull;
}

// clipped lengths of the start-ordered rows [a, hi) against the probe [xs, xe), for every input (zero-length and inverted rows count 0)
template <bool STRICT>
__device__ __forceinline__ unsigned long long scan_bases(const IndexView& ix, int a, int hi, int32_t qs, unsigned long long xs,
                                                         unsigned long long xe) {
    unsigned long long sum = 0;
    for (int p = hi - 1; p >= a; --p) {
        const int2 v = ix.ep[p];
        if (!lt_op<STRICT>(qs, v.y)) break;
        const unsigned long long rs = (unsigned long long)flip(ix.b_start[p]);
        const unsigned long long re = (unsigned long long)flip(v.x) + (STRICT ? 0ull : 1ull);
        const unsigned long long lo = rs > xs ? rs : xs, up = re < xe ? re : xe;
        sum += up > lo ? up - lo : 0ull;
    }
    return sum;
}

constexpr int DSUM_TILES_PER_WG = 4;

template <bool STRICT, int N, bool LM>
__global__ __launch_bounds__(PROBE_THREADS) void k_depth_sum(IndexView ix, const unsigned long long* __restrict__ pa,
                                                             const unsigned long long* __restrict__ pe_sum,
                                                             const int32_t* __restrict__ pc, const int32_t* __restrict__ ps,
                                                             const int32_t* __restrict__ pe, int64_t n, bool vec_ok,
                                                             long long* __restrict__ bases) {
    __shared__ int4 l_cm[LM ? 2 * CM_LDS : 1];
    if (LM) {
        for (int i = threadIdx.x; i < 2 * ix.n_contigs; i += PROBE_THREADS) l_cm[i] = ix.cmeta_j[i];
        __syncthreads();
    }
    const bool inv = ix.flags[0] != 0;
#pragma unroll 1
  for (int t = 0; t < DSUM_TILES_PER_WG; ++t) {
    const int64_t i0 = ((int64_t)blockIdx.x * DSUM_TILES_PER_WG + t) * (PROBE_THREADS * N) + (int64_t)threadIdx.x * N;
    if (i0 - (int64_t)threadIdx.x * N >= n) break;
    int32_t c[N], s[N], e[N];
    load_items_nt(pc, i0, n, vec_ok, -1, c);
    load_items_nt(ps, i0, n, vec_ok, 0, s);
    load_items_nt(pe, i0, n, vec_ok, 0, e);
    // phase 1: metadata and the (usually single) record gather of every probe, issued together
    int a[N], b[N];
    unsigned long long te[N], ts[N];
    int he[N], hs[N];          // 0: ranks = a, 1: ranks = b, 2: table
    bool same[N], wide[N];
    uint32_t oe[N], os[N];     // offset of the target inside its bin
    int4 re[N], rs[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const bool ok = i0 + k < n && (uint32_t)c[k] < (uint32_t)ix.n_contigs;
        int4 m0 = make_int4(0, 0, 0, 0), m1 = make_int4(0, 0, 0, 0);
        if (ok) {
            if (LM) { m0 = l_cm[2 * c[k]]; m1 = l_cm[2 * c[k] + 1]; }
            else { m0 = ix.cmeta_j[2 * c[k]]; m1 = ix.cmeta_j[2 * c[k] + 1]; }
        }
        a[k] = m0.x; b[k] = m0.y;
        const uint32_t ulo = (uint32_t)m0.z, uhi = (uint32_t)m0.w;
        te[k] = (unsigned long long)flip(e[k]) + (STRICT ? 0ull : 1ull);   // = e'_q: starts below it, ends (as B) at or below it
        ts[k] = (unsigned long long)flip(s[k]) + (STRICT ? 1ull : 0ull);   // starts and ends (as B) at or below s_q
        he[k] = (b[k] <= a[k] || te[k] <= ulo) ? 0 : (te[k] > uhi ? 1 : 2);
        hs[k] = (b[k] <= a[k] || ts[k] <= ulo) ? 0 : (ts[k] > uhi ? 1 : 2);
        const uint32_t de = (uint32_t)te[k] - ulo, ds = (uint32_t)ts[k] - ulo, bmask = (1u << m1.x) - 1u;   // shift <= 31
        const uint32_t se = he[k] == 2 ? (uint32_t)m1.y + (de >> m1.x) : 0u;
        const uint32_t ss = hs[k] == 2 ? (uint32_t)m1.y + (ds >> m1.x) : 0u;
        oe[k] = de & bmask; os[k] = ds & bmask; wide[k] = m1.x > 16;
        same[k] = he[k] == 2 && hs[k] == 2 && se == ss;                   // a probe is short against a bin: the usual case
        re[k] = make_int4(0, 0, 0, 0); rs[k] = make_int4(0, 0, 0, 0);
        if (he[k] == 2) re[k] = ix.crec[se];
        if (hs[k] == 2 && !same[k]) rs[k] = ix.crec[ss];
    }
    // phase 2: the four ranks of every probe (the record answers them; a crowded bin touches the key array)
    int rae[N], rbe[N], ras[N], rbs[N];
    bool plain[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (same[k]) rs[k] = re[k];
        rae[k] = he[k] == 0 ? a[k] : (he[k] == 1 ? b[k] : joint_rank(ix.b_start, re[k].x, (uint32_t)re[k].z, oe[k], wide[k], te[k], b[k]));
        const bool empty = STRICT ? (s[k] >= e[k]) : (s[k] > e[k]);
        plain[k] = !inv && !empty && b[k] > a[k];
        rbe[k] = a[k]; ras[k] = a[k]; rbs[k] = a[k];
        if (plain[k]) {
            rbe[k] = he[k] == 0 ? a[k] : (he[k] == 1 ? b[k] : joint_rank(ix.e_end, re[k].y, (uint32_t)re[k].w, oe[k], wide[k], te[k], b[k]));
            ras[k] = hs[k] == 0 ? a[k] : (hs[k] == 1 ? b[k] : joint_rank(ix.b_start, rs[k].x, (uint32_t)rs[k].z, os[k], wide[k], ts[k], b[k]));
            rbs[k] = hs[k] == 0 ? a[k] : (hs[k] == 1 ? b[k] : joint_rank(ix.e_end, rs[k].y, (uint32_t)rs[k].w, os[k], wide[k], ts[k], b[k]));
        }
    }
    // phase 3: the four prefix gathers of every probe, issued together
    unsigned long long g_ae[N], g_as[N], g_be[N], g_bs[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        g_ae[k] = 0; g_as[k] = 0; g_be[k] = 0; g_bs[k] = 0;
        if (plain[k]) { g_ae[k] = pa[rae[k]]; g_as[k] = pa[ras[k]]; g_be[k] = pe_sum[rbe[k]]; g_bs[k] = pe_sum[rbs[k]]; }
    }
    long long out[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const unsigned long long xe = te[k], xs = (unsigned long long)flip(s[k]);
        unsigned long long v = 0;
        if (plain[k]) {
            const unsigned long long ce = (unsigned long long)(long long)(rae[k] - rbe[k]), cs = (unsigned long long)(long long)(ras[k] - rbs[k]);
            v = xe * ce - xs * cs - (g_ae[k] - g_as[k]) + (g_be[k] - g_bs[k]);
            if (!STRICT) v += (unsigned long long)(long long)(rbe[k] - rbs[k]);
        } else if (inv && xs < xe) {
            v = scan_bases<STRICT>(ix, a[k], rae[k], s[k], xs, xe);
        }
        out[k] = (long long)v;
    }
    if (i0 + N <= n && (reinterpret_cast<uintptr_t>(bases) & 15u) == 0 && (N % 2) == 0) {
#pragma unroll
        for (int k = 0; k < N; k += 2) {
            typedef long long v2ll __attribute__((ext_vector_type(2)));
            v2ll v; v.x = out[k]; v.y = out[k + 1];
            __builtin_nontemporal_store(v, reinterpret_cast<v2ll*>(bases + i0) + k / 2);
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) if (i0 + k < n) bases[i0 + k] = out[k];
    }
  }
}

}  // namespace ivj
