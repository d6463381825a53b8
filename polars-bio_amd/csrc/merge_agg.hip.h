// merge_agg.hip.h -- pb.merge(agg=...): count / sum / min / max / mean of a value column per merged interval
// (bedtools merge -c/-o).  The cluster sweep of sortscan.hip.h leaves every cluster as a run of equal ids cid1[p] over
// the sorted positions p, and b_row[p] names the input row of p: an aggregate is a segmented reduction over the gather
// values[b_row[p]].
//
//   k_magg_tiles  one workgroup per tile of MAGG_THREADS * MAGG_ITEMS sorted positions.  A thread reduces its MAGG_ITEMS
//                 consecutive positions from its last segment head on; a segmented scan of those thread aggregates (wavefront
//                 first, then across the four wavefronts through LDS) hands every thread the reduction of what precedes it
//                 back to the nearest head inside the tile.  A segment that begins and ends inside the tile is written by
//                 the position that ends it.  The segment open at the tile's start leaves its part in part[2 * tile] (a tile
//                 wholly inside one cluster leaves only this one), the segment that begins inside the tile and is still
//                 open at its end leaves part[2 * tile + 1].
//   k_magg_span   one wavefront per tile: the tile whose last position belongs to a cluster that begins inside it and goes on
//                 past it owns that cluster, and folds its parts -- part[2 * first + 1], then part[2 * t] of the following
//                 tiles -- in ascending tile order, 64 at a time through a fixed shuffle tree.  At most one cluster per tile.
//
// The work per position does not depend on the cluster sizes: no thread or wavefront loops over a cluster's rows; the only
// loop is k_magg_span's over the TILES of one cluster (5 M rows = 2442 tiles = 39 steps of one wavefront).  No atomics: given
// the sorted order, the evaluation order of every sum is fixed by the tile geometry, so integer results are bit-identical from
// run to run and double sums are as reproducible as the order of the index among rows of equal (contig, start) -- see the ABI
// comment of ivj_merge_agg.
//
// State per segment: count of valid values, sum (uint64 for int64 columns: wraps modulo 2^64; double for double columns),
// min, max.  The identities make every merge branch-free: -0.0 for the double sum (x + -0.0 == x bit for bit, for +-0 too),
// NaN for the double min / max (fmin / fmax return the other operand, so NaN survives only where every value is NaN).
#pragma once
#include "scan.hip.h"

namespace ivj {

constexpr int MAGG_THREADS = 256;
constexpr int MAGG_ITEMS = 8;
constexpr int MAGG_TILE = MAGG_THREADS * MAGG_ITEMS;
constexpr int MAGG_WAVES = MAGG_THREADS / kWave;

template <class V> struct AggState;

template <> struct AggState<long long> {
    using Sum = unsigned long long;
    long long cnt;
    unsigned long long sum;
    long long mn, mx;
    __device__ __forceinline__ static AggState identity() { return {0ll, 0ull, 0x7fffffffffffffffll, -0x7fffffffffffffffll - 1ll}; }
    __device__ __forceinline__ void add(long long v) {
        ++cnt; sum += (unsigned long long)v;
        mn = v < mn ? v : mn; mx = v > mx ? v : mx;
    }
    __device__ __forceinline__ static AggState merge(const AggState& a, const AggState& b) {      // a = the earlier positions
        return {a.cnt + b.cnt, a.sum + b.sum, b.mn < a.mn ? b.mn : a.mn, b.mx > a.mx ? b.mx : a.mx};
    }
    __device__ __forceinline__ double mean() const { return (double)(long long)sum / (double)cnt; }
};

template <> struct AggState<double> {
    using Sum = double;
    long long cnt;
    double sum, mn, mx;
    __device__ __forceinline__ static AggState identity() { return {0ll, -0.0, __builtin_nan(""), __builtin_nan("")}; }
    __device__ __forceinline__ void add(double v) {
        ++cnt; sum += v;
        mn = fmin(mn, v); mx = fmax(mx, v);
    }
    __device__ __forceinline__ static AggState merge(const AggState& a, const AggState& b) {
        return {a.cnt + b.cnt, a.sum + b.sum, fmin(a.mn, b.mn), fmax(a.mx, b.mx)};
    }
    __device__ __forceinline__ double mean() const { return sum / (double)cnt; }
};

// the caller's columns of one value column (capacity >= number of clusters); NULL = not asked for
template <class V> struct AggOut {
    typename AggState<V>::Sum* sum;
    V* mn;
    V* mx;
    double* mean;
    long long* count;
};

template <class V>
__device__ __forceinline__ void magg_write(const AggOut<V>& o, int64_t c, const AggState<V>& s) {
    if (o.count) o.count[c] = s.cnt;
    if (o.sum) o.sum[c] = s.cnt ? s.sum : (typename AggState<V>::Sum)0;       // no valid value: 0 (the double identity is -0.0)
    if (o.mn) o.mn[c] = s.mn;
    if (o.mx) o.mx[c] = s.mx;
    if (o.mean) o.mean[c] = s.mean();
}

template <class S>
__device__ __forceinline__ S magg_shfl_up(const S& s, int d) {
    S o;
    o.cnt = __shfl_up(s.cnt, d, kWave); o.sum = __shfl_up(s.sum, d, kWave);
    o.mn = __shfl_up(s.mn, d, kWave); o.mx = __shfl_up(s.mx, d, kWave);
    return o;
}
template <class S>
__device__ __forceinline__ S magg_shfl_down(const S& s, int d) {
    S o;
    o.cnt = __shfl_down(s.cnt, d, kWave); o.sum = __shfl_down(s.sum, d, kWave);
    o.mn = __shfl_down(s.mn, d, kWave); o.mx = __shfl_down(s.mx, d, kWave);
    return o;
}

// cid1: 1-based cluster id per sorted position (non-decreasing); values[b_row[p]] is the value of position p, used when
// 0 <= b_row[p] < n_values and (valid == NULL or valid[b_row[p]]).  part: 2 * number of tiles states.
template <class V>
__global__ __launch_bounds__(MAGG_THREADS) void k_magg_tiles(const uint32_t* __restrict__ cid1, const int32_t* __restrict__ b_row,
                                                             const V* __restrict__ values, const uint8_t* __restrict__ valid,
                                                             int64_t n, int64_t n_values, AggOut<V> out, AggState<V>* __restrict__ part) {
    using S = AggState<V>;
    __shared__ S w_agg[MAGG_WAVES];
    __shared__ int w_head[MAGG_WAVES];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = threadIdx.x / kWave;
    const int64_t p0 = (int64_t)blockIdx.x * MAGG_TILE + (int64_t)threadIdx.x * MAGG_ITEMS;

    // ids of positions p0 - 1 .. p0 + MAGG_ITEMS; 0 = no such position (ids are 1-based), which makes position 0 a head and
    // position n - 1 an end without further tests
    uint32_t cid[MAGG_ITEMS + 2];
#pragma unroll
    for (int j = 0; j < MAGG_ITEMS + 2; ++j) {
        const int64_t q = p0 - 1 + j;
        cid[j] = (q >= 0 && q < n) ? cid1[q] : 0u;
    }
    V x[MAGG_ITEMS];
    bool ok[MAGG_ITEMS];
#pragma unroll
    for (int j = 0; j < MAGG_ITEMS; ++j) {
        ok[j] = false;
        x[j] = (V)0;
        if (p0 + j < n) {
            const int64_t r = (int64_t)b_row[p0 + j];
            if ((uint64_t)r < (uint64_t)n_values && (!valid || valid[r])) { ok[j] = true; x[j] = values[r]; }
        }
    }

    // this thread's aggregate: its positions from its last head on (all of them when it holds no head)
    S agg = S::identity();
    bool has_head = false;
#pragma unroll
    for (int j = 0; j < MAGG_ITEMS; ++j) {
        if (cid[j + 1] != 0u && cid[j + 1] != cid[j]) { agg = S::identity(); has_head = true; }
        if (ok[j]) agg.add(x[j]);
    }

    // inclusive segmented scan over the wavefront: (a, b) -> (b.head ? b : a + b, a.head | b.head)
    S inc = agg;
    int inc_head = has_head ? 1 : 0;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const S o = magg_shfl_up(inc, d);
        const int oh = __shfl_up(inc_head, d, kWave);
        if (lane >= d) {
            if (!inc_head) inc = S::merge(o, inc);
            inc_head |= oh;
        }
    }
    if (lane == kWave - 1) { w_agg[w] = inc; w_head[w] = inc_head; }
    __syncthreads();
    S carry = S::identity();           // the wavefronts before this one, back to their last head
    int carry_head = 0;
#pragma unroll
    for (int i = 0; i < MAGG_WAVES; ++i) {
        if (i < w) {
            const S v = w_agg[i];
            const int h = w_head[i];
            carry = h ? v : S::merge(carry, v);
            carry_head |= h;
        }
    }
    {
        S ex = magg_shfl_up(inc, 1);     // the lanes before this one
        int ex_head = __shfl_up(inc_head, 1, kWave);
        if (lane == 0) { ex = S::identity(); ex_head = 0; }
        carry = ex_head ? ex : S::merge(carry, ex);
        carry_head |= ex_head;
    }

    // second walk: every position that ends its segment knows the whole part of the segment that lies in this tile
    S run = carry;
    bool started = carry_head != 0;      // the running segment began inside this tile
#pragma unroll
    for (int j = 0; j < MAGG_ITEMS; ++j) {
        if (cid[j + 1] == 0u) continue;
        if (cid[j + 1] != cid[j]) { run = S::identity(); started = true; }
        if (ok[j]) run.add(x[j]);
        if (cid[j + 2] != cid[j + 1]) {
            if (started) magg_write(out, (int64_t)cid[j + 1] - 1, run);
            else part[2 * (int64_t)blockIdx.x] = run;
        } else if (threadIdx.x == MAGG_THREADS - 1 && j == MAGG_ITEMS - 1) {
            part[2 * (int64_t)blockIdx.x + (started ? 1 : 0)] = run;
        }
    }
}

// m_first[c]: sorted position of the first row of cluster c, m_first[number of clusters] = n
template <class V>
__global__ __launch_bounds__(MAGG_THREADS) void k_magg_span(const uint32_t* __restrict__ cid1, const int32_t* __restrict__ m_first,
                                                            int64_t n, int64_t n_tiles, const AggState<V>* __restrict__ part,
                                                            AggOut<V> out) {
    using S = AggState<V>;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t t = (int64_t)blockIdx.x * MAGG_WAVES + threadIdx.x / kWave;
    if (t >= n_tiles) return;
    const int64_t last = (t + 1) * MAGG_TILE - 1;            // last position of tile t
    if (last >= n - 1) return;                               // position n - 1 ends its cluster
    const uint32_t c1 = cid1[last];
    if (cid1[last + 1] != c1) return;                        // nothing open at the tile's end
    const int64_t c = (int64_t)c1 - 1;
    if ((int64_t)m_first[c] < t * MAGG_TILE) return;         // the cluster began in an earlier tile, which owns it
    const int64_t t_last = ((int64_t)m_first[c + 1] - 1) / MAGG_TILE;
    const int64_t k = t_last - t + 1;
    S acc = S::identity();
    for (int64_t base = 0; base < k; base += kWave) {
        const int64_t i = base + lane;
        S v = S::identity();
        if (i < k) v = part[i == 0 ? 2 * t + 1 : 2 * (t + i)];
        // balanced tree over neighbours: after the step of distance d, lane i (a multiple of 2 d) holds lanes i .. i + 2 d - 1 in
        // order; lanes off that path merge leftovers nobody reads
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) v = S::merge(v, magg_shfl_down(v, d));
        acc = S::merge(acc, v);                              // lane 0 holds the fold
    }
    if (lane == 0) magg_write(out, c, acc);
}

}  // namespace ivj
