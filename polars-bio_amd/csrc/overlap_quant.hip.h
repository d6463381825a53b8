// overlap_quant.hip.h -- pb.map_quantiles / pb.map_median: exact ORDER STATISTICS of a build-side (df2) value column over the build
// rows that match each probe (df1) row (bedtools map -o median).  The candidate walk of overlap_agg.hip.h joined to the radix select
// of depth_quant.hip.h: no pair is written anywhere and nothing is sorted.
//
// A probe row with m matching valid values v[0] <= ... <= v[m - 1] and K requests (q_j, upper_j) shared by all rows:
//     h = q_j * (double)(m - 1)  (one IEEE product, __dmul_rn),  rank = upper_j ? ceil(h) : floor(h),  out[row][j] = v[rank];
// count[row] = m; a row with m == 0 gets all-zero bits.  The order is that of the 64-bit KEY of a value (ovq_key): int64 with the
// sign bit flipped; doubles with every NaN made the canonical quiet NaN first, then u ^ (sign ? ~0 : 1 << 63) -- np.sort's order,
// NaN last, with -0.0 placed just below +0.0 (they compare equal, so which zero a rank returns is unspecified).
//
// The walk (ovq_walk) is the candidate walk of cand_walk.hip.h with the strided test loop: the loose candidate range of every probe
// of the tile from flat_range, never tightened, then per candidate the plain or (THRESH) the thresholded predicate on the 16-byte
// rec4 record (cand_match), the validity byte and the 8 value bytes of the same sorted position (k_oagg_gather's arrays).  A range
// may span any number of chunks.  What differs from overlap_agg.hip.h is what a match does, and that the walk is repeated.
//
// State per (row, rank), in LDS: a 2^B-bin uint32 histogram (dynamic; B = IVJ_OVQ_BITS), the 64-bit prefix (the key bits settled so
// far) and the 32-bit residual rank among the values whose key starts with that prefix (m < 2^31).  A workgroup owns
// P = floor(IVJ_OVQ_LDS_BYTES / (K * 2^B * 4)) consecutive rows, clamped to [1, IVJ_OVQ_MAX_TILE]; P * K never exceeds OVQ_MAXPK.
//
//   survey (once per tile)  every match adds 1 to m[row] and takes part in the tile's AND and OR of the keys (per lane, per
//           wavefront, then across the wavefronts through LDS).  A digit in which AND and OR agree varies in no key of the tile: it
//           needs no pass, its bits are the AND's.  Small integer scores, and float32 columns of one sign widened to double, settle
//           most digits here (the key of a negative double is its complement: with both signs the low zero bits differ).  Then one thread per (row, rank) forms the rank from m; the prefix starts as the AND.
//   select, most significant varying digit first, shift = digit * B   zero the histograms; walk again (the records are L2-resident);
//           a match whose key agrees with the (row, rank)'s prefix above the digit adds 1 to bin (key >> shift) & (2^B - 1); after
//           the barrier one thread per (row, rank) scans the bins for the first whose cumulative count exceeds the residual, takes
//           the count below it off the residual and writes the digit into the prefix.  After the last pass the prefix is the key.
// Ranks of a row may share a prefix, diverge, or be equal: each owns its histogram.  A row with m == 0 receives no add and is not
// scanned.  LDS adds only (every candidate of a chunk may add to one address: the LDS unit serialises them), no global atomic,
// integers only: identical from run to run.
// LDS: 48 KiB dynamic (the histograms) + 23.2 KiB static (OvqLds) = 71.2 KiB: two workgroups fit the CU's 160 KiB.
// What bounds it: per CANDIDATE (not per match) and walk one 16-byte record and the predicate, per match 8 value bytes, K LDS reads
// of the prefix and up to K LDS adds; paid 1 + npass times, npass = the varying digits of the tile (16 at B = 4 for arbitrary doubles).
#pragma once
#include "overlap_agg.hip.h"

namespace ivj {

constexpr int OVQ_BITS = IVJ_OVQ_BITS;
constexpr int OVQ_NB = 1 << OVQ_BITS;                                        // bins per (row, rank)
constexpr int OVQ_NDIG = (64 + OVQ_BITS - 1) / OVQ_BITS;                     // digits of a key (the top one may be short)
constexpr int OVQ_MAXPK = IVJ_OVQ_LDS_BYTES / (OVQ_NB * 4);                  // (row, rank) states of a workgroup
static_assert(OVQ_BITS >= 4 && OVQ_BITS <= 8, "below 4 bits P x K exceeds the tile; above 8 a row of 16 ranks exceeds the budget");
static_assert(IVJ_OVQ_MAX_TILE == THRESH_TILE, "a thread holds THRESH_ITEMS probes of the tile");
static_assert(IVJ_MAX_OVQ_RANKS * OVQ_NB * 4 <= IVJ_OVQ_LDS_BYTES, "one row's histograms fit the budget");
static_assert(sizeof(unsigned long long) == 8 && OVQ_MAXPK < 65536, "keys are 64-bit; a state index fits the walk's arithmetic");

// the requests of a call, by value in the kernel arguments
struct OvqReq {
    double q[IVJ_MAX_OVQ_RANKS];
    uint8_t upper[IVJ_MAX_OVQ_RANKS];
};

// the order-preserving key of a value's 8 bytes, and its inverse
template <int DTYPE>
__device__ __forceinline__ unsigned long long ovq_key(unsigned long long u) {
    constexpr unsigned long long SIGN = 1ull << 63;
    if (DTYPE == IVJ_AGG_I64) return u ^ SIGN;
    if ((u & ~SIGN) > 0x7ff0000000000000ull) u = 0x7ff8000000000000ull;      // every NaN is one value
    return u ^ ((u & SIGN) ? ~0ull : SIGN);
}
template <int DTYPE>
__device__ __forceinline__ unsigned long long ovq_unkey(unsigned long long k) {
    constexpr unsigned long long SIGN = 1ull << 63;
    if (DTYPE == IVJ_AGG_I64) return k ^ SIGN;
    return (k & SIGN) ? (k ^ SIGN) : ~k;
}

struct OvqLds {
    uint32_t base[THRESH_TILE];       // first candidate position of the probe - tile-local offset of its first candidate, modulo 2^32
    int2 q[THRESH_TILE];              // {start, end}
    uint32_t thr[THRESH_TILE];        // max(min_overlap, probe_min[row])
    uint32_t m[THRESH_TILE];          // matching valid candidates of the probe
    __align__(16) uint16_t marks[THRESH_CH];
    int scan_i[WALK_WAVES];
    long long scan_ll[WALK_WAVES];
    unsigned long long kand[WALK_WAVES], kor[WALK_WAVES];
    double rq[IVJ_MAX_OVQ_RANKS];
    uint32_t rup[IVJ_MAX_OVQ_RANKS];
    unsigned long long prefix[OVQ_MAXPK];
    uint32_t res[OVQ_MAXPK];
};

// One walk over the tile's T candidates (cand_walk.hip.h, the strided test loop): f(q, key) for every (probe q of the tile,
// candidate) that matches and whose value is valid.  cn / off: the thread's THRESH_ITEMS probes' candidate counts and tile-local
// offsets.  Uniform: every thread of the workgroup calls it.
template <bool STRICT, bool THRESH, int DTYPE, class F>
__device__ __forceinline__ void ovq_walk(const IndexView& ix, const uint32_t* __restrict__ bm_sorted, const unsigned long long* __restrict__ vals_sorted,
                                         const uint8_t* __restrict__ ok_sorted, const long long T, const int (&cn)[THRESH_ITEMS],
                                         const long long (&off)[THRESH_ITEMS], OvqLds& L, F&& f) {
    for (long long c0 = 0; c0 < T; c0 += THRESH_CH) {
        const int nC = walk_chunk_len(T, c0);
        walk_marks(L.marks, L.scan_i, c0, nC, off, cn);
        const uint32_t c0lo = (uint32_t)c0;
        for (int i = threadIdx.x; i < nC; i += THRESH_THREADS) {
            const WalkAt at = walk_probe(L.base, L.marks, i, c0lo);
            const int4 v = ix.rec4[at.p];                  // {start, end, build row, -}
            const bool m = cand_match<STRICT, THRESH>(L.q[at.q], v, L.thr[at.q], bm_sorted, at.p);
            if (m && ok_sorted[at.p] != 0) f(at.q, ovq_key<DTYPE>(vals_sorted[at.p]));
        }
    }
}

// P probes per workgroup, K requests per probe, `dyn` bytes of dynamic LDS >= P * K * OVQ_NB * 4.  pos (NULL: identity) = the
// probe's position in the caller's columns when the probes were bucketed: probe_min is read and the results are written there.
// out: row-major n x K, the column's 8-byte type; count: n entries or NULL.
template <bool STRICT, bool THRESH, int DTYPE>
__global__ __launch_bounds__(THRESH_THREADS, 2) void k_overlap_quant(IndexView ix, const int32_t* __restrict__ pc, const int32_t* __restrict__ ps,
                                                                     const int32_t* __restrict__ pe, const int32_t* __restrict__ pos, int64_t n,
                                                                     int P, int K, OvqReq rq, uint32_t min_overlap,
                                                                     const uint32_t* __restrict__ probe_min, const uint32_t* __restrict__ bm_sorted,
                                                                     const unsigned long long* __restrict__ vals_sorted,
                                                                     const uint8_t* __restrict__ ok_sorted, unsigned long long* __restrict__ out,
                                                                     long long* __restrict__ count) {
    extern __shared__ __align__(16) uint32_t l_ovq_hist[];
    __shared__ OvqLds L;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const long long ntiles = (n + P - 1) / P;
    const long long tile = xcd_tile64(blockIdx.x, ntiles);
    if (tile >= ntiles) return;                            // uniform
    const int64_t r0 = (int64_t)tile * P;
    const int np = (int)((n - r0) < (int64_t)P ? (n - r0) : (int64_t)P);      // >= 1
    const int cnt = np * K;                                                   // <= OVQ_MAXPK
#pragma unroll
    for (int j = 0; j < IVJ_MAX_OVQ_RANKS; ++j)
        if (tid == j) { L.rq[j] = rq.q[j]; L.rup[j] = rq.upper[j]; }
    // the loose candidate range of every probe
    int cn[THRESH_ITEMS], lo[THRESH_ITEMS];
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k) {
        const int q = tid * THRESH_ITEMS + k;
        const bool valid = q < np;
        int32_t c = -1, s = 0, e = 0;
        int64_t at = r0 + q;
        if (valid) {
            c = pc[r0 + q]; s = ps[r0 + q]; e = pe[r0 + q];
            if (pos) at = (int64_t)pos[r0 + q];
        }
        uint32_t thr = THRESH ? min_overlap : 0u;
        if (THRESH && valid && probe_min) { const uint32_t pm = probe_min[at]; thr = thr > pm ? thr : pm; }
        // (THRESH) a probe that covers no position, or whose own minimum is "never", has no candidates
        const bool can = THRESH ? (valid && thr != THRESH_NEVER && (STRICT ? s < e : s <= e)) : valid;
        flat_range<STRICT>(ix, c, s, e, can, lo[k], cn[k]);
        L.q[q] = make_int2(s, e); L.thr[q] = thr; L.m[q] = 0u;
    }
    long long T;
    long long off[THRESH_ITEMS];
    walk_offsets(cn, L.scan_ll, off, T);
#pragma unroll
    for (int k = 0; k < THRESH_ITEMS; ++k) L.base[tid * THRESH_ITEMS + k] = (uint32_t)lo[k] - (uint32_t)off[k];
    // survey: matches per probe, the AND and OR of the tile's keys  (the walk's first barrier publishes the LDS arrays)
    unsigned long long ka = ~0ull, ko = 0ull;
    ovq_walk<STRICT, THRESH, DTYPE>(ix, bm_sorted, vals_sorted, ok_sorted, T, cn, off, L, [&](int q, unsigned long long key) {
        atomicAdd(&L.m[q], 1u);
        ka &= key; ko |= key;
    });
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        ka &= (unsigned long long)__shfl_xor((long long)ka, o, kWave);
        ko |= (unsigned long long)__shfl_xor((long long)ko, o, kWave);
    }
    if (lane == 0) { L.kand[w] = ka; L.kor[w] = ko; }
    __syncthreads();                                       // ... and m[] is complete
    ka = ~0ull; ko = 0ull;
#pragma unroll
    for (int k = 0; k < WALK_WAVES; ++k) { ka &= L.kand[k]; ko |= L.kor[k]; }
    const unsigned long long vary = (ka & ~ko) ? 0ull : (ka ^ ko);            // no match in the tile: AND = ~0 and OR = 0, no pass
    // the state of every (probe, request): the rank among the probe's m values; the digits that do not vary are the AND's
    for (int i = tid; i < cnt; i += THRESH_THREADS) {
        const int q = i / K, j = i - q * K;
        const uint32_t m = L.m[q];
        uint32_t rank = 0u;
        if (m > 0u) {
            const double h = __dmul_rn(L.rq[j], (double)(m - 1u));
            const double r = L.rup[j] ? ceil(h) : floor(h);
            rank = (uint32_t)r;
            rank = rank < m ? rank : m - 1u;
        }
        L.prefix[i] = ka; L.res[i] = rank;
    }
    for (int d = OVQ_NDIG - 1; d >= 0; --d) {
        const int shift = d * OVQ_BITS;
        if (((vary >> shift) & (unsigned long long)(OVQ_NB - 1)) == 0ull) continue;     // uniform: the digit is settled
        __syncthreads();                                   // the previous pass's bins are read
        for (int i = tid; i < cnt * OVQ_NB; i += THRESH_THREADS) l_ovq_hist[i] = 0u;
        // (the walk's first barrier publishes the zeros and the state; a pass implies T > 0)
        ovq_walk<STRICT, THRESH, DTYPE>(ix, bm_sorted, vals_sorted, ok_sorted, T, cn, off, L, [&](int q, unsigned long long key) {
            const int bin = (int)((key >> shift) & (unsigned long long)(OVQ_NB - 1));
            for (int j = 0; j < K; ++j) {
                const unsigned long long x = key ^ L.prefix[q * K + j];
                const bool same = shift + OVQ_BITS >= 64 ? true : (x >> ((shift + OVQ_BITS) & 63)) == 0ull;
                if (same) atomicAdd(&l_ovq_hist[(q * K + j) * OVQ_NB + bin], 1u);
            }
        });
        __syncthreads();
        for (int i = tid; i < cnt; i += THRESH_THREADS) {
            if (L.m[i / K] == 0u) continue;
            const uint32_t rs = L.res[i];
            uint32_t cum = 0u;
            int t = 0;
            for (; t < OVQ_NB - 1; ++t) {
                const uint32_t c = l_ovq_hist[i * OVQ_NB + t];
                if (cum + c > rs) break;
                cum += c;
            }
            L.res[i] = rs - cum;
            L.prefix[i] = (L.prefix[i] & ~((unsigned long long)(OVQ_NB - 1) << shift)) | ((unsigned long long)t << shift);
        }
    }
    __syncthreads();
    // the tile's np x K block (contiguous in the row-major output unless the probes were bucketed) and its counts
    for (int i = tid; i < cnt; i += THRESH_THREADS) {
        const int q = i / K, j = i - q * K;
        const int64_t at = pos ? (int64_t)pos[r0 + q] : r0 + q;
        out[at * K + j] = L.m[q] ? ovq_unkey<DTYPE>(L.prefix[i]) : 0ull;
    }
    if (count) {
        for (int q = tid; q < np; q += THRESH_THREADS) {
            const int64_t at = pos ? (int64_t)pos[r0 + q] : r0 + q;
            count[at] = (long long)L.m[q];
        }
    }
}

}  // namespace ivj
