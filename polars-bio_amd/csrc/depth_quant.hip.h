// depth_quant.hip.h -- pb.depth_quantiles / pb.median_depth: exact ORDER STATISTICS of the build side's depth over the positions
// of every probe row.
//
// A probe row with position set Q, L = |Q| >= 1, has the sorted depths v[0] <= ... <= v[L - 1] of its positions (uncovered positions
// are in the list at depth 0).  For K ranks per row:  out[row][j] = v[rank[row][j]];  -1 for a rank outside [0, L) and for a row
// without a position or outside the dictionary.  Quantiles are the host's arithmetic on ranks (range_op.quantile_ranks).
//
// k_depth_quant walks as k_depth_hist does (depth_hist.hip.h): the exact block range [i0, i1) of each probe from dh_range, then
// the candidate walk of cand_walk.hip.h with the strided test loop, one 16-byte {start, end, depth, 0} record per lane, and the
// two edge clips.  A range may span any number of chunks.  What differs is what an item does and that the walk is repeated: a radix select, most significant digit
// first, B = IVJ_QUANT_BITS bits per pass, over the depths under every row.
//
// State per (row, rank), in LDS: a 2^B-bin uint64 histogram (dynamic), a 32-bit prefix (the digits chosen so far) and the residual
// rank among the positions whose depth starts with that prefix.  A workgroup owns P = floor(IVJ_QUANT_LDS_BYTES / (K * 2^B * 8))
// consecutive rows, clamped to [1, IVJ_QUANT_MAX_TILE]; P * K never exceeds DQT_MAXPK.
//
//   survey (once per tile)  every item adds its clipped length to covered[row] (64-bit LDS add) and takes part in the tile's
//           maximum depth (a maximum per lane, per wavefront, then one LDS max).  uncovered = |Q| - covered.  The uncovered
//           positions are the smallest values of the list, so they are settled here and never enter a histogram: a rank below
//           `uncovered` is answered 0, any other rank continues as rank - uncovered among the covered positions (depth >= 1).
//           npass = ceil(bits(tile max depth) / B), uniform across the workgroup: one artefact pile elsewhere in the genome adds
//           no pass to this tile.  A tile with no block under it has npass = 0.
//   select, p = npass - 1 .. 0, shift = p B   zero the histograms; walk the items again (their records are L2-resident); an item of
//           clipped length len and depth d adds len to bin (d >> shift) & (2^B - 1) of each rank j of its row whose prefix equals
//           d >> (shift + B) (a 64-bit shift: shift + B reaches 32); after the barrier one thread per (row, rank) scans the bins
//           for the first t whose cumulative count exceeds the residual, takes the count below t off the residual and sets
//           prefix = prefix << B | t.  After the last pass the prefix is the answer.
// A settled (row, rank) carries a prefix with the top bit set (DQT_NONE: -1, DQT_ZERO: 0), which no depth >> n equals (depths are
// below 2^31), so the walk leaves it alone.  The residual is below |Q| <= 2^32 and is kept in 32 bits.
// Ranks of a row may share a prefix, diverge, or be equal: each owns its histogram, so none sees another.  Every item of a chunk
// may add to one address: the LDS unit serialises them.  No global atomic, integer adds only: identical from run to run.  The
// tile's P x K int32 block is contiguous in the row-major output and leaves coalesced.
// LDS: 64 KiB dynamic (the histograms; the survey's covered[] lies in them before the first pass) + 14.1 KiB static: per-probe
// {first block - offset, start, end} and 8256 bytes in which the contig metadata (LM, range phase only) is followed by the walk's
// marks and scan words and the per-(row, rank) state: two workgroups fit the CU's 160 KiB.
// What bounds it: per (row, block) incidence one 16-byte record read, K LDS reads of the prefix and up to K LDS adds per pass,
// paid 1 + npass times; n x K x 4 bytes written.
#pragma once
#include "depth_hist.hip.h"

namespace ivj {

constexpr int DQT_BITS = IVJ_QUANT_BITS;
constexpr int DQT_NB = 1 << DQT_BITS;                                        // bins per (row, rank)
constexpr int DQT_MAXPK = IVJ_QUANT_LDS_BYTES / (DQT_NB * 8);                // (row, rank) states of a workgroup
constexpr uint32_t DQT_NONE = 0xffffffffu, DQT_ZERO = 0xfffffffeu;           // settled: the answer is -1 / 0
static_assert(DQT_BITS >= 4 && DQT_BITS <= 8, "below 4 bits P x K exceeds the tile; above 8 a row of 16 ranks exceeds the budget");
static_assert(DQT_MAXPK <= WALK_TILE && IVJ_QUANT_MAX_TILE == WALK_TILE, "a thread holds WALK_ITEMS probes of the tile");
static_assert(IVJ_MAX_QUANT_RANKS * DQT_NB * 8 <= IVJ_QUANT_LDS_BYTES, "one row's histograms fit the budget");

// the walk's words and the select state, and the contig metadata they share their LDS with
struct DqtWords {
    __align__(16) uint16_t marks[WALK_CH];
    int scan_i[WALK_WAVES];
    long long scan_ll[WALK_WAVES];
    uint32_t tmax;                                         // the tile's maximum depth
    uint32_t pad[3];
    uint32_t prefix[DQT_MAXPK];
    uint32_t res[DQT_MAXPK];
};
constexpr int DQT_SCRATCH = 2 * CM_LDS * 16 > (int)sizeof(DqtWords) ? 2 * CM_LDS * 16 : (int)sizeof(DqtWords);
static_assert(DQT_SCRATCH % 16 == 0, "the dynamic LDS starts on a 16-byte boundary");

// One walk over the tile's T items (cand_walk.hip.h, the strided test loop): f(q, len, depth) for every (probe of the tile, block
// under it) with the block clipped to the probe.  cn / off: the thread's WALK_ITEMS probes' item counts and tile-local offsets;
// l_base[q] = first block - offset modulo 2^32.  Uniform: every thread of the workgroup calls it.
template <bool STRICT, class F>
__device__ __forceinline__ void dqt_walk(const long long T, const int (&cn)[WALK_ITEMS], const long long (&off)[WALK_ITEMS], DqtWords& W,
                                         const uint32_t* l_base, const int2* l_q, const int4* __restrict__ brec, F&& f) {
    for (long long c0 = 0; c0 < T; c0 += WALK_CH) {
        const int nC = walk_chunk_len(T, c0);
        walk_marks(W.marks, W.scan_i, c0, nC, off, cn);
        const uint32_t c0lo = (uint32_t)c0;
        for (int i = threadIdx.x; i < nC; i += WALK_THREADS) {
            const WalkAt at = walk_probe(l_base, W.marks, i, c0lo);
            const int2 qq = l_q[at.q];
            const int4 r = brec[at.p];                     // {start, end, depth, 0}
            const long long lo = qq.x > r.x ? qq.x : r.x, hi = qq.y < r.y ? qq.y : r.y;
            if (r.z > 0) f(at.q, (unsigned long long)(hi - lo + (STRICT ? 0ll : 1ll)), (uint32_t)r.z);
        }
    }
}

// ix = the index of the BLOCKS, brec = their {start, end, depth, 0} records; have == 0: no blocks at all (ix holds the dictionary
// size only).  P probes per workgroup, K ranks per probe, `dyn` bytes of dynamic LDS >= P * K * DQT_NB * 8.
// ranks: row-major n x K, 0-based; out: row-major n x K.
template <bool STRICT, bool LM>
__global__ __launch_bounds__(WALK_THREADS) void k_depth_quant(DqIndex ix, int have, const int4* __restrict__ brec, const int32_t* __restrict__ pc,
                                                            const int32_t* __restrict__ ps, const int32_t* __restrict__ pe, int64_t n, int P, int K,
                                                            const int64_t* __restrict__ ranks, int32_t* __restrict__ out) {
    extern __shared__ __align__(16) unsigned long long l_hist[];
    __shared__ uint32_t l_base[WALK_TILE];                   // first block of the probe - tile-local offset of its first item, modulo 2^32
    __shared__ int2 l_q[WALK_TILE];                          // {start, end}; {0, -1} for a probe without a position or outside the dictionary
    __shared__ __align__(16) unsigned char l_u[DQT_SCRATCH];
    const int4* l_cm = reinterpret_cast<const int4*>(l_u);
    DqtWords& W = *reinterpret_cast<DqtWords*>(l_u);
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int64_t r0 = (int64_t)blockIdx.x * P;
    const int np = (int)((n - r0) < (int64_t)P ? (n - r0) : (int64_t)P);      // >= 1 by the grid
    const int cnt = np * K;                                                   // <= DQT_MAXPK
    unsigned long long* l_cov = l_hist;                    // the survey's covered positions per probe, before the first pass
    for (int i = tid; i < np; i += WALK_THREADS) l_cov[i] = 0ull;
    if (LM && have) {
        int4* cm = reinterpret_cast<int4*>(l_u);
        for (int i = tid; i < 2 * ix.n_contigs; i += WALK_THREADS) cm[i] = ix.cmeta_j[i];
    }
    __syncthreads();
    // the block range of every probe
    int cn[WALK_ITEMS];
    int lo0[WALK_ITEMS];
#pragma unroll
    for (int k = 0; k < WALK_ITEMS; ++k) {
        const int q = tid * WALK_ITEMS + k;
        int32_t c = -1, s = 0, e = 0;
        if (q < np) { c = pc[r0 + q]; s = ps[r0 + q]; e = pe[r0 + q]; }
        const bool empty = STRICT ? (s >= e) : (s > e);
        const bool ok = q < np && !empty && (uint32_t)c < (uint32_t)ix.n_contigs;
        int i0 = 0, i1 = 0;
        if (ok && have) {
            int4 m0, m1;
            if (LM) { m0 = l_cm[2 * c]; m1 = l_cm[2 * c + 1]; }
            else { m0 = ix.cmeta_j[2 * c]; m1 = ix.cmeta_j[2 * c + 1]; }
            dh_range<STRICT>(ix, m0, m1, s, e, i0, i1);
        }
        cn[k] = i1 > i0 ? i1 - i0 : 0;
        lo0[k] = i0;
        l_q[q] = ok ? make_int2(s, e) : make_int2(0, -1);
    }
    __syncthreads();                                       // the contig metadata is read: its LDS turns into the walk's words
    long long T;
    long long off[WALK_ITEMS];
    walk_offsets(cn, W.scan_ll, off, T);
#pragma unroll
    for (int k = 0; k < WALK_ITEMS; ++k) l_base[tid * WALK_ITEMS + k] = (uint32_t)lo0[k] - (uint32_t)off[k];
    if (tid == 0) W.tmax = 0u;                             // (the walk's first barrier publishes it and l_base)
    // survey: covered positions per probe, the tile's maximum depth
    {
        uint32_t dmax = 0;
        dqt_walk<STRICT>(T, cn, off, W, l_base, l_q, brec, [&](int q, unsigned long long len, uint32_t d) {
            atomicAdd(&l_cov[q], len);
            dmax = dmax > d ? dmax : d;
        });
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const uint32_t x = (uint32_t)__shfl_xor((int)dmax, o, kWave);
            dmax = dmax > x ? dmax : x;
        }
        if (lane == 0 && dmax) atomicMax(&W.tmax, dmax);
    }
    __syncthreads();
    // the state of every (probe, rank): settled (-1, or 0 among the uncovered positions), or the rank among the covered ones
    for (int i = tid; i < cnt; i += WALK_THREADS) {
        const int q = i / K;
        const int2 qq = l_q[q];
        const long long L = (long long)qq.y - (long long)qq.x + (STRICT ? 0ll : 1ll);
        const long long k = ranks[r0 * K + i];
        uint32_t pf = DQT_NONE, rs = 0u;
        if (k >= 0 && k < L) {
            const long long unc = L - (long long)l_cov[q];
            if (k < unc) pf = DQT_ZERO;
            else { pf = 0u; rs = (uint32_t)(k - unc); }
        }
        W.prefix[i] = pf; W.res[i] = rs;
    }
    const uint32_t tmax = W.tmax;
    const int npass = (32 - __clz((int)tmax) + DQT_BITS - 1) / DQT_BITS;      // tmax = 0: no pass
    for (int p = npass - 1; p >= 0; --p) {
        const int shift = p * DQT_BITS;
        __syncthreads();                                   // covered[] and the previous pass's bins are read
        for (int i = tid; i < cnt * DQT_NB; i += WALK_THREADS) l_hist[i] = 0ull;
        // (the walk's first barrier publishes the zeros and the state)
        dqt_walk<STRICT>(T, cn, off, W, l_base, l_q, brec, [&](int q, unsigned long long len, uint32_t d) {
            const uint32_t hi = (uint32_t)((unsigned long long)d >> (shift + DQT_BITS));
            const int bin = (int)((d >> shift) & (uint32_t)(DQT_NB - 1));
            for (int j = 0; j < K; ++j)
                if (W.prefix[q * K + j] == hi) atomicAdd(&l_hist[(q * K + j) * DQT_NB + bin], len);
        });
        __syncthreads();
        for (int i = tid; i < cnt; i += WALK_THREADS) {
            const uint32_t pf = W.prefix[i];
            if (pf & 0x80000000u) continue;                // settled
            const unsigned long long rs = W.res[i];
            unsigned long long cum = 0;
            int t = 0;
            for (; t < DQT_NB - 1; ++t) {
                const unsigned long long c = l_hist[i * DQT_NB + t];
                if (cum + c > rs) break;
                cum += c;
            }
            W.res[i] = (uint32_t)(rs - cum);
            W.prefix[i] = (pf << DQT_BITS) | (uint32_t)t;
        }
    }
    __syncthreads();
    int32_t* o = out + r0 * K;
    for (int i = tid; i < cnt; i += WALK_THREADS) {
        const uint32_t pf = W.prefix[i];
        o[i] = pf == DQT_ZERO ? 0 : (int32_t)pf;           // DQT_NONE is -1
    }
}

}  // namespace ivj
