// depth_hist.hip.h -- pb.depth_histogram / pb.genome_depth_histogram: the DISTRIBUTION of the build side's depth, per probe row
// (the region form: bedtools coverage -hist, mosdepth's dist) and per contig (the contig form: bedtools genomecov).
//
// With D = max_depth and bins = D + 1, over the depth blocks of the build side (depth.hip.h: disjoint, sorted per contig, depth >= 1):
//   region form   hist[q][min(depth, D)] += |block ∩ Q|  over the blocks [i0, i1) under probe q,  hist[q][0] = |Q| - the row's sum
//   contig form   hist[c][min(depth, D)] += |block|      over the blocks of contig c,             hist[c][0] = 0
// [i0, i1) is the exact block range of depth_query.hip.h (the two joint_rank lookups on the index of the blocks): every block of
// the range shares at least one position with the probe, so there is no candidate test, only the two edge clips
// min(bend, qend) - max(bstart, qstart) (+ 1 Weak), which leave the inner blocks whole.
//
// k_depth_hist, the region form.  A workgroup owns P consecutive probes and their P x bins uint64 histograms in LDS,
// P = floor(IVJ_HIST_LDS_BYTES / (bins * 8)) clamped to [1, IVJ_HIST_MAX_TILE].  The block ranges of the tile are laid out flat
// and walked with the candidate walk of cand_walk.hip.h (walk_offsets, walk_marks, the strided test loop), one block per lane,
// the "candidates" being the blocks of the exact range.  Neighbouring lanes hold neighbouring blocks;
// their depths usually differ, so two lanes rarely add to one address (the LDS unit serialises those that do: D = 1 puts every
// item of a probe on one address and stays correct).  A range may span any number of chunks.  After the walk bin 0 = |Q| - sum of the other bins, and the tile's P x bins block, contiguous in
// the row-major output, leaves as 16-byte stores.  No output is read back, no global atomic is used.
// LDS: the histograms are dynamic; beside them 8 KiB of per-probe {first block, offset, start, end} and 8 KiB shared in turn by
// the contig metadata (LM, range phase only) and the marks and scan words (walk phase only): 64 KiB + 16 KiB, so that two
// workgroups fit the CU's 160 KiB exactly.
// What bounds it: one 16-byte record and one LDS atomic per (row, block) incidence, plus n x bins x 8 bytes written.
//
// k_depth_hist_contigs, the contig form.  Tiles of DH_CH blocks against a zeroed table: a workgroup keeps one bins-entry LDS
// histogram for the contig of its first block; a block of a later contig (the tile that straddles a boundary, a dictionary of
// tiny contigs) goes straight to a global 64-bit atomicAdd; the non-zero LDS bins are flushed with one global atomicAdd each.
// Integer adds commute: the table is bit-identical from run to run.  What bounds it: 16 bytes read per block, and at most
// bins global atomics per tile plus one per block outside the tile's first contig.
#pragma once
#include "cand_walk.hip.h"
#include "depth_query.hip.h"

namespace ivj {

constexpr int DH_THREADS = 256, DH_CH = 2048;             // contig form: threads and blocks per workgroup
constexpr int DH_MAX_BINS = 1024;                            // = IVJ_MAX_HIST_DEPTH + 1
constexpr int DH_ROW_PER_THREAD_BINS = 16;                   // up to this many bins a thread sums a row, above a wavefront does

// the walk's words, and the contig metadata they share their LDS with
struct DhWalk {
    __align__(16) uint16_t marks[WALK_CH];
    int scan_i[WALK_WAVES];
    long long scan_ll[WALK_WAVES];
};
constexpr int DH_SCRATCH = 2 * CM_LDS * 16 > (int)sizeof(DhWalk) ? 2 * CM_LDS * 16 : (int)sizeof(DhWalk);

// the block range [i0, i1) of one probe on the index of the blocks: phases 1 and 2 of k_depth_query for a single row.
// m0 / m1: the contig's two joint-grid metadata words.
template <bool STRICT>
__device__ __forceinline__ void dh_range(const DqIndex& ix, const int4 m0, const int4 m1, int32_t s, int32_t e, int& i0, int& i1) {
    const int a = m0.x, b = m0.y;
    const uint32_t ulo = (uint32_t)m0.z, uhi = (uint32_t)m0.w;
    const unsigned long long te = (unsigned long long)flip(e) + (STRICT ? 0ull : 1ull);
    const unsigned long long ts = (unsigned long long)flip(s) + (STRICT ? 1ull : 0ull);
    const int he = (b <= a || te <= ulo) ? 0 : (te > uhi ? 1 : 2);          // 0: rank = a, 1: rank = b, 2: table
    const int hs = (b <= a || ts <= ulo) ? 0 : (ts > uhi ? 1 : 2);
    const uint32_t de = (uint32_t)te - ulo, ds = (uint32_t)ts - ulo, bmask = (1u << m1.x) - 1u;   // shift <= 31
    const uint32_t se = he == 2 ? (uint32_t)m1.y + (de >> m1.x) : 0u;
    const uint32_t ss = hs == 2 ? (uint32_t)m1.y + (ds >> m1.x) : 0u;
    const uint32_t oe = de & bmask, os = ds & bmask;
    const bool wide = m1.x > 16;
    int4 re = make_int4(0, 0, 0, 0), rs = make_int4(0, 0, 0, 0);
    if (he == 2) re = ix.crec[se];
    if (hs == 2) rs = (he == 2 && se == ss) ? re : ix.crec[ss];
    i1 = he == 0 ? a : (he == 1 ? b : joint_rank(ix.b_start, re.x, (uint32_t)re.z, oe, wide, te, b));
    i0 = hs == 0 ? a : (hs == 1 ? b : joint_rank(ix.e_end, rs.y, (uint32_t)rs.w, os, wide, ts, b));
}

// ix = the index of the BLOCKS, brec = their {start, end, depth, 0} records; have == 0: no blocks at all (ix holds the dictionary
// size only): every row is |Q| in bin 0.  P probes per workgroup, `dyn` bytes of dynamic LDS >= P * (D + 1) * 8.
// out: row-major n x (D + 1), 8-byte aligned.
template <bool STRICT, bool LM>
__global__ __launch_bounds__(WALK_THREADS) void k_depth_hist(DqIndex ix, int have, const int4* __restrict__ brec, const int32_t* __restrict__ pc,
                                                           const int32_t* __restrict__ ps, const int32_t* __restrict__ pe, int64_t n, int P, int D,
                                                           unsigned long long* __restrict__ out) {
    extern __shared__ __align__(16) unsigned long long l_hist[];
    __shared__ int l_lo[WALK_TILE];                          // first block of the probe
    __shared__ uint32_t l_off[WALK_TILE];                    // tile-local offset of its first item, modulo 2^32
    __shared__ int2 l_q[WALK_TILE];                          // {start, end}
    __shared__ __align__(16) unsigned char l_u[DH_SCRATCH];
    const int4* l_cm = reinterpret_cast<const int4*>(l_u);
    DhWalk& W = *reinterpret_cast<DhWalk*>(l_u);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const int bins = D + 1;
    const int64_t r0 = (int64_t)blockIdx.x * P;
    const int np = (int)((n - r0) < (int64_t)P ? (n - r0) : (int64_t)P);      // >= 1 by the grid
    const int cnt = np * bins;                                                // <= the LDS budget / 8
    for (int i = tid; i < cnt; i += WALK_THREADS) l_hist[i] = 0ull;
    if (LM && have) {
        int4* cm = reinterpret_cast<int4*>(l_u);
        for (int i = tid; i < 2 * ix.n_contigs; i += WALK_THREADS) cm[i] = ix.cmeta_j[i];
    }
    __syncthreads();
    // the block range and |Q| of every probe
    int cn[WALK_ITEMS];
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
        l_lo[q] = i0; l_q[q] = make_int2(s, e);
        if (ok) l_hist[q * bins] = (unsigned long long)((long long)e - (long long)s + (STRICT ? 0ll : 1ll));
    }
    __syncthreads();                                       // the contig metadata is read: its LDS turns into the walk's words
    long long T;
    long long off[WALK_ITEMS];
    walk_offsets(cn, W.scan_ll, off, T);
#pragma unroll
    for (int k = 0; k < WALK_ITEMS; ++k) l_off[tid * WALK_ITEMS + k] = (uint32_t)off[k];
    for (long long c0 = 0; c0 < T; c0 += WALK_CH) {
        const int nC = walk_chunk_len(T, c0);
        walk_marks(W.marks, W.scan_i, c0, nC, off, cn);   // (its first barrier publishes l_off)
        const uint32_t c0lo = (uint32_t)c0;
        for (int i = tid; i < nC; i += WALK_THREADS) {
            const WalkAt at = walk_probe(l_lo, l_off, W.marks, i, c0lo);
            const int2 qq = l_q[at.q];
            const int4 r = brec[at.p];                     // {start, end, depth, 0}
            const long long lo = qq.x > r.x ? qq.x : r.x, hi = qq.y < r.y ? qq.y : r.y;
            const int bin = r.z < 0 ? 0 : (r.z < D ? r.z : D);
            atomicAdd(&l_hist[at.q * bins + bin], (unsigned long long)(hi - lo + (STRICT ? 0ll : 1ll)));
        }
    }
    __syncthreads();
    // bin 0 holds |Q|: take the row's other bins off it
    if (bins <= DH_ROW_PER_THREAD_BINS) {
        for (int r = tid; r < np; r += WALK_THREADS) {
            unsigned long long sum = 0;
            for (int d = 1; d <= D; ++d) sum += l_hist[r * bins + d];
            l_hist[r * bins] -= sum;
        }
    } else {
        for (int r = w; r < np; r += WALK_WAVES) {
            unsigned long long sum = 0;
            for (int d = 1 + lane; d <= D; d += kWave) sum += l_hist[r * bins + d];
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, o, kWave);
            if (lane == 0) l_hist[r * bins] -= sum;
        }
    }
    __syncthreads();
    // the tile's block of the output: an 8-byte head where it starts off a 16-byte boundary, pairs, an 8-byte tail
    unsigned long long* o = out + r0 * (int64_t)bins;
    const int head = (int)((reinterpret_cast<uintptr_t>(o) >> 3) & 1u);       // <= cnt: cnt >= 2
    const int npairs = (cnt - head) >> 1;
    typedef unsigned long long v2u __attribute__((ext_vector_type(2)));
    for (int i = tid; i < npairs; i += WALK_THREADS) {
        v2u v; v.x = l_hist[head + 2 * i]; v.y = l_hist[head + 2 * i + 1];
        __builtin_nontemporal_store(v, reinterpret_cast<v2u*>(o + head + 2 * i));
    }
    if (tid == 0) {
        if (head) o[0] = l_hist[0];
        if ((cnt - head) & 1) o[cnt - 1] = l_hist[cnt - 1];
    }
}

// bc / bs / be / bd: the nb blocks in (contig, start) order; out: n_contigs x (D + 1), ZEROED by the host; DH_CH blocks per workgroup
template <bool STRICT>
__global__ __launch_bounds__(DH_THREADS) void k_depth_hist_contigs(const int32_t* __restrict__ bc, const int32_t* __restrict__ bs,
                                                                   const int32_t* __restrict__ be, const int32_t* __restrict__ bd, int64_t nb,
                                                                   int n_contigs, int D, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long l_h[DH_MAX_BINS];
    const int tid = threadIdx.x, bins = D + 1;
    const int64_t base = (int64_t)blockIdx.x * DH_CH;      // < nb by the grid
    for (int i = tid; i < bins; i += DH_THREADS) l_h[i] = 0ull;
    const int32_t c0 = bc[base];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < DH_CH / DH_THREADS; ++j) {
        const int64_t i = base + j * DH_THREADS + tid;
        if (i >= nb) break;
        const int32_t c = bc[i], d = bd[i];
        const unsigned long long len = (unsigned long long)((long long)be[i] - (long long)bs[i] + (STRICT ? 0ll : 1ll));
        const int bin = d < 0 ? 0 : (d < D ? d : D);
        if (c == c0) atomicAdd(&l_h[bin], len);
        else if ((uint32_t)c < (uint32_t)n_contigs) atomicAdd(&out[(size_t)c * bins + bin], len);
    }
    __syncthreads();
    if ((uint32_t)c0 >= (uint32_t)n_contigs) return;       // uniform
    for (int i = tid; i < bins; i += DH_THREADS) {
        const unsigned long long v = l_h[i];
        if (v) atomicAdd(&out[(size_t)c0 * bins + i], v);
    }
}

}  // namespace ivj
