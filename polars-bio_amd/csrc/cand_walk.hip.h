// cand_walk.hip.h -- the candidate walk shared by the kernels that test (or fold) every candidate of every probe of a tile:
// k_overlap_flat, k_overlap_thresh, k_window, k_overlap_quant, k_depth_hist and k_depth_quant.  Small __device__ pieces only: each
// kernel still reads top to bottom as its own code and calls these steps.  oagg_chunk / oagg_tile (overlap_agg.hip.h: k_overlap_agg,
// k_overlap_wagg, k_signal_profile) walk by the same scheme but keep their own text of it: on these pieces k_overlap_agg measured
// 1.4 - 3.8 % slower than before ("Walk consolidation").
//
// THE SCHEME.  A workgroup of WALK_THREADS threads owns a tile of up to WALK_TILE probes, WALK_ITEMS consecutive ones per thread.
// Every probe has a range of cn consecutive records (candidates of flat_range, blocks of dh_range) that begins at record lo.  The
// ranges of the tile are laid end to end -- walk_offsets: an exclusive scan of the lengths gives every probe the tile-local offset
// `off` of its first candidate and the tile its total T -- and this flat space is walked in chunks of WALK_CH candidates
// (walk_chunk_len), one candidate per lane, so that a long range is spread over the whole workgroup and lanes of one probe read
// consecutive records.  A range may span any number of chunks; the last chunk of a tile is partial.
//
// THE MARKS map a candidate of the chunk to its probe (walk_marks): one uint16 per candidate, zeroed, then probe index + 1 written
// at the probe's first candidate of the chunk -- at slot 0 when the range began in an earlier chunk and reaches into this one --
// then an inclusive max-scan over the chunk (probe indices ascend with the offsets, so the maximum so far is the probe the
// candidate belongs to).  A thread scans the eight marks of its own 16-byte vector in registers, two per word, and the workgroup
// joins the threads with one block_exclusive_scan of the per-thread maxima.  Probes with an empty range write no mark.  Every
// candidate of a chunk lies at or after a mark, so marks[i] >= 1 for i < nC.
//
// FROM CANDIDATE TO RECORD (walk_probe).  Candidate i of the chunk that starts at c0 is record lo[q] + (c0 + i - off[q]) of its
// probe q.  Offsets are kept modulo 2^32 in LDS: the index inside one probe's range (< 2^31 records) is exact under that
// arithmetic however many candidates the tile has.  Kernels that need lo and off for nothing else store base = lo - off instead.
//
// Two shapes of the test loop: the strided one (candidate i = tid, tid + WALK_THREADS, ...) and the sub-range one (walk_sub:
// wavefront w takes the candidates [w * per, (w + 1) * per) of the chunk in ascending steps of 64), which keeps a wavefront's
// matches in candidate order -- what the staged pair output (walk_emit_chunk) and the per-probe counts (walk_count_heads) build on.
#pragma once
#include "index_view.hip.h"

namespace ivj {

constexpr int WALK_THREADS = 256;
constexpr int WALK_ITEMS = 2;                                // probes per thread
constexpr int WALK_TILE = WALK_THREADS * WALK_ITEMS;         // probes per workgroup
constexpr int WALK_CH = 2048;                                // candidates per chunk (one 16-byte mark vector per thread)
constexpr int WALK_WAVES = WALK_THREADS / kWave;
static_assert(WALK_CH * 2 == WALK_THREADS * 16, "one uint4 of marks per thread");
static_assert(WALK_TILE < 65535, "probe index + 1 must fit the 16-bit marks");
static_assert(WALK_THREADS == SCAN_THREADS, "block_exclusive_scan is written for SCAN_THREADS");

// The probe columns of a thread's N consecutive probes from i0 on, and at[] = pos[i0 ...] (pos NULL: the position itself).
template <int N>
__device__ __forceinline__ void load_probe_items(const int32_t* __restrict__ pc, const int32_t* __restrict__ ps, const int32_t* __restrict__ pe,
                                                 const int32_t* __restrict__ pos, int64_t i0, int64_t n, bool vec_ok, int32_t (&c)[N],
                                                 int32_t (&s)[N], int32_t (&e)[N], int32_t (&at)[N]) {
    load_items_nt(pc, i0, n, vec_ok, -1, c);
    load_items_nt(ps, i0, n, vec_ok, 0, s);
    load_items_nt(pe, i0, n, vec_ok, 0, e);
    if (pos) load_items(pos, i0, n, vec_ok, 0, at);
    else {
#pragma unroll
        for (int k = 0; k < N; ++k) at[k] = (int32_t)(i0 + k);
    }
}

// The tile's flat offsets: off[k] = tile-local offset of the first candidate of the thread's k-th probe, T = candidates of the
// tile (uniform).  scan_ll: WALK_WAVES words of LDS.  Two barriers (block_exclusive_scan).
template <int ITEMS>
__device__ __forceinline__ void walk_offsets(const int (&cn)[ITEMS], long long* scan_ll, long long (&off)[ITEMS], long long& T) {
    long long tsum = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) tsum += cn[k];
    off[0] = block_exclusive_scan(tsum, SumOp(), 0ll, scan_ll, &T);
#pragma unroll
    for (int k = 1; k < ITEMS; ++k) off[k] = off[k - 1] + cn[k - 1];
}

// for (long long c0 = 0; c0 < T; c0 += WALK_CH): the candidates of the chunk that starts at c0
__device__ __forceinline__ int walk_chunk_len(long long T, long long c0) {
    return (int)((T - c0) < (long long)WALK_CH ? (T - c0) : (long long)WALK_CH);
}

// The sub-range [wb, we) of this wavefront in a chunk of nC candidates: per = ceil(nC / WALK_THREADS) * 64 candidates per
// wavefront (wb + per <= WALK_CH: a staged index wb + rank stays inside the chunk arrays); empty (wb >= we) behind the chunk's end.
__device__ __forceinline__ int walk_per(int nC) { return ((nC + WALK_THREADS - 1) / WALK_THREADS) * kWave; }
struct WalkSub { int wb, we; };
__device__ __forceinline__ WalkSub walk_sub(int nC) {
    const int per = walk_per(nC), wb = (int)(threadIdx.x / kWave) * per;
    return {wb, (wb + per) < nC ? (wb + per) : nC};
}

// The candidate -> probe map of the chunk of nC <= WALK_CH candidates that starts at tile-local offset c0 (the marks of the header
// comment).  off / cn: the thread's probes' offsets (walk_offsets) and range lengths; scan_i: WALK_WAVES words of LDS.
// Uniform: every thread of the workgroup calls it.  The barrier contract:
//   the FIRST barrier publishes the LDS arrays the caller wrote before the call (the per-probe arrays before the first chunk) and
//   retires the previous chunk's use of marks and of whatever the caller staged beside them;
//   the LAST barrier publishes the marks.
template <int ITEMS>
__device__ __forceinline__ void walk_marks(uint16_t* marks, int* scan_i, long long c0, int nC, const long long (&off)[ITEMS],
                                           const int (&cn)[ITEMS]) {
    uint4* marks4 = reinterpret_cast<uint4*>(marks);
    __syncthreads();
    marks4[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        if (cn[k] == 0) continue;
        const long long rel = off[k] - c0;
        if (rel >= 0 && rel < (long long)nC) marks[rel] = (uint16_t)(threadIdx.x * ITEMS + k + 1);
        else if (rel < 0 && rel + cn[k] > 0) marks[0] = (uint16_t)(threadIdx.x * ITEMS + k + 1);
    }
    __syncthreads();
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
    uint32_t run = (uint32_t)block_exclusive_scan((int)tmax, MaxOp(), 0, scan_i, &tot);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t a = wd[j] & 0xffffu, b = wd[j] >> 16;
        run = run > a ? run : a;
        const uint32_t na = run;
        run = run > b ? run : b;
        wd[j] = na | (run << 16);
    }
    marks4[threadIdx.x] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    __syncthreads();
}

// Candidate i of the chunk whose offset is c0lo = (uint32_t)c0: its probe q and its record position p, for either LDS layout
// (lo + off, or base = lo - off).  valid == false (a lane behind the sub-range's end): probe 0, whose arrays are safe to read;
// p is then meaningless and must not be dereferenced.
struct WalkAt { int q, p; };
__device__ __forceinline__ int walk_probe_index(const uint16_t* marks, int i, bool valid) {
    const int q = valid ? (int)marks[i] - 1 : 0;
    return q < 0 ? 0 : q;                                  // (every candidate of a chunk lies at or after a mark)
}
__device__ __forceinline__ WalkAt walk_probe(const int* lo, const uint32_t* off, const uint16_t* marks, int i, uint32_t c0lo, bool valid = true) {
    const int q = walk_probe_index(marks, i, valid);
    return {q, lo[q] + (int)(c0lo + (uint32_t)i - off[q])};
}
__device__ __forceinline__ WalkAt walk_probe(const uint32_t* base, const uint16_t* marks, int i, uint32_t c0lo, bool valid = true) {
    const int q = walk_probe_index(marks, i, valid);
    return {q, (int)(base[q] + c0lo + (uint32_t)i)};
}

// One step of the sub-range loop, per-probe counts: mm = the ballot of the step's matches.  The candidates of one probe are
// consecutive lanes; the first of them (the segment's head) adds the segment's matches to the probe's LDS counter.  Uniform per
// wavefront.
__device__ __forceinline__ void walk_count_heads(uint32_t* cnt, int q, bool valid, unsigned long long mm) {
    if (mm == 0ull) return;                                // uniform
    const int lane = threadIdx.x & (kWave - 1);
    const int qseg = valid ? q : -1;
    const int qprev = __shfl_up(qseg, 1, kWave);
    const bool head = lane == 0 || qprev != qseg;
    const unsigned long long hb = __ballot(head);
    if (head && valid) {
        const unsigned long long above = hb & ~((2ull << lane) - 1ull);   // the heads after this one
        const unsigned long long upto = above ? ((above & (0ull - above)) - 1ull) : ~0ull;
        const int c = (int)__popcll(mm & upto & ~((1ull << lane) - 1ull));
        if (c) atomicAdd(&cnt[q], (uint32_t)c);
    }
}

// The wavefronts' totals through LDS (wtot: WALK_WAVES words): returns the workgroup's total (uniform), pre = the total of the
// wavefronts before this one.  cnt need be right in lane 0 only.  One barrier; a caller that writes wtot again must have passed
// another barrier since (the first one of walk_marks is one).
__device__ __forceinline__ long long walk_wave_prefix(long long* wtot, long long cnt, long long& pre) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    if (lane == 0) wtot[w] = cnt;
    __syncthreads();
    long long tot = 0;
    pre = 0;
#pragma unroll
    for (int k = 0; k < WALK_WAVES; ++k) { const long long x = wtot[k]; if (k < w) pre += x; tot += x; }
    return tot;
}

// The staged pair copy-out of a chunk of nC candidates.  The sub-range loop left the cnt matches of this wavefront in candidate
// order in the slots walk_sub(nC).wb + 0 .. cnt - 1 of the chunk arrays (marks recycled as the probe index of the staged pair: a
// rank never exceeds the index of the candidate, and the lanes of a step have read their marks before any of them writes).
// walk_emit_staged: store(slot, first + j) for the wavefront's j-th match.  walk_emit_chunk: the matches of the whole workgroup
// in candidate order -- store(slot, o) with o = the match's rank in the chunk -- and returns the chunk's total.  What a slot holds
// (the staged mark, the build row, further columns) is the caller's: store reads it.
template <class Store>
__device__ __forceinline__ void walk_emit_staged(int cnt, int nC, long long first, Store&& store) {
    const int lane = threadIdx.x & (kWave - 1), wb = (int)(threadIdx.x / kWave) * walk_per(nC);
    for (int j = lane; j < cnt; j += kWave) store(wb + j, first + j);
}
template <class Store>
__device__ __forceinline__ long long walk_emit_chunk(long long* wtot, int cnt, int nC, Store&& store) {
    long long cpre;
    const long long ctot = walk_wave_prefix(wtot, cnt, cpre);
    walk_emit_staged(cnt, nC, cpre, store);
    return ctot;
}

}  // namespace ivj
