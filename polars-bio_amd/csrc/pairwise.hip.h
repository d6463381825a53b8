// pairwise.hip.h -- pb.pairwise_jaccard: the F x F similarity matrices of F interval frames, reduced from the segment list of
// multi.hip.h (IVJ_MULTI_SEGMENTS, min_frames = 1) where it lies in HBM.
//
// A segment t is (contig, start, end, mask m_t); len_t = the positions it covers (64-bit: a Weak segment [INT32_MIN, INT32_MAX] has
// 2^32).  a_t = 1 iff segment t - 1 lies on the same contig and ends exactly where t begins (contig AND position, the position in
// 64 bits: a Weak end INT32_MAX + 1 is 2^31, not INT32_MIN).  With p_t = a_t ? m_t & m_{t-1} : 0, for every pair i <= j:
//   bases[i][j] = sum_t len_t [i, j in m_t]                       positions both frames cover (the diagonal: |U(frame i)|)
//   runs[i][j]  = sum_t [i, j in m_t] - [i, j in p_t]             maximal runs of U(i) & U(j) (a run starts where the pair enters)
// p_t is a subset of m_t, so a segment adds 0 or 1 to a runs entry: the partial sums never go below zero and fit 32 bits (at most
// one per segment, at most 2^31 segments).
//
// Layout (k_pairwise_acc).  A segment costs p (p + 1) / 2 updates for a mask of p bits against 20 bytes read: nothing here waits
// for HBM, the accumulators live in LDS and are laid out for the adds.  A workgroup holds ONE upper triangle -- 2080 int64 for
// bases, 2080 uint32 for runs, 24.4 KiB -- that all of its wavefronts add into with the LDS's own read-modify-write
// instructions (ds_add_u64 / ds_add_u32, no value returned): the LDS executes one wave-instruction at a time, so adds of two
// wavefronts never meet, a private copy per wavefront would issue the same instructions, and the shared triangle leaves room
// for 16 wavefronts a CU (four per SIMD) to cover each other's issue latency instead of the four that private copies would fit.
// A wavefront step loads 64 segments, one per lane (with segment t - 1 of every lane straight from HBM: the seams between steps,
// tiles and workgroups need no special case), and takes them one by one, wave-uniform (v_readlane).  Lane j owns column j: a
// scalar loop over the set bits i of the mask issues one ds_add_u64 at [i][j] for the lanes with bit j set and j >= i, and one
// ds_add_u32 for those of them whose pair is not in p_t.  Row i of the triangle is contiguous, so the 64 lanes of an add touch
// consecutive addresses: no bank conflict.
//
// Grid.  Persistent: at most one workgroup per CU and never more than there are tiles of PW_TILE segments; a workgroup strides
// over the tiles and writes its triangles as one partial pair to the arena.  k_pairwise_fold sums the partials in workgroup
// order and writes both halves of the full n_frames x n_frames matrices.  Integer sums (the order of integer adds does not
// change them): identical from run to run.
#pragma once
#include "multi.hip.h"

namespace ivj {

constexpr int PW_STEP = kWave;                       // segments of one wavefront step: one per lane
constexpr int PW_THREADS = 1024;                     // 16 wavefronts; IVJ_PAIRWISE_THREADS=256 runs the tiles with 4 (measurement)
constexpr int PW_TILE = 1024;                        // segments of one workgroup tile: PW_TILE / PW_STEP wavefront steps
constexpr int PW_FOLD_THREADS = 256;
constexpr int PW_TRI = MI_MAX_FRAMES * (MI_MAX_FRAMES + 1) / 2;      // entries of the upper triangle, diagonal included
static_assert(PW_STEP == 64 && MI_MAX_FRAMES == 64, "lane j owns column j of a 64-column triangle");
static_assert(PW_TILE % PW_STEP == 0, "a tile is whole wavefront steps");

// entry (i, j), 0 <= i <= j <= 63, of the packed upper triangle: row i begins at 64 i - i (i - 1) / 2, entry j lies j - i behind
__host__ __device__ __forceinline__ uint32_t pw_tri(uint32_t i, uint32_t j) { return ((i * (127u - i)) >> 1) + j; }

// the 64-bit value of lane k (wave-uniform k) as a scalar
__device__ __forceinline__ unsigned long long pw_readlane(unsigned long long v, int k) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), k);
    return ((unsigned long long)hi << 32) | lo;
}

// part_bases / part_runs: gridDim.x triangles of PW_TRI entries, one per workgroup
template <bool STRICT, int THREADS>
__global__ __launch_bounds__(THREADS) void k_pairwise_acc(const int32_t* __restrict__ s_contig, const int32_t* __restrict__ s_start,
                                                            const int32_t* __restrict__ s_end, const unsigned long long* __restrict__ s_mask,
                                                            int64_t n_seg, int64_t n_tiles, unsigned long long* __restrict__ part_bases,
                                                            uint32_t* __restrict__ part_runs) {
    __shared__ unsigned long long l_bases[PW_TRI];
    __shared__ uint32_t l_runs[PW_TRI];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int k = tid; k < PW_TRI; k += THREADS) {
        l_bases[k] = 0ull;
        l_runs[k] = 0u;
    }
    __syncthreads();

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        for (int step = wave; step < PW_TILE / PW_STEP; step += THREADS / kWave) {
            const int64_t t0 = tile * PW_TILE + (int64_t)step * PW_STEP;     // wave-uniform
            if (t0 >= n_seg) break;
            const int64_t left = n_seg - t0;
            const int cnt = left < PW_STEP ? (int)left : PW_STEP;
            const int64_t t = t0 + lane;
            unsigned long long v_mask = 0, v_prev = 0, v_len = 0;
            if (lane < cnt) {
                const long long s = s_start[t], e = s_end[t];
                v_mask = s_mask[t];
                v_len = (unsigned long long)(STRICT ? e - s : e - s + 1);
                if (t > 0) {
                    const long long pe = (long long)s_end[t - 1] + (STRICT ? 0 : 1);
                    if (s_contig[t - 1] == s_contig[t] && pe == s) v_prev = v_mask & s_mask[t - 1];
                }
            }
            for (int k = 0; k < cnt; ++k) {
                unsigned long long m = pw_readlane(v_mask, k);
                const unsigned long long p = pw_readlane(v_prev, k), len = pw_readlane(v_len, k);
                const bool in_m = (m >> lane) & 1ull, in_p = (p >> lane) & 1ull;
                while (m) {
                    const uint32_t i = (uint32_t)__builtin_ctzll(m);        // the row: wave-uniform
                    m &= m - 1;
                    if (in_m && (uint32_t)lane >= i) {
                        const uint32_t at = pw_tri(i, (uint32_t)lane);      // < PW_TRI: i <= lane <= 63
                        atomicAdd(l_bases + at, len);
                        if (!(in_p && ((p >> i) & 1ull))) atomicAdd(l_runs + at, 1u);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < PW_TRI; k += THREADS) {
        part_bases[(size_t)blockIdx.x * PW_TRI + k] = l_bases[k];
        part_runs[(size_t)blockIdx.x * PW_TRI + k] = l_runs[k];
    }
}

// bases / runs: n_frames x n_frames int64, row-major; entry (i, j) and (j, i) from the triangle's (min, max)
__global__ __launch_bounds__(PW_FOLD_THREADS) void k_pairwise_fold(const unsigned long long* __restrict__ part_bases, const uint32_t* __restrict__ part_runs,
                                                             int32_t n_parts, int32_t n_frames, long long* __restrict__ bases,
                                                             long long* __restrict__ runs) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_frames * n_frames) return;
    const int r = idx / n_frames, c = idx - r * n_frames;
    const uint32_t at = r <= c ? pw_tri((uint32_t)r, (uint32_t)c) : pw_tri((uint32_t)c, (uint32_t)r);
    unsigned long long b = 0, n = 0;
    for (int32_t g = 0; g < n_parts; ++g) {
        b += part_bases[(size_t)g * PW_TRI + at];
        n += part_runs[(size_t)g * PW_TRI + at];
    }
    bases[idx] = (long long)b;
    runs[idx] = (long long)n;
}

}  // namespace ivj
