// host_depth_hist.hip.h -- host driver of pb.depth_histogram / pb.genome_depth_histogram (depth_hist.hip.h): per probe row, or per
// contig, the number of positions at each depth 0 .. max_depth of the build side (the last bin: at least max_depth)
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
//
// Every call builds what the kernels read and releases it before it returns, as depth_query_dev does and with its steps 1 and 2:
// the depth blocks of the index (depth_core, with its slow path for a row with start > end), and for the region form an index of
// the blocks (index_build, sweep + end order: the joint grid) and their 16-byte records (k_dq_records; the level 0 of the depth
// tree it also writes is not read).  No tree above it, no planar maps and no threshold table: the cost does not depend on
// max_depth beyond the output itself.  NOTHING IS CACHED ON THE INDEX.
// partition_mode 0, 1 and 2 run the same probe-order kernel and return identical arrays.
#pragma once

namespace {

static_assert(DH_MAX_BINS == IVJ_MAX_HIST_DEPTH + 1, "the contig form's LDS histogram holds IVJ_MAX_HIST_DEPTH + 1 bins");
static_assert(WALK_TILE == IVJ_HIST_MAX_TILE, "a thread holds WALK_ITEMS probes of the tile");

// argument checks shared by all four entries, whatever the number of rows
int depth_hist_check(int32_t max_depth, const void* hist) {
    if (max_depth < 1 || max_depth > IVJ_MAX_HIST_DEPTH) return fail(IVJ_EINVAL, "max_depth must be in 1 .. " + std::to_string(IVJ_MAX_HIST_DEPTH));
    if (!hist) return fail(IVJ_EINVAL, "hist is NULL");
    return IVJ_OK;
}

// LDS bytes the region form's histograms may take: IVJ_HIST_LDS_BYTES; IVJ_HIST_LDS_KB = 64 .. 128 overrides it
// (tools/bench_depth_hist.py: two resident workgroups per CU against one)
size_t depth_hist_budget() {
    if (const char* ev = std::getenv("IVJ_HIST_LDS_KB")) {
        const int kb = std::atoi(ev);
        if (kb >= 64 && kb <= 128) return (size_t)kb * 1024;
    }
    return IVJ_HIST_LDS_BYTES;
}

// probes per workgroup of the region form
int depth_hist_tile(int32_t max_depth, size_t budget) {
    const size_t p = budget / ((size_t)(max_depth + 1) * 8);
    return (int)(p < 1 ? 1 : (p > (size_t)IVJ_HIST_MAX_TILE ? (size_t)IVJ_HIST_MAX_TILE : p));
}

// Steps 1 and 2 of a call of the region form, shared with host_depth_quant.hip.h: the depth blocks of the index, and (when there
// are any) the index of the blocks and their 16-byte records.  Everything is released with the object; the caller waits for the
// stream before that.
struct DepthBlocks {
    DevBuf own;
    IndexHolder h;
    int4* rec = nullptr;
    int64_t nb = 0;
    DqIndex v{nullptr, nullptr, nullptr, nullptr, 0};
};

int depth_blocks_build(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, DepthBlocks& B) {
    // 1. the blocks, library-owned
    int32_t *bc = nullptr, *bs = nullptr, *be = nullptr, *bd = nullptr;
    if (ix->n > 0) IVJ_TRY(depth_core(ctx, ix, opts, -1, &bc, &bs, &be, &bd, &B.own, &B.nb));
    // 2. their index and records (no blocks: every probe row of the dictionary is |Q| in bin 0)
    const int64_t nb = B.nb;
    B.v = DqIndex{nullptr, nullptr, nullptr, nullptr, ix->n_contigs};
    if (nb > 0) {
        const ivj_side blocks{bc, bs, be, nb, nullptr};
        ivj_opts o2 = *opts;
        o2.n_contigs = ix->n_contigs;
        o2.partition_mode = 0;
        IVJ_TRY(index_build(ctx, &blocks, &o2, 3, &B.h.ix));   // sweep only (no lookup tables) + the end order with the joint grid
        const int64_t pad0 = (nb + 15) & ~(int64_t)15;
        IVJ_TRY(arena_reserve(ctx, align_up((size_t)nb * 16) + align_up((size_t)pad0 * 4) + 4096));
        B.rec = arena_take<int4>(ctx, nb);
        int32_t* level0 = arena_take<int32_t>(ctx, pad0);
        LAUNCH(ctx, "depth_hist_records", k_dq_records, grid1d(pad0, 256), 256, (const int32_t*)bs, (const int32_t*)be, (const int32_t*)bd, nb, pad0, B.rec, level0);
        B.v = DqIndex{B.h.ix->cmeta_j, B.h.ix->crec, B.h.ix->b_start, B.h.ix->e_end, B.h.ix->n_contigs};
    }
    return IVJ_OK;
}

int depth_hist_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, int32_t D, int64_t* hist) {
    const int64_t n = probe->n;
    if (n == 0) return IVJ_OK;
    const bool strict = opts->filter_op == IVJ_FILTER_STRICT;
    DepthBlocks B;
    IVJ_TRY(depth_blocks_build(ctx, ix, opts, B));
    const int64_t nb = B.nb;
    const int4* rec = B.rec;
    const DqIndex v = B.v;
    // 3. the probes, P per workgroup
    const int P = depth_hist_tile(D, depth_hist_budget());
    const size_t lds = (size_t)P * (size_t)(D + 1) * 8;
    const int64_t tiles = (n + P - 1) / P;
    const int rc = with_bool(strict, nb > 0 && v.n_contigs <= CM_LDS, [&](auto S, auto LM) -> int {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_depth_hist<S, LM>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        LAUNCH_LDS(ctx, "depth_hist", (k_depth_hist<S, LM>), tiles, WALK_THREADS, lds, v, (int)(nb > 0), (const int4*)rec, probe->contig, probe->start, probe->end,
                   n, P, (int)D, (unsigned long long*)hist);
        return IVJ_OK;
    });
    IVJ_TRY(rc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));              // the blocks and their index are released on return
    return IVJ_OK;
}

int depth_hist_contigs_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int32_t D, int64_t* hist) {
    const int nc = ix->n_contigs;
    if (nc <= 0) return IVJ_OK;
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)nc * (size_t)(D + 1) * 8, ctx->stream));
    if (ix->n == 0) return IVJ_OK;
    const bool strict = opts->filter_op == IVJ_FILTER_STRICT;
    DevBuf own;
    int32_t *bc = nullptr, *bs = nullptr, *be = nullptr, *bd = nullptr;
    int64_t nb = 0;
    IVJ_TRY(depth_core(ctx, ix, opts, -1, &bc, &bs, &be, &bd, &own, &nb));
    if (nb == 0) return IVJ_OK;
    with_bool(strict, [&](auto S) {
        LAUNCH(ctx, "depth_hist_contigs", (k_depth_hist_contigs<S>), grid1d(nb, DH_CH), DH_THREADS, (const int32_t*)bc, (const int32_t*)bs, (const int32_t*)be,
               (const int32_t*)bd, nb, nc, (int)D, (unsigned long long*)hist);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));              // the blocks are released on return
    return IVJ_OK;
}

}  // namespace
