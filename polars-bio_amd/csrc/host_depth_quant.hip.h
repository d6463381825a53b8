// host_depth_quant.hip.h -- host driver of pb.depth_quantiles / pb.median_depth (depth_quant.hip.h): per probe row and per requested
// rank the order statistic of the build side's depth over the row's positions
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
//
// Every call builds what the kernel reads and releases it before it returns, with steps 1 and 2 of depth_hist_dev as they are
// (depth_blocks_build: the depth blocks of the index, an index of the blocks, their 16-byte records).  No histogram leaves the
// device and nothing grows with the depth.  NOTHING IS CACHED ON THE INDEX.
// partition_mode 0, 1 and 2 run the same probe-order kernel and return identical arrays.
#pragma once

namespace {

// argument checks shared by both entries, whatever the number of rows
int depth_quant_check(int32_t n_ranks, const void* ranks, const void* out) {
    if (n_ranks < 1 || n_ranks > IVJ_MAX_QUANT_RANKS) return fail(IVJ_EINVAL, "n_ranks must be in 1 .. " + std::to_string(IVJ_MAX_QUANT_RANKS));
    if (!ranks) return fail(IVJ_EINVAL, "ranks is NULL");
    if (!out) return fail(IVJ_EINVAL, "out is NULL");
    return IVJ_OK;
}

// probes per workgroup
int depth_quant_tile(int32_t n_ranks) {
    const size_t p = (size_t)IVJ_QUANT_LDS_BYTES / ((size_t)n_ranks * DQT_NB * 8);
    return (int)(p < 1 ? 1 : (p > (size_t)IVJ_QUANT_MAX_TILE ? (size_t)IVJ_QUANT_MAX_TILE : p));
}

int depth_quant_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, int32_t K, const int64_t* ranks, int32_t* out) {
    const int64_t n = probe->n;
    if (n == 0) return IVJ_OK;
    const bool strict = opts->filter_op == IVJ_FILTER_STRICT;
    DepthBlocks B;
    IVJ_TRY(depth_blocks_build(ctx, ix, opts, B));
    const int P = depth_quant_tile(K);
    const size_t lds = (size_t)P * (size_t)K * DQT_NB * 8;
    const int64_t tiles = (n + P - 1) / P;
    const int rc = with_bool(strict, B.nb > 0 && B.v.n_contigs <= CM_LDS, [&](auto S, auto LM) -> int {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_depth_quant<S, LM>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        LAUNCH_LDS(ctx, "depth_quant", (k_depth_quant<S, LM>), tiles, WALK_THREADS, lds, B.v, (int)(B.nb > 0), (const int4*)B.rec, probe->contig, probe->start,
                   probe->end, n, P, (int)K, ranks, out);
        return IVJ_OK;
    });
    IVJ_TRY(rc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));              // the blocks and their index are released on return
    return IVJ_OK;
}

}  // namespace
