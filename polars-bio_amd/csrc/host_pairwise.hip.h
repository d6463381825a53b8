// host_pairwise.hip.h -- driver of pb.pairwise_jaccard (pairwise.hip.h): the segments of all frames by multi_core, reduced on the
// device into the two n_frames x n_frames matrices
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
#pragma once

namespace {

// bases_dev / runs_dev: n_frames * n_frames int64 each in HBM, row-major, full symmetric matrices (pairwise.hip.h); ix[f] NULL =
// an empty frame.  Waits for the stream: the segment list is released on return.
int pairwise_core(ivj_ctx* ctx, ivj_index* const* ix, int32_t n_frames, const ivj_opts* opts, int64_t* bases_dev, int64_t* runs_dev) {
    IVJ_TRY(multi_check(ix, n_frames, opts, 1, IVJ_MULTI_SEGMENTS));
    if (!bases_dev || !runs_dev) return fail(IVJ_EINVAL, "multi_pairwise: the output matrices are NULL");
    const size_t cells = (size_t)n_frames * (size_t)n_frames;
    HIP_TRY(hipMemsetAsync(bases_dev, 0, cells * 8, ctx->stream));
    HIP_TRY(hipMemsetAsync(runs_dev, 0, cells * 8, ctx->stream));
    DevBuf own;
    int32_t *s_contig = nullptr, *s_start = nullptr, *s_end = nullptr;
    unsigned long long* s_mask = nullptr;
    int64_t n_seg = 0;
    IVJ_TRY(multi_core(ctx, ix, n_frames, opts, 1, IVJ_MULTI_SEGMENTS, -1, &s_contig, &s_start, &s_end, &s_mask, &own, &n_seg));
    if (n_seg == 0) {                                        // every frame empty: the zero matrices
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return IVJ_OK;
    }
    const int64_t n_tiles = (n_seg + PW_TILE - 1) / PW_TILE;
    const int64_t cus = ctx->n_cus > 0 ? ctx->n_cus : 256;
    const int32_t n_parts = (int32_t)(n_tiles < cus ? n_tiles : cus);        // persistent: one workgroup per CU at most
    IVJ_TRY(arena_reserve(ctx, align_up((size_t)n_parts * PW_TRI * 8) + align_up((size_t)n_parts * PW_TRI * 4) + 4096));
    unsigned long long* part_bases = arena_take<unsigned long long>(ctx, (size_t)n_parts * PW_TRI);
    uint32_t* part_runs = arena_take<uint32_t>(ctx, (size_t)n_parts * PW_TRI);
    const char* ev = std::getenv("IVJ_PAIRWISE_THREADS");     // measurement: 256 = 4 wavefronts a workgroup instead of 16
    with_bool(opts->filter_op == IVJ_FILTER_STRICT, ev && std::atoi(ev) == 256, [&](auto S, auto FEW) {
        constexpr int THREADS = FEW ? 256 : PW_THREADS;
        LAUNCH(ctx, "pairwise_acc", (k_pairwise_acc<S, THREADS>), n_parts, THREADS, (const int32_t*)s_contig, (const int32_t*)s_start,
               (const int32_t*)s_end, (const unsigned long long*)s_mask, n_seg, n_tiles, part_bases, part_runs);
    });
    LAUNCH(ctx, "pairwise_fold", k_pairwise_fold, grid1d((int64_t)cells, PW_FOLD_THREADS), PW_FOLD_THREADS, (const unsigned long long*)part_bases,
           (const uint32_t*)part_runs, n_parts, n_frames, (long long*)bases_dev, (long long*)runs_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IVJ_OK;
}

}  // namespace
