// host_depth.hip.h -- driver of pb.depth (depth.hip.h): run-length coverage blocks of the indexed frame
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
#pragma once

namespace {

// Blocks of constant depth >= 1 of the index's rows, (contig id, start) order.  capacity < 0: library-allocated device
// outputs in *own (host path), otherwise the caller's buffers; *n_blocks always receives the total, nothing is written
// when it exceeds the capacity.  An index without the end order is completed here (build_end_order).
// sanitized: the index holds no dictionary row with start > end (the second level of the slow path below).
// runs: the maximal runs of depth >= 1 instead of the blocks (host_setop.hip.h); three columns, o_depth is not touched.
int depth_core(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int64_t capacity, int32_t** o_contig, int32_t** o_start, int32_t** o_end,
               int32_t** o_depth, DevBuf* own, int64_t* n_blocks, bool sanitized = false, bool runs = false) {
    const int64_t n = ix->n;
    const bool strict = opts->filter_op == IVJ_FILTER_STRICT;
    *n_blocks = 0;
    if (n == 0 || ix->n_contigs <= 0) return IVJ_OK;
    IVJ_TRY(build_end_order(ctx, ix));                       // before the arena is taken: it reserves for itself
    const int64_t n_tiles = (2 * n + DP_TILE - 1) / DP_TILE;
    const size_t words = align_up((size_t)(n_tiles + 2) * 4);
    IVJ_TRY(arena_reserve(ctx, 3 * words + align_up((size_t)(scan_num_tiles(n_tiles) + 2) * 4) + 4096));
    uint32_t* part = arena_take<uint32_t>(ctx, n_tiles + 2);
    uint32_t* cnt = arena_take<uint32_t>(ctx, n_tiles + 2);
    uint32_t* off = arena_take<uint32_t>(ctx, n_tiles + 2);
    uint32_t* partials = arena_take<uint32_t>(ctx, scan_num_tiles(n_tiles) + 2);
    uint32_t* total_dev = partials + scan_num_tiles(n_tiles) + 1;
    const int32_t *bc = ix->b_contig, *bs = ix->b_start, *ee = ix->e_end;
    with_bool(strict, runs, [&](auto S, auto R) {
        LAUNCH(ctx, "depth_partition", (k_depth_partition<S>), grid1d(n_tiles + 1, DP_THREADS), DP_THREADS, bc, bs, ee, n, n_tiles, part);
        LAUNCH(ctx, "depth_count", (k_depth_tile<S, false, R>), n_tiles, DP_THREADS, bc, bs, ee, n, ix->n_contigs, (const uint32_t*)part, cnt,
               (const uint32_t*)nullptr, 0u, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
    });
    device_scan<uint32_t, SumOp, false>(ctx, "depth_scan", cnt, off, n_tiles, 0u, partials, total_dev);
    // the total and the index's "some row has start > end" flag come back in one wait
    ctx->h_total[0] = 0; ctx->h_total[1] = 0;
    HIP_TRY(hipMemcpyAsync(ctx->h_total, total_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_total + 1, ix->flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipGetLastError());
    if (ctx->h_total[1] != 0) {
        // Slow path.  A row with start > end puts its "-1" before its "+1": the walk would report a negative depth between
        // the two.  Such rows cover nothing, so the frame is indexed again without them (and without zero-length rows and
        // rows outside the dictionary, which contribute nothing either) and the blocks are taken from that index.
        if (sanitized) return fail(IVJ_ESTATE, "depth: the re-indexed frame still holds a row with start > end");
        DevBuf cols;
        const size_t col = align_up((size_t)n * 4);
        hipError_t e = hipMalloc(&cols.p, 3 * col);
        if (e != hipSuccess) return fail(IVJ_ENOMEM, std::string("hipMalloc(depth rows): ") + hipGetErrorString(e));
        int32_t* c = (int32_t*)cols.p; int32_t* s = (int32_t*)((char*)cols.p + col); int32_t* en = (int32_t*)((char*)cols.p + 2 * col);
        with_bool(strict, [&](auto S) { LAUNCH(ctx, "depth_sanitize", (k_depth_sanitize<S>), grid1d(n, 256), 256, bc, bs, (const int2*)ix->ep, n, ix->n_contigs, c, s, en); });
        HIP_TRY(hipGetLastError());
        const ivj_side clean{c, s, en, n, nullptr};
        ivj_opts o2 = *opts;
        o2.n_contigs = ix->n_contigs;
        IndexHolder h;
        IVJ_TRY(index_build(ctx, &clean, &o2, 3, &h.ix));    // sweep only + end order
        const int rc = depth_core(ctx, h.ix, &o2, capacity, o_contig, o_start, o_end, o_depth, own, n_blocks, true, runs);
        HIP_TRY(hipStreamSynchronize(ctx->stream));          // the temporary index and columns are released on return
        return rc;
    }
    const int64_t total = (int64_t)(uint32_t)ctx->h_total[0];
    *n_blocks = total;
    if (total == 0) return IVJ_OK;
    if (runs) IVJ_TRY(place_outputs(total, capacity, {o_contig, o_start, o_end}, own, "setop", "runs"));
    else IVJ_TRY(place_outputs(total, capacity, {o_contig, o_start, o_end, o_depth}, own, "depth", "blocks", "depth "));
    with_bool(strict, runs, [&](auto S, auto R) {
        LAUNCH(ctx, "depth_fill", (k_depth_tile<S, true, R>), n_tiles, DP_THREADS, bc, bs, ee, n, ix->n_contigs, (const uint32_t*)part, (uint32_t*)nullptr,
               (const uint32_t*)off, (uint32_t)total, *o_contig, *o_start, *o_end, *o_depth);
    });
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

}  // namespace
