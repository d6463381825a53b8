// host_multi.hip.h -- driver of pb.multi_intersect / pb.consensus (multi.hip.h): union runs of every frame, one index over all
// runs, then the membership walk
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
#pragma once

namespace {

int multi_check(ivj_index* const* ix, int32_t n_frames, const ivj_opts* opts, int32_t min_frames, int32_t mode) {
    if (n_frames < 1 || n_frames > IVJ_MAX_FRAMES)
        return fail(IVJ_EINVAL, "multi_inter: n_frames must be in 1 .. " + std::to_string(IVJ_MAX_FRAMES) + ", got " + std::to_string(n_frames));
    if (!ix) return fail(IVJ_EINVAL, "multi_inter: the frame array is NULL");
    if (min_frames < 1 || min_frames > n_frames)
        return fail(IVJ_EINVAL, "multi_inter: min_frames must be in 1 .. n_frames (" + std::to_string(n_frames) + "), got " + std::to_string(min_frames));
    if (mode != IVJ_MULTI_SEGMENTS && mode != IVJ_MULTI_CONSENSUS) return fail(IVJ_EINVAL, "multi_inter: mode must be 0 (segments) or 1 (consensus)");
    for (int32_t f = 0; f < n_frames; ++f)
        if (ix[f] && ix[f]->n > 0 && ix[f]->n_contigs != opts->n_contigs)
            return fail(IVJ_EINVAL, "multi_inter: every index must be built over the contig dictionary of opts (n_contigs " +
                                        std::to_string(opts->n_contigs) + ", index of frame " + std::to_string(f) + ": " + std::to_string(ix[f]->n_contigs) + ")");
    return IVJ_OK;
}

// Segments (mode 0: maximal runs of one membership mask with >= min_frames bits) or consensus regions (mode 1: maximal runs
// covered by >= min_frames frames) of the frames ix[0 .. n_frames), NULL = an empty frame, in (contig id, start) order.
// capacity < 0: library-allocated device outputs in *own (host path), otherwise the caller's buffers; *n_out always receives
// the total, nothing is written when it exceeds the capacity.  o_mask is written for segments only.
int multi_core(ivj_ctx* ctx, ivj_index* const* ix, int32_t n_frames, const ivj_opts* opts, int32_t min_frames, int32_t mode, int64_t capacity,
               int32_t** o_contig, int32_t** o_start, int32_t** o_end, unsigned long long** o_mask, DevBuf* own, int64_t* n_out) {
    *n_out = 0;
    IVJ_TRY(multi_check(ix, n_frames, opts, min_frames, mode));
    const bool strict = opts->filter_op == IVJ_FILTER_STRICT;
    const bool consensus = mode == IVJ_MULTI_CONSENSUS;

    // 1. the union runs of every frame, concatenated in frame order
    std::vector<RunList> runs((size_t)n_frames);
    std::vector<uint32_t> h_off((size_t)n_frames + 1, 0u);
    int64_t n = 0;
    for (int32_t f = 0; f < n_frames; ++f) {
        IVJ_TRY(union_runs(ctx, ix[f], opts, runs[f]));
        n += runs[f].n;
        if (n > 0x3fffffffll) return fail(IVJ_EINVAL, "multi_inter: the frames hold more than 2^30 union runs");
        h_off[f + 1] = (uint32_t)n;
    }
    if (n == 0) return IVJ_OK;
    const size_t col = align_up((size_t)n * 4), tag_col = align_up((size_t)n), off_bytes = align_up(((size_t)n_frames + 1) * 4);
    DevBuf cat;
    hipError_t e = hipMalloc(&cat.p, 3 * col + 2 * tag_col + off_bytes);
    if (e != hipSuccess) return fail(IVJ_ENOMEM, std::string("hipMalloc(multi_inter runs): ") + hipGetErrorString(e));
    int32_t* c_contig = (int32_t*)cat.p;
    int32_t* c_start = (int32_t*)((char*)cat.p + col);
    int32_t* c_end = (int32_t*)((char*)cat.p + 2 * col);
    uint8_t* tag_a = (uint8_t*)cat.p + 3 * col;
    uint8_t* tag_e = tag_a + tag_col;
    uint32_t* run_off = (uint32_t*)(tag_e + tag_col);
    for (int32_t f = 0; f < n_frames; ++f) {
        if (runs[f].n == 0) continue;
        const size_t at = h_off[f], bytes = (size_t)runs[f].n * 4;
        HIP_TRY(hipMemcpyAsync(c_contig + at, runs[f].contig, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(c_start + at, runs[f].start, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(c_end + at, runs[f].end, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    {
        HostXfer copy(ctx->stream, &ctx->xfer);              // through the context's pinned staging, as every host copy of the driver
        copy.h2d(run_off, h_off.data(), ((size_t)n_frames + 1) * 4);
        HIP_TRY(copy.finish());
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));              // the per-frame run lists are released here
    runs.clear();

    // 2. one index over all runs: both event streams, sorted (a run covers at least one position: the fast path of depth_core)
    const ivj_side all{c_contig, c_start, c_end, n, nullptr};
    ivj_opts o2 = *opts;
    o2.partition_mode = 0;
    IndexHolder h;
    IVJ_TRY(index_build(ctx, &all, &o2, 3, &h.ix));          // sweep only + end order
    ivj_index* rx = h.ix;

    // 3. the walk
    const int64_t n_tiles = (2 * n + MI_TILE - 1) / MI_TILE;
    const size_t words = align_up((size_t)(n_tiles + 2) * 4), words64 = align_up((size_t)(n_tiles + 2) * 8);
    IVJ_TRY(arena_reserve(ctx, 3 * words + 2 * words64 + align_up((size_t)(scan_num_tiles(n_tiles) + 2) * 4) +
                                   align_up((size_t)(scan_num_tiles(n_tiles) + 2) * 8) + 4096));
    uint32_t* part = arena_take<uint32_t>(ctx, n_tiles + 2);
    uint32_t* cnt = arena_take<uint32_t>(ctx, n_tiles + 2);
    uint32_t* off = arena_take<uint32_t>(ctx, n_tiles + 2);
    unsigned long long* tile_x = arena_take<unsigned long long>(ctx, n_tiles + 2);
    unsigned long long* tile_m = arena_take<unsigned long long>(ctx, n_tiles + 2);
    uint32_t* partials = arena_take<uint32_t>(ctx, scan_num_tiles(n_tiles) + 2);
    unsigned long long* partials64 = arena_take<unsigned long long>(ctx, scan_num_tiles(n_tiles) + 2);
    uint32_t* total_dev = partials + scan_num_tiles(n_tiles) + 1;
    const int32_t *bc = rx->b_contig, *bs = rx->b_start, *ee = rx->e_end;
    LAUNCH(ctx, "multi_tags", k_multi_tags, grid1d(n, 256), 256, (const int32_t*)rx->b_row, (const int32_t*)rx->e_pos, n, (const uint32_t*)run_off, n_frames,
           tag_a, tag_e);
    with_bool(strict, [&](auto S) {
        LAUNCH(ctx, "multi_partition", (k_depth_partition<S>), grid1d(n_tiles + 1, DP_THREADS), DP_THREADS, bc, bs, ee, n, n_tiles, part);
    });
    LAUNCH(ctx, "multi_tile_xor", k_multi_tile_xor, n_tiles, MI_THREADS, (const uint8_t*)tag_a, (const uint8_t*)tag_e, n, (const uint32_t*)part, tile_x);
    device_scan<unsigned long long, XorOp, false>(ctx, "multi_xor_scan", tile_x, tile_m, n_tiles, 0ull, partials64, (unsigned long long*)nullptr);
    with_bool(strict, consensus, [&](auto S, auto C) {
        LAUNCH(ctx, "multi_count", (k_multi_tile<S, false, C>), n_tiles, MI_THREADS, bc, bs, ee, (const uint8_t*)tag_a, (const uint8_t*)tag_e, n, rx->n_contigs,
               min_frames, (const uint32_t*)part, (const unsigned long long*)tile_m, cnt, (const uint32_t*)nullptr, 0u, (int32_t*)nullptr, (int32_t*)nullptr,
               (int32_t*)nullptr, (unsigned long long*)nullptr);
    });
    device_scan<uint32_t, SumOp, false>(ctx, "multi_scan", cnt, off, n_tiles, 0u, partials, total_dev);
    ctx->h_total[0] = 0;
    HIP_TRY(hipMemcpyAsync(ctx->h_total, total_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipGetLastError());
    const int64_t total = (int64_t)(uint32_t)ctx->h_total[0];
    *n_out = total;
    if (total == 0) return IVJ_OK;
    if (capacity < 0) {
        const size_t ocol = align_up((size_t)total * 4);
        e = hipMalloc(&own->p, align_up((size_t)total * 8) + 3 * ocol);
        if (e != hipSuccess) return fail(IVJ_ENOMEM, std::string("hipMalloc(multi_inter regions): ") + hipGetErrorString(e));
        char* p = (char*)own->p;
        *o_mask = (unsigned long long*)p; p += align_up((size_t)total * 8);
        *o_contig = (int32_t*)p; *o_start = (int32_t*)(p + ocol); *o_end = (int32_t*)(p + 2 * ocol);
    } else {
        if (total > capacity)
            return fail(IVJ_ECAPACITY, "multi_inter output capacity " + std::to_string(capacity) + " < " + std::to_string(total) + " regions");
        if (!*o_contig || !*o_start || !*o_end || (!consensus && !*o_mask)) return fail(IVJ_EINVAL, "multi_inter output buffers are NULL");
    }
    with_bool(strict, consensus, [&](auto S, auto C) {
        LAUNCH(ctx, "multi_fill", (k_multi_tile<S, true, C>), n_tiles, MI_THREADS, bc, bs, ee, (const uint8_t*)tag_a, (const uint8_t*)tag_e, n, rx->n_contigs,
               min_frames, (const uint32_t*)part, (const unsigned long long*)tile_m, (uint32_t*)nullptr, (const uint32_t*)off, (uint32_t)total, *o_contig,
               *o_start, *o_end, *o_mask);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));              // the run index and the concatenation are released on return
    return IVJ_OK;
}

}  // namespace
