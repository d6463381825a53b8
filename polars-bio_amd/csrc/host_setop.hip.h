// host_setop.hip.h -- driver of the set operations and their stats (setop.hip.h): union runs of both frames, then the set walk
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
#pragma once

namespace {

// truth table of an operation over the state in-U1 | in-U2 << 1 (bit s = state s belongs to the result); 0: no such operation
uint32_t setop_table(int32_t op) {
    switch (op) {
        case IVJ_SETOP_INTERSECTION: return 0x8u;            // {3}
        case IVJ_SETOP_UNION: return 0xeu;                   // {1, 2, 3}
        case IVJ_SETOP_DIFFERENCE: return 0x2u;              // {1}
        case IVJ_SETOP_SYMMETRIC_DIFFERENCE: return 0x6u;    // {1, 2}
    }
    return 0u;
}

// the union runs of one indexed frame, in a library allocation (ix == nullptr or an empty index: no runs)
struct RunList {
    DevBuf buf;
    int32_t *contig = nullptr, *start = nullptr, *end = nullptr;
    int64_t n = 0;
    SoStream stream() const { return SoStream{contig, start, end, 2 * n}; }
};
int union_runs(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, RunList& r) {
    if (!ix || ix->n == 0) return IVJ_OK;
    int32_t* no_depth = nullptr;
    return depth_core(ctx, ix, opts, -1, &r.contig, &r.start, &r.end, &no_depth, &r.buf, &r.n, false, true);
}

int setop_check_pair(const ivj_index* ix_a, const ivj_index* ix_b, const ivj_opts* opts) {
    for (const ivj_index* ix : {ix_a, ix_b})
        if (ix && ix->n > 0 && ix->n_contigs != opts->n_contigs)
            return fail(IVJ_EINVAL, "set operation: both indexes must be built over the contig dictionary of opts (n_contigs " +
                                        std::to_string(opts->n_contigs) + ", index " + std::to_string(ix->n_contigs) + ")");
    return IVJ_OK;
}

// Regions of op(U(a), U(b)) in (contig id, start) order.  capacity < 0: library-allocated device outputs in *own (host path),
// otherwise the caller's buffers; *n_regions always receives the total, nothing is written when it exceeds the capacity.
int setop_core(ivj_ctx* ctx, ivj_index* ix_a, ivj_index* ix_b, const ivj_opts* opts, int32_t op, int64_t capacity, int32_t** o_contig,
               int32_t** o_start, int32_t** o_end, DevBuf* own, int64_t* n_regions) {
    *n_regions = 0;
    const uint32_t table = setop_table(op);
    if (!table) return fail(IVJ_EINVAL, "set operation must be 0 (intersection), 1 (union), 2 (difference) or 3 (symmetric difference)");
    IVJ_TRY(setop_check_pair(ix_a, ix_b, opts));
    const bool strict = opts->filter_op == IVJ_FILTER_STRICT;
    RunList ra, rb;
    IVJ_TRY(union_runs(ctx, ix_a, opts, ra));
    IVJ_TRY(union_runs(ctx, ix_b, opts, rb));
    const SoStream sa = ra.stream(), sb = rb.stream();
    const int64_t events = sa.n + sb.n;
    if (events == 0) return IVJ_OK;
    const int64_t n_tiles = (events + SO_TILE - 1) / SO_TILE;
    const size_t words = align_up((size_t)(n_tiles + 2) * 4);
    IVJ_TRY(arena_reserve(ctx, 3 * words + align_up((size_t)(scan_num_tiles(n_tiles) + 2) * 4) + 4096));
    uint32_t* part = arena_take<uint32_t>(ctx, n_tiles + 2);
    uint32_t* cnt = arena_take<uint32_t>(ctx, n_tiles + 2);
    uint32_t* off = arena_take<uint32_t>(ctx, n_tiles + 2);
    uint32_t* partials = arena_take<uint32_t>(ctx, scan_num_tiles(n_tiles) + 2);
    uint32_t* total_dev = partials + scan_num_tiles(n_tiles) + 1;
    with_bool(strict, [&](auto S) {
        LAUNCH(ctx, "setop_partition", (k_so_partition<S>), grid1d(n_tiles + 1, SO_THREADS), SO_THREADS, sa, sb, n_tiles, part);
        LAUNCH(ctx, "setop_count", (k_so_tile<S, SO_COUNT>), n_tiles, SO_THREADS, sa, sb, table, (const uint32_t*)part, cnt, (const uint32_t*)nullptr, 0u,
               (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (unsigned long long*)nullptr);
    });
    device_scan<uint32_t, SumOp, false>(ctx, "setop_scan", cnt, off, n_tiles, 0u, partials, total_dev);
    ctx->h_total[0] = 0;
    HIP_TRY(hipMemcpyAsync(ctx->h_total, total_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipGetLastError());
    const int64_t total = (int64_t)(uint32_t)ctx->h_total[0];
    *n_regions = total;
    if (total == 0) return IVJ_OK;
    IVJ_TRY(place_outputs(total, capacity, {o_contig, o_start, o_end}, own, "setop", "regions", "setop "));
    with_bool(strict, [&](auto S) {
        LAUNCH(ctx, "setop_fill", (k_so_tile<S, SO_FILL>), n_tiles, SO_THREADS, sa, sb, table, (const uint32_t*)part, (uint32_t*)nullptr, (const uint32_t*)off,
               (uint32_t)total, *o_contig, *o_start, *o_end, (unsigned long long*)nullptr);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));              // the run lists are released on return
    return IVJ_OK;
}

// bases[0..2] = positions only U(a), only U(b), both cover; *n_intersections = regions of the intersection.  One walk, no regions written.
int set_stats_core(ivj_ctx* ctx, ivj_index* ix_a, ivj_index* ix_b, const ivj_opts* opts, int64_t bases[3], int64_t* n_intersections) {
    bases[0] = bases[1] = bases[2] = 0;
    *n_intersections = 0;
    IVJ_TRY(setop_check_pair(ix_a, ix_b, opts));
    const bool strict = opts->filter_op == IVJ_FILTER_STRICT;
    RunList ra, rb;
    IVJ_TRY(union_runs(ctx, ix_a, opts, ra));
    IVJ_TRY(union_runs(ctx, ix_b, opts, rb));
    const SoStream sa = ra.stream(), sb = rb.stream();
    const int64_t events = sa.n + sb.n;
    if (events == 0) return IVJ_OK;
    const int64_t n_tiles = (events + SO_TILE - 1) / SO_TILE;
    IVJ_TRY(arena_reserve(ctx, align_up((size_t)(n_tiles + 2) * 4) + align_up((size_t)n_tiles * SO_STAT_WORDS * 8) + align_up(SO_STAT_WORDS * 8) + 4096));
    uint32_t* part = arena_take<uint32_t>(ctx, n_tiles + 2);
    unsigned long long* tile_stats = arena_take<unsigned long long>(ctx, n_tiles * SO_STAT_WORDS);
    unsigned long long* sums = arena_take<unsigned long long>(ctx, SO_STAT_WORDS);
    with_bool(strict, [&](auto S) {
        LAUNCH(ctx, "setop_partition", (k_so_partition<S>), grid1d(n_tiles + 1, SO_THREADS), SO_THREADS, sa, sb, n_tiles, part);
        LAUNCH(ctx, "setop_stats", (k_so_tile<S, SO_STATS>), n_tiles, SO_THREADS, sa, sb, 0u, (const uint32_t*)part, (uint32_t*)nullptr, (const uint32_t*)nullptr, 0u,
               (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, tile_stats);
    });
    LAUNCH(ctx, "setop_reduce", k_so_reduce, 1, SO_THREADS, (const unsigned long long*)tile_stats, n_tiles, sums);
    HIP_TRY(hipMemcpyAsync(ctx->h_total, sums, SO_STAT_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < 3; ++k) bases[k] = (int64_t)ctx->h_total[k];
    *n_intersections = (int64_t)ctx->h_total[3];
    return IVJ_OK;
}

}  // namespace
