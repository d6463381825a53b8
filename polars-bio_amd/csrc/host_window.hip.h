// host_window.hip.h -- drivers of the distance-window join and count (window.hip.h): count -> scan -> emit
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
#pragma once

namespace {

int check_window(const ivj_window* w) {
    if (!w) return fail(IVJ_EINVAL, "window is NULL");
    return IVJ_OK;
}

// what the count pass leaves for the emit pass of the same call (device pointers into the context's buffers)
struct WindowPlan {
    bool empty = true;                                    // nothing can match: no kernel ran
    const int32_t *qc = nullptr, *qs = nullptr, *qe = nullptr, *pos = nullptr, *row_id = nullptr;
    ivj_window win{0, 0, nullptr, nullptr, 0};
    long long* tile_tot = nullptr;                        // tiles + 1: exclusive scan of the tile totals, last = total
    int64_t n = 0, tiles = 0;
    bool vec = false, strict = false;
};

// the one launch of k_window: FORM is WIN_COUNT for the count pass, WIN_PAIRS / WIN_DIST (out_d non-NULL) for the emit pass
template <int FORM>
void window_launch(ivj_ctx* ctx, const char* name, ivj_index* ix, const WindowPlan& P, long long* tile_tot, long long* counts, int32_t* out_p,
                   int32_t* out_b, long long* out_d) {
    IndexView v = view_of(ix);
    with_bool(P.strict, [&](auto S) {
        LAUNCH(ctx, name, (k_window<S, FORM>), 8 * ((P.tiles + 7) / 8), WIN_THREADS, v, P.qc, P.qs, P.qe, P.pos, P.row_id, P.n, P.vec, P.win.left,
               P.win.right, P.win.probe_left, P.win.probe_right, P.win.min_distance, tile_tot, counts, out_p, out_b, out_d);
    });
}

// Count pass.  counts_dev (may be NULL): per-probe counts in probe input order.  want_pairs: also the tile totals, their scan and
// the grand total in *total (one 8-byte D2H); otherwise *total is not touched and nothing waits for the stream.
int window_count(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, const ivj_window* win, int64_t* counts_dev,
                 bool want_pairs, WindowPlan& P, int64_t* total) {
    const int64_t n = probe->n;
    ctx->ov_n = -1;                                       // invalidates a pending count -> fill hand-over
    if (want_pairs) *total = 0;
    P = WindowPlan();
    if (n == 0) return IVJ_OK;
    if (!ix->has_tables) return fail(IVJ_ESTATE, "this index was built for merge / cluster only (with_end_order & 2): it has no lookup tables");
    if (ix->n == 0 || ix->n_contigs <= 0) {
        if (counts_dev) HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)n * 8, ctx->stream));
        return IVJ_OK;
    }
    IVJ_TRY(need_tables(ctx, ix));
    IVJ_TRY(build_flat(ctx, ix));
    P.empty = false;
    P.n = n; P.tiles = (n + WIN_TILE - 1) / WIN_TILE;
    P.strict = opts->filter_op == IVJ_FILTER_STRICT;
    P.win = *win;
    P.qc = probe->contig; P.qs = probe->start; P.qe = probe->end; P.row_id = probe->row_id;
    // large inputs: the probes bucketed by genomic position; pos = each bucketed probe's place in the caller's columns, where its
    // extents are read and its count is written
    if (want_partition(ix, n, opts)) IVJ_TRY(bucket_probes(ctx, ix, probe, opts, &P.qc, &P.qs, &P.qe, &P.pos));
    const size_t tt_bytes = align_up((size_t)(P.tiles + 2) * 8), part_bytes = align_up((size_t)(scan_num_tiles(P.tiles) + 2) * 8);
    IVJ_TRY(arena_reserve(ctx, tt_bytes + part_bytes + 4096));
    P.tile_tot = arena_take<long long>(ctx, (size_t)P.tiles + 2);
    long long* partials = arena_take<long long>(ctx, (size_t)scan_num_tiles(P.tiles) + 2);
    P.vec = aligned16(P.qc) && aligned16(P.qs) && aligned16(P.qe) && aligned16(P.pos);
    window_launch<WIN_COUNT>(ctx, "overlap_window_count", ix, P, want_pairs ? P.tile_tot : (long long*)nullptr, (long long*)counts_dev, nullptr,
                             nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    if (!want_pairs) return IVJ_OK;
    device_scan<long long, SumOp, false>(ctx, "window_scan", P.tile_tot, P.tile_tot, P.tiles, 0ll, partials, P.tile_tot + P.tiles);
    HIP_TRY(hipMemcpyAsync(ctx->h_total, P.tile_tot + P.tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(wait_stream(ctx, ctx->stream));
    HIP_TRY(hipGetLastError());
    *total = *ctx->h_total;
    return IVJ_OK;
}

// Emit pass: exactly the counted pairs, tile after tile, into buffers that hold them.  out_d NULL: no distance column.
int window_emit(ivj_ctx* ctx, ivj_index* ix, const WindowPlan& P, int32_t* out_p, int32_t* out_b, int64_t* out_d) {
    if (P.empty) return IVJ_OK;
    if (out_d) window_launch<WIN_DIST>(ctx, "overlap_window_emit", ix, P, P.tile_tot, nullptr, out_p, out_b, (long long*)out_d);
    else window_launch<WIN_PAIRS>(ctx, "overlap_window_emit", ix, P, P.tile_tot, nullptr, out_p, out_b, nullptr);
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

int overlap_window_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, const ivj_window* win, int32_t* out_p,
                       int32_t* out_b, int64_t* out_d, int64_t capacity, int64_t* n_pairs) {
    WindowPlan P;
    IVJ_TRY(window_count(ctx, ix, probe, opts, win, nullptr, true, P, n_pairs));
    const int64_t total = *n_pairs;
    if (total == 0 || (capacity == 0 && !out_p && !out_b)) return IVJ_OK;            // nothing to write / count only
    if (total > capacity) return fail(IVJ_ECAPACITY, "output capacity " + std::to_string(capacity) + " < " + std::to_string(total) + " pairs");
    return window_emit(ctx, ix, P, out_p, out_b, out_d);
}

// both host entries: sides, per-row extents and index into HBM; dwin receives the device form of the window
struct WindowHost : JoinHost {
    DevMin pl, pr;
    ivj_window dwin{0, 0, nullptr, nullptr, 0};
};
int window_upload(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_window* win, WindowHost& H) {
    IVJ_TRY(upload_sides(ctx, probe, build, H));
    IVJ_TRY(upload_min(ctx, win->probe_left, probe->n, H.pl));
    IVJ_TRY(upload_min(ctx, win->probe_right, probe->n, H.pr));
    H.dwin = *win;
    H.dwin.probe_left = H.pl.p; H.dwin.probe_right = H.pr.p;
    return index_build(ctx, &H.db.s, opts, 0, &H.h.ix);
}

}  // namespace
