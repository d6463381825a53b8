// host_signal.hip.h -- drivers of pb.signal_summary / pb.signal_profile (signal.hip.h): the set-up, gather and output block of
// host_overlap_agg.hip.h with the weighted kernels in place of k_overlap_agg.
// Part of the single translation unit ivjoin.hip (included there, after host_overlap_agg.hip.h); not a stand-alone header.
#pragma once

namespace {

// ---- overlap_wagg: probe rows -----------------------------------------------------------------------------------------------------

// overlap_agg_plan with the thresholded walk whatever thr says: without thresholds the effective minimum is 1
int overlap_wagg_plan(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, const ivj_thresholds* thr, OaggPlan& P) {
    IVJ_TRY(overlap_agg_plan(ctx, ix, probe, opts, thr, P));
    P.thresh = true;
    return IVJ_OK;
}

// One value column: gather -> weighted reduce.  Device pointers; o.* hold P.n entries, o.count receives the bases.
int overlap_wagg_col(ivj_ctx* ctx, ivj_index* ix, const OaggPlan& P, const ivj_agg_in& in, int64_t n_values, const ivj_agg_out& o) {
    if (P.n == 0) return IVJ_OK;
    if (P.empty) return overlap_agg_zero(ctx, P.n, 1, &in, &o);
    IVJ_TRY(overlap_agg_gather(ctx, ix, P, in, n_values));
    const int64_t grid = 8 * ((P.tiles + 7) / 8);
    IndexView v = view_of(ix);
    with_bool(P.strict, in.dtype == IVJ_AGG_I64, [&](auto S, auto I) {
        using V = typename std::conditional<decltype(I)::value, long long, double>::type;
        LAUNCH(ctx, "overlap_wagg", (k_overlap_wagg<S, decltype(I)::value ? IVJ_AGG_I64 : IVJ_AGG_F64>), grid, THRESH_THREADS, v, P.qc, P.qs, P.qe, P.pos, P.n,
               P.vec, P.min_overlap, P.probe_min, P.bm_sorted, (const V*)P.vals, (const uint8_t*)P.ok, overlap_agg_out<V>(in.ops, o));
    });
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

// sides (and minima) into HBM + the index; the thresholded walk needs no end order
int overlap_wagg_upload(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr, SelectHost& U) {
    if (thr) return select_upload(ctx, probe, build, opts, thr, U);
    return upload_join(ctx, probe, build, opts, 0, U.H);
}

// ---- signal_profile: the bins of the windows as probes ----------------------------------------------------------------------------

// The windows are read in their own order: opts->partition_mode is ignored, as by depth_profile.
int signal_profile_plan(ivj_ctx* ctx, ivj_index* ix, const ivj_side* windows, int32_t n_bins, const ivj_opts* opts, OaggPlan& P) {
    ctx->ov_n = -1;                                       // invalidates a pending count -> fill hand-over
    P = OaggPlan();
    P.n = windows->n * (int64_t)n_bins;                   // output elements
    if (!ix->has_tables) return fail(IVJ_ESTATE, "this index was built for merge / cluster only (with_end_order & 2): it has no lookup tables");
    if (windows->n == 0 || ix->n == 0 || ix->n_contigs <= 0) return IVJ_OK;
    P.tiles = (P.n + THRESH_TILE - 1) / THRESH_TILE;
    if (8 * ((P.tiles + 7) / 8) > 0x7fffffffll)
        return fail(IVJ_EINVAL, "signal_profile: " + std::to_string(windows->n) + " windows x " + std::to_string(n_bins) + " bins exceed one launch");
    IVJ_TRY(need_tables(ctx, ix));
    IVJ_TRY(build_flat(ctx, ix));
    P.empty = false;
    P.strict = opts->filter_op == IVJ_FILTER_STRICT;
    P.thresh = true;
    P.qc = windows->contig; P.qs = windows->start; P.qe = windows->end;
    IVJ_TRY(arena_reserve(ctx, align_up((size_t)ix->n * 8) + align_up((size_t)ix->n) + 4096));
    P.vals = arena_take<unsigned long long>(ctx, (size_t)ix->n);
    P.ok = arena_take<uint8_t>(ctx, (size_t)ix->n);
    return IVJ_OK;
}

// One value column over the n_windows x n_bins grid.  Device pointers; o.* hold P.n = n_windows * n_bins entries.
int signal_profile_col(ivj_ctx* ctx, ivj_index* ix, const OaggPlan& P, const uint8_t* reverse, int64_t n_windows, int32_t n_bins,
                       const ivj_agg_in& in, int64_t n_values, const ivj_agg_out& o) {
    if (P.n == 0) return IVJ_OK;
    if (P.empty) return overlap_agg_zero(ctx, P.n, 1, &in, &o);
    IVJ_TRY(overlap_agg_gather(ctx, ix, P, in, n_values));
    const int64_t grid = 8 * ((P.tiles + 7) / 8);
    IndexView v = view_of(ix);
    with_bool(P.strict, in.dtype == IVJ_AGG_I64, [&](auto S, auto I) {
        using V = typename std::conditional<decltype(I)::value, long long, double>::type;
        LAUNCH(ctx, "signal_profile", (k_signal_profile<S, decltype(I)::value ? IVJ_AGG_I64 : IVJ_AGG_F64>), grid, THRESH_THREADS, v, P.qc, P.qs, P.qe, reverse,
               n_windows, (int)n_bins, (const V*)P.vals, (const uint8_t*)P.ok, overlap_agg_out<V>(in.ops, o));
    });
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

// the argument checks both profile entries share; rows_present: value pointers must exist
int signal_profile_check(const ivj_opts* opts, const ivj_side* windows, int32_t n_bins, int32_t n_cols, const ivj_agg_in* cols,
                         const ivj_agg_out* outs, bool rows_present) {
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(windows, "windows"));
    IVJ_TRY(depth_profile_check(n_bins));
    IVJ_TRY(check_agg_cols(n_cols, cols, rows_present));
    if (!outs) return fail(IVJ_EINVAL, "agg_out is NULL");
    if (windows->n > 0) IVJ_TRY(check_agg_outs(n_cols, cols, outs));
    return IVJ_OK;
}

// Host buffers: the windows and the index travel once; the matrices in chunks of rows, so that the five result blocks of a column
// never take more than 5 x DPROF_CHUNK_BYTES of device memory (the value column is sent again per chunk).
int signal_profile_host(ivj_ctx* ctx, const ivj_side* windows, const uint8_t* reverse, int32_t n_bins, const ivj_side* build,
                        const ivj_opts* opts, int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* agg_out) {
    JoinHost J;
    DevBuf rev;
    IVJ_TRY(profile_upload(ctx, windows, reverse, build, opts, J, rev));
    const int64_t n = windows->n, nb = build->n;
    const size_t row_bytes = (size_t)n_bins * 8;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(DPROF_CHUNK_BYTES / row_bytes)));
    std::vector<ivj_agg_out> part_out((size_t)n_cols);
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        ivj_side part = J.dp.s;
        part.contig += r0; part.start += r0; part.end += r0; part.n = m;
        const uint8_t* prev = reverse ? (const uint8_t*)rev.p + r0 : nullptr;
        const size_t at = (size_t)r0 * (size_t)n_bins;
        for (int32_t k = 0; k < n_cols; ++k) {
            const ivj_agg_out& o = agg_out[k];
            part_out[k] = ivj_agg_out{o.sum ? (char*)o.sum + at * 8 : nullptr, o.min ? (char*)o.min + at * 8 : nullptr,
                                      o.max ? (char*)o.max + at * 8 : nullptr, o.mean ? o.mean + at : nullptr, o.count ? o.count + at : nullptr};
        }
        OaggPlan P;
        IVJ_TRY(signal_profile_plan(ctx, J.h.ix, &part, n_bins, opts, P));
        IVJ_TRY(agg_cols_host(ctx, P.n, nb, n_cols, cols, part_out.data(), [&](const ivj_agg_in& in, const ivj_agg_out& dev) {
            return signal_profile_col(ctx, J.h.ix, P, prev, m, n_bins, in, nb, dev);
        }));
    }
    return IVJ_OK;
}

}  // namespace
