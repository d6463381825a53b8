// host_overlap_agg.hip.h -- driver of pb.map_overlaps (overlap_agg.hip.h): per value column gather -> reduce, over one probe
// bucketing, one set of flat tables and one gather of the build minima.
// Part of the single translation unit ivjoin.hip (included there, after host_thresh.hip.h and host_merge_agg.hip.h); not a stand-alone header.
#pragma once

namespace {

// sum and count are defined (0) where nothing can match; min / max / mean are unspecified there
int overlap_agg_zero(ivj_ctx* ctx, int64_t n, int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* outs) {
    for (int32_t k = 0; k < n_cols; ++k) {
        if (cols[k].ops & IVJ_AGG_SUM) HIP_TRY(hipMemsetAsync(outs[k].sum, 0, (size_t)n * 8, ctx->stream));
        if (cols[k].ops & IVJ_AGG_COUNT) HIP_TRY(hipMemsetAsync(outs[k].count, 0, (size_t)n * 8, ctx->stream));
    }
    return IVJ_OK;
}

template <class V>
AggOut<V> overlap_agg_out(uint32_t ops, const ivj_agg_out& o) {
    AggOut<V> out;
    out.sum = (ops & IVJ_AGG_SUM) ? (typename AggState<V>::Sum*)o.sum : nullptr;
    out.mn = (ops & IVJ_AGG_MIN) ? (V*)o.min : nullptr;
    out.mx = (ops & IVJ_AGG_MAX) ? (V*)o.max : nullptr;
    out.mean = (ops & IVJ_AGG_MEAN) ? o.mean : nullptr;
    out.count = (ops & IVJ_AGG_COUNT) ? (long long*)o.count : nullptr;
    return out;
}

// what the set-up leaves for the per-column passes of the same call (device pointers into the context's buffers)
struct OaggPlan {
    bool empty = true;                                    // nothing can match: no kernel runs, sum / count are zeroed
    const int32_t *qc = nullptr, *qs = nullptr, *qe = nullptr, *pos = nullptr;
    const uint32_t *probe_min = nullptr, *bm_sorted = nullptr;
    uint32_t min_overlap = 0;
    unsigned long long* vals = nullptr;                   // the value column in index order
    uint8_t* ok = nullptr;                                // ... and its validity bytes
    int64_t n = 0, tiles = 0;
    bool vec = false, strict = false, thresh = false;
};

// Set-up shared by the columns: tables, probe bucketing, arena scratch, the build minima in index order.  thr NULL: the plain predicate.
int overlap_agg_plan(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, const ivj_thresholds* thr, OaggPlan& P) {
    const int64_t n = probe->n;
    ctx->ov_n = -1;                                       // invalidates a pending count -> fill hand-over
    P = OaggPlan();
    P.n = n;
    if (!ix->has_tables) return fail(IVJ_ESTATE, "this index was built for merge / cluster only (with_end_order & 2): it has no lookup tables");
    if (n == 0 || ix->n == 0 || ix->n_contigs <= 0) return IVJ_OK;
    IVJ_TRY(need_tables(ctx, ix));
    IVJ_TRY(build_flat(ctx, ix));
    P.empty = false;
    P.tiles = (n + THRESH_TILE - 1) / THRESH_TILE;
    P.strict = opts->filter_op == IVJ_FILTER_STRICT;
    P.thresh = thr != nullptr;
    P.min_overlap = thr ? thr->min_overlap : 0u;
    P.probe_min = thr ? thr->probe_min : nullptr;
    P.qc = probe->contig; P.qs = probe->start; P.qe = probe->end;
    // large inputs: the probes bucketed by genomic position, as in thresh_count; pos = each bucketed probe's place in the caller's columns
    if (want_partition(ix, n, opts)) IVJ_TRY(bucket_probes(ctx, ix, probe, opts, &P.qc, &P.qs, &P.qe, &P.pos));
    const bool with_bm = thr && thr->build_min;
    IVJ_TRY(arena_reserve(ctx, align_up((size_t)ix->n * 8) + align_up((size_t)ix->n) + (with_bm ? align_up((size_t)ix->n * 4) : 0) + 4096));
    P.vals = arena_take<unsigned long long>(ctx, (size_t)ix->n);
    P.ok = arena_take<uint8_t>(ctx, (size_t)ix->n);
    if (with_bm) {
        uint32_t* bm = arena_take<uint32_t>(ctx, (size_t)ix->n);
        LAUNCH(ctx, "thresh_gather", k_thresh_gather, grid1d(ix->n, 256), 256, (const int32_t*)ix->b_row, thr->build_min, ix->n, ix->n, bm);
        P.bm_sorted = bm;
    }
    P.vec = aligned16(P.qc) && aligned16(P.qs) && aligned16(P.qe) && aligned16(P.pos);
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

// the value column and its validity bytes in index order (P.vals / P.ok)
int overlap_agg_gather(ivj_ctx* ctx, ivj_index* ix, const OaggPlan& P, const ivj_agg_in& in, int64_t n_values) {
    if (n_values > 0)
        LAUNCH(ctx, "overlap_agg_gather", k_oagg_gather, grid1d(ix->n, 256), 256, (const int32_t*)ix->b_row, (const unsigned long long*)in.values,
               in.valid, ix->n, n_values, P.vals, P.ok);
    else HIP_TRY(hipMemsetAsync(P.ok, 0, (size_t)ix->n, ctx->stream));        // no values: every row is out of range
    return IVJ_OK;
}

// One value column: gather -> reduce.  Device pointers; o.* hold P.n entries.  Enqueued on the context's stream.
int overlap_agg_col(ivj_ctx* ctx, ivj_index* ix, const OaggPlan& P, const ivj_agg_in& in, int64_t n_values, const ivj_agg_out& o) {
    if (P.n == 0) return IVJ_OK;
    if (P.empty) return overlap_agg_zero(ctx, P.n, 1, &in, &o);
    IVJ_TRY(overlap_agg_gather(ctx, ix, P, in, n_values));
    const int64_t grid = 8 * ((P.tiles + 7) / 8);
    IndexView v = view_of(ix);
    with_bool(P.strict, P.thresh, [&](auto S, auto T) {
        if (in.dtype == IVJ_AGG_I64)
            LAUNCH(ctx, "overlap_agg", (k_overlap_agg<S, T, IVJ_AGG_I64>), grid, THRESH_THREADS, v, P.qc, P.qs, P.qe, P.pos, P.n, P.vec, P.min_overlap,
                   P.probe_min, P.bm_sorted, (const long long*)P.vals, (const uint8_t*)P.ok, overlap_agg_out<long long>(in.ops, o));
        else
            LAUNCH(ctx, "overlap_agg", (k_overlap_agg<S, T, IVJ_AGG_F64>), grid, THRESH_THREADS, v, P.qc, P.qs, P.qe, P.pos, P.n, P.vec, P.min_overlap,
                   P.probe_min, P.bm_sorted, (const double*)P.vals, (const uint8_t*)P.ok, overlap_agg_out<double>(in.ops, o));
    });
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

// the argument checks both entries share; rows_present: value pointers must exist
int overlap_agg_check(const ivj_opts* opts, const ivj_side* probe, const ivj_thresholds* thr, int32_t n_cols, const ivj_agg_in* cols,
                      const ivj_agg_out* outs, bool rows_present) {
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe, "probe"));
    if (thr) IVJ_TRY(check_thresholds(thr));
    IVJ_TRY(check_agg_cols(n_cols, cols, rows_present));
    if (!outs) return fail(IVJ_EINVAL, "agg_out is NULL");
    if (probe->n > 0) IVJ_TRY(check_agg_outs(n_cols, cols, outs));
    return IVJ_OK;
}

// The host entries of the family: per value column the values (nb rows, + validity) go up, col(in, dev) enqueues the column's
// passes on device pointers, and the result columns that were asked for (n entries each) come down -- through one staging block,
// reused column after column.
template <class ColFn>
int agg_cols_host(ivj_ctx* ctx, int64_t n, int64_t nb, int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* agg_out, ColFn&& col) {
    const size_t col8 = align_up((size_t)n * 8), val8 = align_up((size_t)(nb + 1) * 8), val1 = align_up((size_t)nb + 1);
    DevBuf stage;
    hipError_t e = hipMalloc(&stage.p, val8 + val1 + 5 * col8);
    if (e != hipSuccess) return fail(IVJ_ENOMEM, std::string("hipMalloc(value and result columns): ") + hipGetErrorString(e));
    char* base = (char*)stage.p;
    void* d_val = base;
    uint8_t* d_valid = (uint8_t*)(base + val8);
    void* d_res[5];
    for (int r = 0; r < 5; ++r) d_res[r] = base + val8 + val1 + (size_t)r * col8;
    const ivj_agg_out dev{d_res[0], d_res[1], d_res[2], (double*)d_res[3], (int64_t*)d_res[4]};
    int rc = IVJ_OK;
    hipError_t ce = hipSuccess;
    {
        HostXfer copy(ctx->stream, &ctx->xfer);
        for (int32_t k = 0; k < n_cols && rc == IVJ_OK; ++k) {
            // the copies and the launches are ordered by the stream: column k + 1 overwrites the buffers after column k's copies left
            const bool with_valid = nb > 0 && cols[k].valid;
            if (nb > 0) copy.h2d(d_val, cols[k].values, (size_t)nb * 8);
            if (with_valid) copy.h2d(d_valid, cols[k].valid, (size_t)nb);
            const ivj_agg_in in{d_val, with_valid ? d_valid : nullptr, cols[k].dtype, cols[k].ops};
            rc = col(in, dev);
            const uint32_t ops = cols[k].ops;
            const ivj_agg_out& o = agg_out[k];
            if (ops & IVJ_AGG_SUM) copy.d2h(o.sum, dev.sum, (size_t)n * 8);
            if (ops & IVJ_AGG_MIN) copy.d2h(o.min, dev.min, (size_t)n * 8);
            if (ops & IVJ_AGG_MAX) copy.d2h(o.max, dev.max, (size_t)n * 8);
            if (ops & IVJ_AGG_MEAN) copy.d2h(o.mean, dev.mean, (size_t)n * 8);
            if (ops & IVJ_AGG_COUNT) copy.d2h(o.count, dev.count, (size_t)n * 8);
        }
        ce = copy.finish();
    }
    if (rc != IVJ_OK) return rc;
    if (ce != hipSuccess) return fail(IVJ_EHIP, std::string("copies(overlap aggregates): ") + hipGetErrorString(ce));
    return IVJ_OK;
}

}  // namespace
