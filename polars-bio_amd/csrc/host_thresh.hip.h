// host_thresh.hip.h -- drivers of the thresholded overlap join and count (thresh.hip.h): count -> scan -> emit
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
#pragma once

namespace {

int check_thresholds(const ivj_thresholds* t) {
    if (!t) return fail(IVJ_EINVAL, "thresholds is NULL");
    if (t->min_overlap == 0 && !t->probe_min && !t->build_min)
        return fail(IVJ_EINVAL, "no threshold is set (min_overlap 0, probe_min and build_min NULL): use the plain entry points");
    return IVJ_OK;
}

// what the count pass leaves for the emit pass of the same call (device pointers into the context's buffers)
struct ThreshPlan {
    bool empty = true;                                    // nothing can match: no kernel ran
    const int32_t *qc = nullptr, *qs = nullptr, *qe = nullptr, *pos = nullptr, *row_id = nullptr;
    const uint32_t *probe_min = nullptr, *bm_sorted = nullptr;
    uint32_t min_overlap = 0;
    long long* tile_tot = nullptr;                        // tiles + 1: exclusive scan of the tile totals, last = total
    int64_t n = 0, tiles = 0;
    bool vec = false, strict = false;
};

// Count pass.  counts_dev (may be NULL): per-probe counts in probe input order.  want_pairs: also the tile totals, their scan and
// the grand total in *total (one 8-byte D2H); otherwise *total is not touched and nothing waits for the stream.
int thresh_count(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, const ivj_thresholds* thr, int64_t* counts_dev,
                 bool want_pairs, ThreshPlan& P, int64_t* total) {
    const int64_t n = probe->n;
    ctx->ov_n = -1;                                       // invalidates a pending count -> fill hand-over
    if (want_pairs) *total = 0;
    P = ThreshPlan();
    if (n == 0) return IVJ_OK;
    if (!ix->has_tables) return fail(IVJ_ESTATE, "this index was built for merge / cluster only (with_end_order & 2): it has no lookup tables");
    if (ix->n == 0 || ix->n_contigs <= 0) {
        if (counts_dev) HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)n * 8, ctx->stream));
        return IVJ_OK;
    }
    IVJ_TRY(need_tables(ctx, ix));
    IVJ_TRY(build_flat(ctx, ix));
    P.empty = false;
    P.n = n; P.tiles = (n + THRESH_TILE - 1) / THRESH_TILE;
    P.strict = opts->filter_op == IVJ_FILTER_STRICT;
    P.min_overlap = thr->min_overlap; P.probe_min = thr->probe_min;
    P.qc = probe->contig; P.qs = probe->start; P.qe = probe->end; P.row_id = probe->row_id;
    // large inputs: the probes bucketed by genomic position (the table and record reads of a tile then stay in the L2s); pos = each
    // bucketed probe's place in the caller's columns, where its minimum is read and its count is written
    if (want_partition(ix, n, opts)) IVJ_TRY(bucket_probes(ctx, ix, probe, opts, &P.qc, &P.qs, &P.qe, &P.pos));
    const size_t tt_bytes = align_up((size_t)(P.tiles + 2) * 8), part_bytes = align_up((size_t)(scan_num_tiles(P.tiles) + 2) * 8);
    IVJ_TRY(arena_reserve(ctx, tt_bytes + part_bytes + (thr->build_min ? align_up((size_t)ix->n * 4) : 0) + 4096));
    P.tile_tot = arena_take<long long>(ctx, (size_t)P.tiles + 2);
    long long* partials = arena_take<long long>(ctx, (size_t)scan_num_tiles(P.tiles) + 2);
    if (thr->build_min) {
        uint32_t* bm = arena_take<uint32_t>(ctx, (size_t)ix->n);
        LAUNCH(ctx, "thresh_gather", k_thresh_gather, grid1d(ix->n, 256), 256, (const int32_t*)ix->b_row, thr->build_min, ix->n, ix->n, bm);
        P.bm_sorted = bm;
    }
    P.vec = aligned16(P.qc) && aligned16(P.qs) && aligned16(P.qe) && aligned16(P.pos);
    IndexView v = view_of(ix);
    with_bool(P.strict, [&](auto S) {
        LAUNCH(ctx, "overlap_thresh_count", (k_overlap_thresh<S, false>), 8 * ((P.tiles + 7) / 8), THRESH_THREADS, v, P.qc, P.qs, P.qe, P.pos,
               P.row_id, n, P.vec, P.min_overlap, P.probe_min, P.bm_sorted, want_pairs ? P.tile_tot : (long long*)nullptr, (long long*)counts_dev,
               (int32_t*)nullptr, (int32_t*)nullptr);
    });
    HIP_TRY(hipGetLastError());
    if (!want_pairs) return IVJ_OK;
    device_scan<long long, SumOp, false>(ctx, "thresh_scan", P.tile_tot, P.tile_tot, P.tiles, 0ll, partials, P.tile_tot + P.tiles);
    HIP_TRY(hipMemcpyAsync(ctx->h_total, P.tile_tot + P.tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(wait_stream(ctx, ctx->stream));
    HIP_TRY(hipGetLastError());
    *total = *ctx->h_total;
    return IVJ_OK;
}

// Emit pass: exactly the counted pairs, tile after tile, into buffers that hold them.
int thresh_emit(ivj_ctx* ctx, ivj_index* ix, const ThreshPlan& P, int32_t* out_p, int32_t* out_b) {
    if (P.empty) return IVJ_OK;
    IndexView v = view_of(ix);
    with_bool(P.strict, [&](auto S) {
        LAUNCH(ctx, "overlap_thresh_emit", (k_overlap_thresh<S, true>), 8 * ((P.tiles + 7) / 8), THRESH_THREADS, v, P.qc, P.qs, P.qe, P.pos,
               P.row_id, P.n, P.vec, P.min_overlap, P.probe_min, P.bm_sorted, P.tile_tot, (long long*)nullptr, out_p, out_b);
    });
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

int overlap_thresh_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, const ivj_thresholds* thr, int32_t* out_p,
                       int32_t* out_b, int64_t capacity, int64_t* n_pairs) {
    ThreshPlan P;
    IVJ_TRY(thresh_count(ctx, ix, probe, opts, thr, nullptr, true, P, n_pairs));
    const int64_t total = *n_pairs;
    if (total == 0 || (capacity == 0 && !out_p && !out_b)) return IVJ_OK;            // nothing to write / count only
    if (total > capacity) return fail(IVJ_ECAPACITY, "output capacity " + std::to_string(capacity) + " < " + std::to_string(total) + " pairs");
    return thresh_emit(ctx, ix, P, out_p, out_b);
}

// host columns of minima -> HBM (NULL stays NULL)
struct DevMin {
    uint32_t* p = nullptr;
    ~DevMin() { if (p) (void)hipFree(p); }
};
int upload_min(ivj_ctx* ctx, const uint32_t* h, int64_t n, DevMin& d) {
    if (!h || n == 0) return IVJ_OK;
    hipError_t e = hipMalloc((void**)&d.p, (size_t)n * 4);
    if (e != hipSuccess) return fail(IVJ_ENOMEM, std::string("hipMalloc(minima): ") + hipGetErrorString(e));
    HostXfer copy(ctx->stream, &ctx->xfer);
    copy.h2d(d.p, h, (size_t)n * 4);
    HIP_TRY(copy.finish());
    return IVJ_OK;
}

// both host entries: sides, minima and index into HBM; dthr receives the device form of the thresholds
struct ThreshHost : JoinHost {
    DevMin pm, bm;
    ivj_thresholds dthr{0, nullptr, nullptr};
};
int thresh_upload(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr, ThreshHost& H) {
    IVJ_TRY(upload_sides(ctx, probe, build, H));
    IVJ_TRY(upload_min(ctx, thr->probe_min, probe->n, H.pm));
    IVJ_TRY(upload_min(ctx, thr->build_min, build->n, H.bm));
    H.dthr.min_overlap = thr->min_overlap; H.dthr.probe_min = H.pm.p; H.dthr.build_min = H.bm.p;
    // a side without rows brings no minima: what was a requirement on its rows constrains nothing
    if (H.dthr.min_overlap == 0 && !H.dthr.probe_min && !H.dthr.build_min) H.dthr.min_overlap = 1;
    return index_build(ctx, &H.db.s, opts, 0, &H.h.ix);
}

}  // namespace
