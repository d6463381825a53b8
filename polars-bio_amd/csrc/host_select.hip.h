// host_select.hip.h -- drivers of the semi / anti / left outer join kinds (select.hip.h): count per probe -> select
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
#pragma once

namespace {

int check_select_mode(int32_t mode) {
    if (mode != IVJ_SELECT_SEMI && mode != IVJ_SELECT_ANTI) return fail(IVJ_EINVAL, "mode must be IVJ_SELECT_SEMI (0) or IVJ_SELECT_ANTI (1)");
    return IVJ_OK;
}

// what the count pass leaves for the emit pass of the same call: pointers into the context's selection scratch (sel_buf), which
// no other driver touches -- the count kernels and the inner join of an outer join may use the arena in between
struct SelectPlan {
    bool empty = true;                 // no probe rows: no kernel ran
    bool wide = false;                 // the counts are int64 (thresholded count), else int32
    const void* counts = nullptr;
    long long* tile_tot = nullptr;     // tiles + 1: exclusive scan of the tile totals, last = the number of selected rows
    const int32_t* row_id = nullptr;
    int64_t n = 0, tiles = 0;
    int anti = 0;
};

int select_reserve(ivj_ctx* ctx, int64_t n, int64_t tiles) {
    const size_t need = align_up((size_t)n * 8) + align_up((size_t)(tiles + 2) * 8) + align_up((size_t)(scan_num_tiles(tiles) + 2) * 8);
    if (need <= ctx->sel_cap) return IVJ_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->sel_buf) HIP_TRY(hipFree(ctx->sel_buf));
    ctx->sel_buf = nullptr; ctx->sel_cap = 0;
    const size_t want = align_up(need + need / 8, 1 << 16);
    hipError_t e = hipMalloc((void**)&ctx->sel_buf, want);
    if (e != hipSuccess) return fail(IVJ_ENOMEM, std::string("selection scratch hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
    ctx->sel_cap = want;
    return IVJ_OK;
}

// Count pass: the per-probe counts of the existing count kernels into the selection scratch, the kept rows per tile, their scan and
// the number of selected rows in *n_rows (one 8-byte D2H).  thr NULL: the plain predicate (k_count_overlaps, int32 counts); otherwise
// the count form of k_overlap_thresh (int64 counts) -- with tp / n_pairs given it also leaves the plan and the total of the
// thresholded inner join (thresh_count with want_pairs), which the outer join emits from.
int select_count(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, const ivj_thresholds* thr, int32_t mode,
                 SelectPlan& S, int64_t* n_rows, ThreshPlan* tp = nullptr, int64_t* n_pairs = nullptr) {
    const int64_t n = probe->n;
    S = SelectPlan();
    *n_rows = 0;
    if (n_pairs) *n_pairs = 0;
    if (!ix->has_tables) return fail(IVJ_ESTATE, "this index was built for merge / cluster only (with_end_order & 2): it has no lookup tables");
    if (n == 0) return IVJ_OK;
    S.empty = false;
    S.n = n; S.tiles = (n + SELECT_TILE - 1) / SELECT_TILE;
    S.anti = mode == IVJ_SELECT_ANTI ? 1 : 0;
    S.row_id = probe->row_id;
    S.wide = thr != nullptr;
    IVJ_TRY(select_reserve(ctx, n, S.tiles));
    char* base = ctx->sel_buf;
    S.counts = base;
    S.tile_tot = reinterpret_cast<long long*>(base + align_up((size_t)n * 8));
    long long* partials = reinterpret_cast<long long*>(base + align_up((size_t)n * 8) + align_up((size_t)(S.tiles + 2) * 8));
    if (thr) {
        ThreshPlan local;
        IVJ_TRY(thresh_count(ctx, ix, probe, opts, thr, (int64_t*)base, tp != nullptr, tp ? *tp : local, n_pairs));
        LAUNCH(ctx, "select_count", (k_select_count<long long>), S.tiles, SELECT_THREADS, (const long long*)base, n, S.anti, S.tile_tot);
    } else {
        IVJ_TRY(count_overlaps_dev(ctx, ix, probe, opts, nullptr, (int32_t*)base));
        LAUNCH(ctx, "select_count", (k_select_count<int32_t>), S.tiles, SELECT_THREADS, (const int32_t*)base, n, S.anti, S.tile_tot);
    }
    HIP_TRY(hipGetLastError());
    device_scan<long long, SumOp, false>(ctx, "select_scan", S.tile_tot, S.tile_tot, S.tiles, 0ll, partials, S.tile_tot + S.tiles);
    HIP_TRY(hipMemcpyAsync(ctx->h_total, S.tile_tot + S.tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(wait_stream(ctx, ctx->stream));
    HIP_TRY(hipGetLastError());
    *n_rows = *ctx->h_total;
    return IVJ_OK;
}

// Emit pass: exactly the counted rows, ascending, into buffers that hold them; pad (may be NULL) receives -1 at the same positions.
int select_emit(ivj_ctx* ctx, const SelectPlan& S, int32_t* rows, int32_t* pad) {
    if (S.empty) return IVJ_OK;
    if (S.wide) {
        LAUNCH(ctx, "select_emit", (k_select_emit<long long>), S.tiles, SELECT_THREADS, (const long long*)S.counts, S.n, S.anti, S.row_id,
               (const long long*)S.tile_tot, rows, pad);
    } else {
        LAUNCH(ctx, "select_emit", (k_select_emit<int32_t>), S.tiles, SELECT_THREADS, (const int32_t*)S.counts, S.n, S.anti, S.row_id,
               (const long long*)S.tile_tot, rows, pad);
    }
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

int overlap_select_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, const ivj_thresholds* thr, int32_t mode,
                       int32_t* rows, int32_t* pad, int64_t capacity, int64_t* n_rows) {
    SelectPlan S;
    IVJ_TRY(select_count(ctx, ix, probe, opts, thr, mode, S, n_rows));
    const int64_t total = *n_rows;
    if (total == 0 || (capacity == 0 && !rows && !pad)) return IVJ_OK;               // nothing to write / count only
    if (total > capacity) return fail(IVJ_ECAPACITY, "output capacity " + std::to_string(capacity) + " < " + std::to_string(total) + " rows");
    return select_emit(ctx, S, rows, pad);
}

// sides (and minima) into HBM + the index; *dthr = the device form of the thresholds, NULL without any
struct SelectHost {
    ThreshHost H;
    const ivj_thresholds* dthr = nullptr;
};
int select_upload(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr, SelectHost& U) {
    if (thr) {
        IVJ_TRY(thresh_upload(ctx, probe, build, opts, thr, U.H));
        U.dthr = &U.H.dthr;
        return IVJ_OK;
    }
    return upload_join(ctx, probe, build, opts, 1, U.H);
}

}  // namespace
