// host_overlap_quant.hip.h -- driver of pb.map_quantiles / pb.map_median (overlap_quant.hip.h): the set-up and the gather of
// pb.map_overlaps (overlap_agg_plan, overlap_agg_gather: tables, probe bucketing, the value column in index order), then one
// launch of k_overlap_quant.
// Part of the single translation unit ivjoin.hip (included there, after host_overlap_agg.hip.h); not a stand-alone header.
#pragma once

namespace {

// the argument checks both entries share; rows_present: the value pointer must exist
int overlap_quant_check(const ivj_opts* opts, const ivj_side* probe, const ivj_thresholds* thr, const ivj_agg_in* col, int32_t n_q,
                        const double* q, const void* out, bool rows_present) {
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe, "probe"));
    if (thr) IVJ_TRY(check_thresholds(thr));
    if (n_q < 1 || n_q > IVJ_MAX_OVQ_RANKS) return fail(IVJ_EINVAL, "n_q must be in 1 .. " + std::to_string(IVJ_MAX_OVQ_RANKS));
    if (!q) return fail(IVJ_EINVAL, "q is NULL");
    for (int32_t j = 0; j < n_q; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return fail(IVJ_EINVAL, "q[" + std::to_string(j) + "] is not in [0, 1]");
    if (!col) return fail(IVJ_EINVAL, "col is NULL");
    if (col->dtype != IVJ_AGG_I64 && col->dtype != IVJ_AGG_F64) return fail(IVJ_EINVAL, "value column: dtype must be IVJ_AGG_I64 or IVJ_AGG_F64");
    if (rows_present && !col->values) return fail(IVJ_EINVAL, "value column: values is NULL");
    if (probe->n > 0 && !out) return fail(IVJ_EINVAL, "out is NULL");
    return IVJ_OK;
}

// probes per workgroup
int overlap_quant_tile(int32_t n_q) {
    const int p = OVQ_MAXPK / (int)n_q;
    return p < 1 ? 1 : (p > IVJ_OVQ_MAX_TILE ? IVJ_OVQ_MAX_TILE : p);
}

// gather -> select on device pointers; out: P.n x n_q, count: P.n or NULL.  Enqueued on the context's stream.
int overlap_quant_col(ivj_ctx* ctx, ivj_index* ix, const OaggPlan& P, const ivj_agg_in& in, int64_t n_values, int32_t n_q, const double* q,
                      const uint8_t* upper, void* out, int64_t* count) {
    if (P.n == 0) return IVJ_OK;
    if (P.empty) {                                        // nothing can match: all-zero bits, count 0
        HIP_TRY(hipMemsetAsync(out, 0, (size_t)P.n * (size_t)n_q * 8, ctx->stream));
        if (count) HIP_TRY(hipMemsetAsync(count, 0, (size_t)P.n * 8, ctx->stream));
        return IVJ_OK;
    }
    IVJ_TRY(overlap_agg_gather(ctx, ix, P, in, n_values));
    OvqReq rq;
    std::memset(&rq, 0, sizeof(rq));
    for (int32_t j = 0; j < n_q; ++j) { rq.q[j] = q[j]; rq.upper[j] = (upper && upper[j]) ? 1 : 0; }
    const int rows = overlap_quant_tile(n_q);
    const size_t lds = (size_t)rows * (size_t)n_q * OVQ_NB * 4;
    const int64_t tiles = (P.n + rows - 1) / rows;
    const int64_t grid = 8 * ((tiles + 7) / 8);
    IndexView v = view_of(ix);
    const int rc = with_bool(P.strict, P.thresh, [&](auto S, auto T) -> int {
        auto launch = [&](auto kernel) -> int {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            LAUNCH_LDS(ctx, "overlap_quant", kernel, grid, THRESH_THREADS, lds, v, P.qc, P.qs, P.qe, P.pos, P.n, rows, (int)n_q, rq, P.min_overlap,
                       P.probe_min, P.bm_sorted, (const unsigned long long*)P.vals, (const uint8_t*)P.ok, (unsigned long long*)out, (long long*)count);
            return IVJ_OK;
        };
        if (in.dtype == IVJ_AGG_I64) return launch(&k_overlap_quant<S, T, IVJ_AGG_I64>);
        return launch(&k_overlap_quant<S, T, IVJ_AGG_F64>);
    });
    IVJ_TRY(rc);
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

}  // namespace
