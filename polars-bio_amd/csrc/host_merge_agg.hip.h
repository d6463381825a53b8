// host_merge_agg.hip.h -- driver of the per-cluster aggregates of pb.merge(agg=...) (merge_agg.hip.h)
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
#pragma once

namespace {

constexpr uint32_t AGG_ALL_OPS = IVJ_AGG_SUM | IVJ_AGG_MIN | IVJ_AGG_MAX | IVJ_AGG_MEAN | IVJ_AGG_COUNT;

inline int64_t magg_num_tiles(int64_t n) { return (n + MAGG_TILE - 1) / MAGG_TILE; }
// arena bytes of the tile parts (both state types are 32 bytes); goes into cluster_core's extra_bytes
size_t merge_agg_bytes(int64_t n) { return align_up((size_t)(2 * magg_num_tiles(n) + 1) * sizeof(AggState<double>)); }
static_assert(sizeof(AggState<double>) == 32 && sizeof(AggState<long long>) == 32, "merge_agg_bytes assumes 32-byte states");

int check_agg_cols(int32_t n_cols, const ivj_agg_in* cols, bool rows_present) {
    if (n_cols < 1 || n_cols > IVJ_MAX_AGG_COLS) return fail(IVJ_EINVAL, "n_cols must be in [1, " + std::to_string(IVJ_MAX_AGG_COLS) + "]");
    if (!cols) return fail(IVJ_EINVAL, "cols is NULL");
    for (int32_t k = 0; k < n_cols; ++k) {
        const std::string who = "value column " + std::to_string(k);
        if (cols[k].ops == 0 || (cols[k].ops & ~AGG_ALL_OPS)) return fail(IVJ_EINVAL, who + ": ops must be a non-empty mask of IVJ_AGG_*");
        if (cols[k].dtype != IVJ_AGG_I64 && cols[k].dtype != IVJ_AGG_F64) return fail(IVJ_EINVAL, who + ": dtype must be IVJ_AGG_I64 or IVJ_AGG_F64");
        if (rows_present && !cols[k].values) return fail(IVJ_EINVAL, who + ": values is NULL");
    }
    return IVJ_OK;
}

// every output column of an operation that was asked for exists
int check_agg_outs(int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* o) {
    for (int32_t k = 0; k < n_cols; ++k) {
        const uint32_t ops = cols[k].ops;
        if (((ops & IVJ_AGG_SUM) && !o[k].sum) || ((ops & IVJ_AGG_MIN) && !o[k].min) || ((ops & IVJ_AGG_MAX) && !o[k].max) ||
            ((ops & IVJ_AGG_MEAN) && !o[k].mean) || ((ops & IVJ_AGG_COUNT) && !o[k].count))
            return fail(IVJ_EINVAL, "value column " + std::to_string(k) + ": an output column of a requested operation is NULL");
    }
    return IVJ_OK;
}

// one value column over the clusters of cl (device pointers throughout); part: merge_agg_bytes(ix->n) from the arena
template <class V>
void merge_agg_launch(ivj_ctx* ctx, const ivj_index* ix, const Clusters& cl, const ivj_agg_in& in, int64_t n_values, const ivj_agg_out& o, void* part) {
    using S = AggState<V>;
    const uint32_t ops = in.ops;
    AggOut<V> out;
    out.sum = (ops & IVJ_AGG_SUM) ? (typename S::Sum*)o.sum : nullptr;
    out.mn = (ops & IVJ_AGG_MIN) ? (V*)o.min : nullptr;
    out.mx = (ops & IVJ_AGG_MAX) ? (V*)o.max : nullptr;
    out.mean = (ops & IVJ_AGG_MEAN) ? o.mean : nullptr;
    out.count = (ops & IVJ_AGG_COUNT) ? (long long*)o.count : nullptr;
    const int64_t n = ix->n, tiles = magg_num_tiles(n);
    LAUNCH(ctx, "merge_agg_tiles", (k_magg_tiles<V>), tiles, MAGG_THREADS, (const uint32_t*)cl.cid1, (const int32_t*)ix->b_row, (const V*)in.values,
           in.valid, n, n_values, out, (S*)part);
    if (tiles > 1)
        LAUNCH(ctx, "merge_agg_span", (k_magg_span<V>), grid1d(tiles, MAGG_WAVES), MAGG_THREADS, (const uint32_t*)cl.cid1, (const int32_t*)cl.m_first, n, tiles,
               (const S*)part, out);
}

int merge_agg_col(ivj_ctx* ctx, const ivj_index* ix, const Clusters& cl, const ivj_agg_in& in, int64_t n_values, const ivj_agg_out& o, void* part) {
    if (ix->n == 0) return IVJ_OK;
    if (in.dtype == IVJ_AGG_I64) merge_agg_launch<long long>(ctx, ix, cl, in, n_values, o, part);
    else merge_agg_launch<double>(ctx, ix, cl, in, n_values, o, part);
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

}  // namespace
