// host_depth_sum.hip.h -- host driver of pb.mean_depth's per-row base sums (depth_sum.hip.h) and the position sums they read
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
#pragma once

namespace {

// psum = PA | PE: exclusive 64-bit prefix sums of flip(b_start) and flip(e_end), n + 1 entries each, in an allocation of the index's
// own (released with it), on the first call that needs them: index_build does not pay for them.  One map launch + one scan per array.
int build_position_sums(ivj_ctx* ctx, ivj_index* ix) {
    if (ix->has_psum) return IVJ_OK;
    IVJ_TRY(build_end_order(ctx, ix));
    const int64_t m = ix->n + 1;
    const size_t stride = align_up((size_t)m * 8) / 8;
    if (!ix->psum) {
        hipError_t e = hipMalloc((void**)&ix->psum, 2 * stride * 8);
        if (e != hipSuccess) { ix->psum = nullptr; return fail(IVJ_ENOMEM, std::string("hipMalloc(position sums): ") + hipGetErrorString(e)); }
    }
    IVJ_TRY(arena_reserve(ctx, align_up((size_t)scan_num_tiles(m) * 8) + 4096));
    long long* partials = arena_take<long long>(ctx, scan_num_tiles(m));
    const int32_t* keys[2] = {ix->b_start, ix->e_end};
    for (int k = 0; k < 2; ++k) {
        unsigned long long* out = ix->psum + (size_t)k * stride;
        LAUNCH(ctx, "position_map", k_position_map, grid1d(m, 256), 256, keys[k], ix->n, out);
        device_scan<long long, SumOp, false>(ctx, "position_sums", (const long long*)out, (long long*)out, m, 0ll, partials, (long long*)nullptr);
    }
    HIP_TRY(hipGetLastError());
    ix->psum_stride = stride;
    ix->has_psum = true;
    return IVJ_OK;
}

int depth_sum_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, int64_t* bases) {
    // the kernel reads the joint grid only; the start table is needed by the bucketed form
    if (!ix->has_tables || opts->partition_mode == 1) IVJ_TRY(need_tables(ctx, ix));
    const int64_t n = probe->n;
    if (n == 0) return IVJ_OK;
    if (ix->n == 0) {
        HIP_TRY(hipMemsetAsync(bases, 0, (size_t)n * 8, ctx->stream));
        return IVJ_OK;
    }
    IVJ_TRY(build_end_order(ctx, ix));
    IVJ_TRY(build_position_sums(ctx, ix));                   // before the arena is taken: it reserves for itself
    // partition_mode 1 only: the probes bucketed by genomic position, summed in bucket order into scratch, brought back to probe order
    // with the coalesced inverse permutation (as count_overlaps_dev).  Not the default, as there: the record gathers are the same, and
    // tools/bench_mean_depth.py times both forms ("Mean depth").
    const int32_t *qc = probe->contig, *qs = probe->start, *qe = probe->end;
    long long* o_bases = (long long*)bases;
    const bool bucketed = opts->partition_mode == 1;
    if (bucketed) {
        IVJ_TRY(bucket_probes(ctx, ix, probe, opts, &qc, &qs, &qe));
        IVJ_TRY(arena_reserve(ctx, align_up((size_t)n * 8) + 4096));
        o_bases = arena_take<long long>(ctx, n);
    }
    constexpr int NT = PROBE_THREADS * PROBE_ITEMS_LAT * DSUM_TILES_PER_WG;
    const int64_t tiles = (n + NT - 1) / NT;
    const bool vec = aligned16(qc) && aligned16(qs) && aligned16(qe);
    IndexView v = view_of(ix);
    const unsigned long long *pa = ix->psum, *pe = ix->psum + ix->psum_stride;
    with_bool(opts->filter_op == IVJ_FILTER_STRICT, ix->n_contigs <= CM_LDS, [&](auto S, auto LM) {
        LAUNCH(ctx, "depth_sum", (k_depth_sum<S, PROBE_ITEMS_LAT, LM>), tiles, PROBE_THREADS, v, pa, pe, qc, qs, qe, n, vec, o_bases);
    });
    HIP_TRY(hipGetLastError());
    if (bucketed) IVJ_TRY(unpermute_i64(ctx, n, o_bases, bases));
    return IVJ_OK;
}

}  // namespace
