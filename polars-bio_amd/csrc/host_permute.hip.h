// host_permute.hip.h -- driver of pb.permutation_test (permute.hip.h): sort df1 once, mark the build rows without a position, then
// per chunk of permutations one k_permute launch and one fold.
// Part of the single translation unit ivjoin.hip (included there, after host_overlap_agg.hip.h); not a stand-alone header.
#pragma once

namespace {

constexpr int64_t PERM_MAX = 1ll << 20;                          // permutations per call
constexpr size_t PERM_PARTIAL_BYTES = (size_t)64 << 20;          // the partials of one launch stay below this (or hold one permutation block)

int permute_check(const ivj_opts* opts, const ivj_side* probe, const int32_t* contig_len, const int32_t* offsets, int64_t n_perm,
                  const int64_t* n_pairs, const int64_t* n_rows) {
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe, "probe"));
    if (n_perm < 1 || n_perm > PERM_MAX) return fail(IVJ_EINVAL, "n_perm must be in [1, 2^20]");
    if (!n_pairs || !n_rows) return fail(IVJ_EINVAL, "n_pairs or n_rows is NULL");
    if (opts->n_contigs > 0 && (!contig_len || !offsets)) return fail(IVJ_EINVAL, "contig_len or offsets is NULL");
    return IVJ_OK;
}

// what the set-up leaves for the launches of the same call; the sorted probe rows live in `sorted` (an index built without tables)
struct PermPlan {
    bool empty = true;                                           // nothing can match: the outputs are zeroed, no kernel runs
    IndexHolder sorted;
    const uint32_t *zs = nullptr, *ze = nullptr, *ztot = nullptr;
    longlong2* partial = nullptr;
    int64_t n = 0, tiles = 0;
    int per_launch = PERM_BLOCK;                                 // permutations per launch
    bool strict = false;
};

// Set-up: the joint grid of the build index, df1 in (contig, start) order, the prefix counts of build rows that cover no position.
// Every partition_mode routes to the one form: the sorted probe order is the locality the bucketed forms of other calls buy.
int permute_plan(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, int64_t n_perm, PermPlan& P) {
    ctx->ov_n = -1;                                              // invalidates a pending count -> fill hand-over (the arena is retaken)
    P.n = probe->n;
    P.strict = opts->filter_op == IVJ_FILTER_STRICT;
    if (!ix->has_tables) IVJ_TRY(need_tables(ctx, ix));          // (reports the merge / cluster only index)
    if (probe->n == 0 || ix->n == 0 || ix->n_contigs <= 0) return IVJ_OK;
    IVJ_TRY(build_end_order(ctx, ix));                           // e_end / e_pos and the joint grid
    ivj_opts sopts = *opts;
    sopts.n_contigs = ix->n_contigs; sopts.partition_mode = 0;
    IVJ_TRY(index_build(ctx, probe, &sopts, 2, &P.sorted.ix));   // sort only: no lookup tables
    P.empty = false;
    P.tiles = (P.n + PERM_TILE - 1) / PERM_TILE;
    // permutations per launch: whole blocks, at most PERM_CHUNK, and partials of at most PERM_PARTIAL_BYTES (one block at least)
    int64_t per = (int64_t)(PERM_PARTIAL_BYTES / ((size_t)P.tiles * 16)) / PERM_BLOCK * PERM_BLOCK;
    per = per < PERM_BLOCK ? PERM_BLOCK : (per > PERM_CHUNK ? PERM_CHUNK : per);
    if (per > n_perm) per = n_perm;
    P.per_launch = (int)per;
    const size_t zcol = align_up((size_t)(ix->n + 1) * 4);
    IVJ_TRY(arena_reserve(ctx, 2 * zcol + align_up((size_t)(scan_num_tiles(ix->n + 1) + 2) * 4) + align_up(16) +
                                   align_up((size_t)P.tiles * (size_t)per * 16) + 4096));
    uint32_t* zs = arena_take<uint32_t>(ctx, (size_t)ix->n + 1);
    uint32_t* ze = arena_take<uint32_t>(ctx, (size_t)ix->n + 1);
    uint32_t* scan_partials = arena_take<uint32_t>(ctx, (size_t)scan_num_tiles(ix->n + 1) + 2);
    uint32_t* ztot = arena_take<uint32_t>(ctx, 4);
    P.partial = arena_take<longlong2>(ctx, (size_t)P.tiles * (size_t)per);
    with_bool(P.strict, [&](auto S) {
        LAUNCH(ctx, "permute_zmark", (k_perm_zmark<S>), grid1d(ix->n + 1, 256), 256, (const int32_t*)ix->b_start, (const int2*)ix->ep,
               (const int32_t*)ix->e_end, (const int32_t*)ix->e_pos, ix->n, zs, ze);
    });
    device_scan<uint32_t, SumOp, false>(ctx, "permute_zscan", (const uint32_t*)ze, ze, ix->n + 1, 0u, scan_partials, (uint32_t*)nullptr);
    device_scan<uint32_t, SumOp, false>(ctx, "permute_zscan", (const uint32_t*)zs, zs, ix->n + 1, 0u, scan_partials, ztot);
    HIP_TRY(hipGetLastError());
    P.zs = zs; P.ze = ze; P.ztot = ztot;
    return IVJ_OK;
}

// n_perm permutations whose offsets start at offsets_dev (row-major n_perm x n_contigs): launch after launch of at most
// P.per_launch of them.  Device pointers; enqueued on the context's stream.
int permute_run(ivj_ctx* ctx, ivj_index* ix, const PermPlan& P, const int32_t* contig_len_dev, const int32_t* offsets_dev, int64_t n_perm,
                int64_t* n_pairs_dev, int64_t* n_rows_dev) {
    if (P.empty) {
        HIP_TRY(hipMemsetAsync(n_pairs_dev, 0, (size_t)n_perm * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(n_rows_dev, 0, (size_t)n_perm * 8, ctx->stream));
        return IVJ_OK;
    }
    const ivj_index* sx = P.sorted.ix;
    IndexView v = view_of(ix);
    for (int64_t p0 = 0; p0 < n_perm; p0 += P.per_launch) {
        const int np = (int)((n_perm - p0) < (int64_t)P.per_launch ? (n_perm - p0) : (int64_t)P.per_launch);
        const int32_t* off = offsets_dev + (size_t)p0 * (size_t)ix->n_contigs;
        const dim3 grid((unsigned)P.tiles, (unsigned)((np + PERM_BLOCK - 1) / PERM_BLOCK));
        with_bool(P.strict, [&](auto S) {
            t_begin(ctx, "permute_overlaps");
            hipLaunchKernelGGL((k_permute<S>), grid, dim3(PERM_THREADS), 0, ctx->stream, v, P.zs, P.ze, P.ztot, (const int32_t*)sx->b_contig,
                               (const int32_t*)sx->b_start, (const int2*)sx->ep, P.n, contig_len_dev, off, np, P.partial);
            t_end(ctx);
        });
        LAUNCH(ctx, "permute_fold", k_permute_fold, (np + kWave - 1) / kWave, PERM_FOLD_THREADS, (const longlong2*)P.partial, P.tiles, np,
               (long long*)n_pairs_dev + p0, (long long*)n_rows_dev + p0);
    }
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

int permute_overlaps_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, const int32_t* contig_len_dev,
                         const int32_t* offsets_dev, int64_t n_perm, int64_t* n_pairs_dev, int64_t* n_rows_dev) {
    PermPlan P;
    IVJ_TRY(permute_plan(ctx, ix, probe, opts, n_perm, P));
    return permute_run(ctx, ix, P, contig_len_dev, offsets_dev, n_perm, n_pairs_dev, n_rows_dev);
}

}  // namespace
