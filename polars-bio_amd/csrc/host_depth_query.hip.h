// host_depth_query.hip.h -- host driver of pb.depth_summary (depth_query.hip.h): per probe row the maximum depth of the build side
// and the positions covered at least T deep, for up to IVJ_MAX_THRESHOLDS thresholds
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
//
// Every call builds what the probe kernel reads and releases it before it returns: the depth blocks of the index (depth_core, with
// its slow path for an index that holds a row with start > end), an index of the blocks (index_build, sweep + end order: the joint
// grid), and in the context's arena the block records, the interleaved threshold table and the tree of depth maxima.  NOTHING IS
// CACHED ON THE INDEX: the blocks depend on the mode (Strict / Weak) and the table on the threshold list, so what to keep, and
// keyed by what, is a decision for a later change, to be taken with the build / probe split of tools/bench_depth_summary.py in hand.
// The threshold table is K planar maps scanned in place (device_scan<long long, SumOp>, one launch each) and one interleaving
// kernel: the scan template is written for scalar types.
// partition_mode 1 is routed to the same probe-order kernel as 0 and 2: the three return identical arrays.
#pragma once

namespace {

static_assert(DQ_MAX_T == IVJ_MAX_THRESHOLDS, "DqThresholds holds IVJ_MAX_THRESHOLDS values");

int depth_query_zero(ivj_ctx* ctx, int64_t n, int32_t n_thr, int32_t* max_depth, int64_t* bases_ge) {
    if (max_depth) HIP_TRY(hipMemsetAsync(max_depth, 0, (size_t)n * 4, ctx->stream));
    if (n_thr > 0) HIP_TRY(hipMemsetAsync(bases_ge, 0, (size_t)n_thr * (size_t)n * 8, ctx->stream));
    return IVJ_OK;
}

// argument checks shared by both entries, whatever the number of probe rows
int depth_query_check(const int32_t* thresholds, int32_t n_thr, const void* max_depth, const void* bases_ge) {
    if (n_thr < 0 || n_thr > IVJ_MAX_THRESHOLDS) return fail(IVJ_EINVAL, "n_thresholds must be in 0 .. " + std::to_string(IVJ_MAX_THRESHOLDS));
    if (n_thr > 0 && !thresholds) return fail(IVJ_EINVAL, "thresholds is NULL");
    for (int k = 0; k < n_thr; ++k)
        if (thresholds[k] < 1) return fail(IVJ_EINVAL, "thresholds[" + std::to_string(k) + "] must be >= 1");
    if (!max_depth && !bases_ge) return fail(IVJ_EINVAL, "max_depth and bases_ge are both NULL");
    if (n_thr > 0 && !bases_ge) return fail(IVJ_EINVAL, "bases_ge is NULL");
    return IVJ_OK;
}

// the run-time KPAD (0, 1, 2, 4 or 8) as a template argument, once: f receives std::integral_constant<int, KPAD> (as with_bool)
template <class F>
auto with_kpad(int kpad, F&& f) {
    switch (kpad) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return f(std::integral_constant<int, 8>{});
    }
}

int depth_query_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe, const ivj_opts* opts, const int32_t* thresholds, int32_t n_thr,
                    int32_t* max_depth, int64_t* bases_ge) {
    const int64_t n = probe->n;
    if (n == 0) return IVJ_OK;
    if (ix->n == 0) return depth_query_zero(ctx, n, n_thr, max_depth, bases_ge);
    const bool strict = opts->filter_op == IVJ_FILTER_STRICT;
    // 1. the blocks, library-owned
    DevBuf own;
    int32_t *bc = nullptr, *bs = nullptr, *be = nullptr, *bd = nullptr;
    int64_t nb = 0;
    IVJ_TRY(depth_core(ctx, ix, opts, -1, &bc, &bs, &be, &bd, &own, &nb));
    if (nb == 0) return depth_query_zero(ctx, n, n_thr, max_depth, bases_ge);
    // 2. their index: already in (contig, start) order and disjoint, so sorted position = end-sorted position = block number
    const ivj_side blocks{bc, bs, be, nb, nullptr};
    ivj_opts o2 = *opts;
    o2.n_contigs = ix->n_contigs;
    o2.partition_mode = 0;
    IndexHolder h;
    IVJ_TRY(index_build(ctx, &blocks, &o2, 3, &h.ix));       // sweep only (no lookup tables) + the end order with the joint grid
    // 3. records, threshold table, tree: in the arena (the index build is done with it)
    const int kpad = n_thr == 0 ? 0 : (n_thr == 1 ? 1 : (n_thr == 2 ? 2 : (n_thr <= 4 ? 4 : 8)));
    const int64_t m = nb + 1;
    const size_t stride = align_up((size_t)m * 8) / 8;
    const HierShape hs = hier_shape(nb);
    IVJ_TRY(arena_reserve(ctx, align_up((size_t)nb * 16) + align_up(hs.values * 4) + (size_t)(n_thr ? n_thr : 1) * stride * 8 +
                               align_up((size_t)m * (kpad ? kpad : 1) * 8) + align_up((size_t)scan_num_tiles(m) * 8) + 4096));
    int4* rec = arena_take<int4>(ctx, nb);
    int32_t* tv = arena_take<int32_t>(ctx, hs.values);
    long long* planar = arena_take<long long>(ctx, (size_t)(n_thr ? n_thr : 1) * stride);
    unsigned long long* tab = arena_take<unsigned long long>(ctx, (size_t)m * (kpad ? kpad : 1));
    long long* partials = arena_take<long long>(ctx, scan_num_tiles(m));
    DqThresholds thr;
    for (int k = 0; k < DQ_MAX_T; ++k) thr.t[k] = k < n_thr ? thresholds[k] : INT32_MAX;
    const int64_t pad0 = (hs.len[0] + 15) & ~(int64_t)15;
    LAUNCH(ctx, "depth_query_records", k_dq_records, grid1d(pad0, 256), 256, (const int32_t*)bs, (const int32_t*)be, (const int32_t*)bd, nb, pad0, rec, tv);
    for (int l = 1; l <= hs.nlev; ++l) {
        const int64_t padded = (hs.len[l] + 15) & ~(int64_t)15;
        LAUNCH(ctx, "depth_query_tree", k_dq_tree_level, grid1d(padded, 256), 256, (const int32_t*)(tv + hs.off[l - 1]), hs.len[l - 1], tv + hs.off[l], padded);
    }
    if (n_thr > 0) {
        with_bool(strict, [&](auto S) {
            LAUNCH(ctx, "depth_query_lengths", (k_dq_lengths<S>), grid1d(m, 256), 256, (const int32_t*)bs, (const int32_t*)be, (const int32_t*)bd, nb, thr, (int)n_thr, stride, planar);
        });
        for (int k = 0; k < n_thr; ++k) {
            long long* col = planar + (size_t)k * stride;
            device_scan<long long, SumOp, false>(ctx, "depth_query_scan", (const long long*)col, col, m, 0ll, partials, (long long*)nullptr);
        }
        with_kpad(kpad, [&](auto KP) {
            if constexpr (decltype(KP)::value > 0)
                LAUNCH(ctx, "depth_query_table", (k_dq_interleave<decltype(KP)::value>), grid1d(m, 256), 256, (const long long*)planar, stride, (int)n_thr, m, tab);
        });
    }
    HIP_TRY(hipGetLastError());
    // 4. the probes, in probe order
    constexpr int NT = PROBE_THREADS * PROBE_ITEMS_LAT * DQ_TILES_PER_WG;
    const int64_t tiles = (n + NT - 1) / NT;
    const int32_t *qc = probe->contig, *qs = probe->start, *qe = probe->end;
    // vector access: the probe columns; every column of bases_ge (its base, and an even n or a single column); max_depth
    const int vec = ((aligned16(qc) && aligned16(qs) && aligned16(qe)) ? 1 : 0) |
                    ((n_thr > 0 && aligned16(bases_ge) && (n % 2 == 0 || n_thr == 1)) ? 2 : 0) |
                    ((max_depth && (reinterpret_cast<uintptr_t>(max_depth) & 7u) == 0) ? 4 : 0);
    const DqIndex v{h.ix->cmeta_j, h.ix->crec, h.ix->b_start, h.ix->e_end, h.ix->n_contigs};
    with_kpad(kpad, [&](auto KP) {
        with_bool(strict, h.ix->n_contigs <= CM_LDS, [&](auto S, auto LM) {
            LAUNCH(ctx, "depth_query", (k_depth_query<S, decltype(KP)::value, LM>), tiles, PROBE_THREADS, v, (const int32_t*)tv, (int)nb, (const int4*)rec,
                   (const unsigned long long*)tab, thr, (int)n_thr, qc, qs, qe, n, vec, max_depth, (long long*)bases_ge);
        });
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));              // the blocks and their index are released on return
    return IVJ_OK;
}

}  // namespace
