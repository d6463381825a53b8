// host_group.hip.h -- host driver of the group-id passes (group.hip.h): ivj_group_ids_dev, and the argument checks it shares with
// its host twin ivj_host_group_ids (host_frontdoor.hip.h).
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
#pragma once

namespace {

// D = n_contigs * prod(cards), refused beyond 2^31 (int32 keys and gids)
int group_domain(int32_t n_contigs, int32_t n_cols, const int32_t* cards, int64_t* domain) {
    if (n_contigs < 0) return fail(IVJ_EINVAL, "group ids: n_contigs < 0");
    if (n_cols < 0 || n_cols > GRP_MAX_COLS) return fail(IVJ_EINVAL, "group ids: n_cols must be in [0, " + std::to_string(GRP_MAX_COLS) + "]");
    if (n_cols > 0 && !cards) return fail(IVJ_EINVAL, "group ids: cards is NULL");
    std::string desc = std::to_string(n_contigs);
    int64_t d = n_contigs;
    bool over = false;
    for (int j = 0; j < n_cols; ++j) {
        if (cards[j] < 0) return fail(IVJ_EINVAL, "group ids: a cardinality is negative");
        desc += " x " + std::to_string(cards[j]);
        if (!over && d > 0 && cards[j] > GRP_MAX_DOMAIN / d) over = true;
        if (!over) d *= cards[j];
    }
    if (over || d > GRP_MAX_DOMAIN)
        return fail(IVJ_EINVAL, "group ids: key space " + desc + " exceeds 2^31 keys");
    *domain = d;
    return IVJ_OK;
}

int group_cols(GroupCols* c, const int32_t* contig, const int32_t* const* codes, int64_t n, int32_t n_cols, const int32_t* cards, int32_t n_contigs,
               const char* what) {
    std::memset(c, 0, sizeof(*c));
    if (n < 0) return fail(IVJ_EINVAL, std::string("group ids: ") + what + " n < 0");
    if (n > 0x7fff0000ll) return fail(IVJ_EINVAL, std::string("group ids: ") + what + " exceeds the int32 row-index range");
    if (n > 0 && !contig) return fail(IVJ_EINVAL, std::string("group ids: ") + what + " contig is NULL");
    if (n > 0 && n_cols > 0 && !codes) return fail(IVJ_EINVAL, std::string("group ids: ") + what + " codes is NULL");
    c->contig = contig;
    for (int j = 0; j < n_cols; ++j) {
        if (n > 0 && !codes[j]) return fail(IVJ_EINVAL, std::string("group ids: ") + what + " has a NULL code column");
        c->code[j] = n > 0 ? codes[j] : nullptr;
        c->card[j] = cards[j];
    }
    c->k = n_cols;
    c->n_contigs = n_contigs;
    c->n = n;
    return IVJ_OK;
}

}  // namespace

extern "C" {

int ivj_group_ids_dev(ivj_ctx* ctx, const int32_t* probe_contig, const int32_t* const* probe_codes, int64_t n_probe,
                      const int32_t* build_contig, const int32_t* const* build_codes, int64_t n_build, int32_t n_cols, const int32_t* cards,
                      int32_t n_contigs, int32_t* probe_gid, int32_t* build_gid, int32_t* group_keys, int64_t keys_cap, int32_t* n_groups) try {
    if (!ctx || !n_groups) return fail(IVJ_EINVAL, "group ids: ctx or n_groups is NULL");
    int64_t D = 0;
    IVJ_TRY(group_domain(n_contigs, n_cols, cards, &D));
    GroupCols pc, bc;
    IVJ_TRY(group_cols(&pc, probe_contig, probe_codes, n_probe, n_cols, cards, n_contigs, "probe"));
    IVJ_TRY(group_cols(&bc, build_contig, build_codes, n_build, n_cols, cards, n_contigs, "build"));
    if ((n_probe > 0 && !probe_gid) || (n_build > 0 && !build_gid)) return fail(IVJ_EINVAL, "group ids: a gid output is NULL");
    if (keys_cap < 0 || (keys_cap > 0 && !group_keys)) return fail(IVJ_EINVAL, "group ids: bad group_keys / keys_cap");
    *n_groups = 0;
    DeviceGuard g(ctx->device);
    const int64_t words = (D + 31) / 32;
    if (words == 0 || n_build == 0) {                    // no key present: every row is -1
        if (n_probe) HIP_TRY(hipMemsetAsync(probe_gid, 0xff, (size_t)n_probe * 4, ctx->stream));
        if (n_build) HIP_TRY(hipMemsetAsync(build_gid, 0xff, (size_t)n_build * 4, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return IVJ_OK;
    }
    const int64_t tiles = scan_num_tiles(words);
    IVJ_TRY(arena_reserve(ctx, 3 * align_up((size_t)words * 4) + align_up((size_t)(tiles + 1) * 4) + align_up(4) + 4096));
    uint32_t* bitmap = arena_take<uint32_t>(ctx, (size_t)words);
    uint32_t* cnt = arena_take<uint32_t>(ctx, (size_t)words);
    uint32_t* rank = arena_take<uint32_t>(ctx, (size_t)words);
    uint32_t* partials = arena_take<uint32_t>(ctx, (size_t)tiles + 1);
    uint32_t* total = arena_take<uint32_t>(ctx, 1);
    HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)words * 4, ctx->stream));
    // mark: enough workgroups to fill the device; each one privatizes the whole bitmap when it fits LDS
    const int64_t row_blocks = (n_build + GRP_THREADS * 8 - 1) / (GRP_THREADS * 8);
    const int cus = ctx->n_cus > 0 ? ctx->n_cus : 256;
    if (D <= GRP_LDS_BITS) {
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(row_blocks, (int64_t)cus * 4));
        t_begin(ctx, "group_mark_lds");
        hipLaunchKernelGGL(k_group_mark_lds, dim3(grid), dim3(GRP_THREADS), (size_t)words * 4, ctx->stream, bc, (uint32_t)words, bitmap);
        t_end(ctx);
    } else {
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(row_blocks, (int64_t)cus * 16));
        LAUNCH(ctx, "group_mark", k_group_mark_global, grid, GRP_THREADS, bc, bitmap);
    }
    HIP_TRY(hipGetLastError());
    LAUNCH(ctx, "group_popc", k_group_popc, grid1d(words, GRP_THREADS), GRP_THREADS, (const uint32_t*)bitmap, words, cnt);
    device_scan<uint32_t, SumOp, false>(ctx, "group_rank", cnt, rank, words, 0u, partials, total);
    HIP_TRY(hipGetLastError());
    auto remap = [&](const GroupCols& c, int32_t* gid) {
        bool vec = aligned16(c.contig) && aligned16(gid);
        for (int j = 0; j < c.k; ++j) vec = vec && aligned16(c.code[j]);
        LAUNCH(ctx, "group_remap", k_group_remap, grid1d((c.n + GRP_REMAP_ITEMS - 1) / GRP_REMAP_ITEMS, GRP_THREADS), GRP_THREADS, c,
               (const uint32_t*)bitmap, (const uint32_t*)rank, gid, vec ? 1 : 0);
    };
    if (n_probe) remap(pc, probe_gid);
    remap(bc, build_gid);
    if (group_keys && keys_cap > 0)
        LAUNCH(ctx, "group_table", k_group_table, grid1d(words, GRP_THREADS), GRP_THREADS, (const uint32_t*)bitmap, (const uint32_t*)rank, words, bc,
               group_keys, keys_cap);
    HIP_TRY(hipGetLastError());
    uint32_t G = 0;
    HIP_TRY(hipMemcpyAsync(&G, total, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_groups = (int32_t)G;
    if (group_keys && (int64_t)G > keys_cap)
        return fail(IVJ_ECAPACITY, "group ids: " + std::to_string(G) + " groups, group_keys holds " + std::to_string(keys_cap) + " rows");
    return IVJ_OK;
} IVJ_ABI_CATCH

}  // extern "C"
