// host_depth_profile.hip.h -- host driver of pb.depth_profile (depth_profile.hip.h): the rows x bins matrix of per-bin base sums
// Part of the single translation unit ivjoin.hip (included there, in this order); not a stand-alone header.
//
// The windows are read in probe order only: opts->partition_mode is ignored (a bucketed form would have to bring n_bins values per
// row back into row order, and the lanes of a row already gather neighbouring grid records).
#pragma once

namespace {

int depth_profile_check(int32_t n_bins) {
    if (n_bins < 1 || n_bins > DPROF_MAX_BINS)
        return fail(IVJ_EINVAL, "n_bins must be in [1, " + std::to_string(DPROF_MAX_BINS) + "], got " + std::to_string(n_bins));
    return IVJ_OK;
}

int depth_profile_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* windows, const uint8_t* reverse, int32_t n_bins, const ivj_opts* opts,
                      int64_t* bases) {
    if (!ix->has_tables) IVJ_TRY(need_tables(ctx, ix));       // the kernel reads the joint grid only
    const int64_t n = windows->n;
    if (n == 0) return IVJ_OK;
    if (ix->n == 0) {
        HIP_TRY(hipMemsetAsync(bases, 0, (size_t)n * (size_t)n_bins * 8, ctx->stream));
        return IVJ_OK;
    }
    IVJ_TRY(build_end_order(ctx, ix));
    IVJ_TRY(build_position_sums(ctx, ix));
    const int64_t edges = n * ((int64_t)n_bins + 1);
    const int64_t wgs = (edges - 1 + DPROF_WG_EDGES - 1) / DPROF_WG_EDGES;     // the last edge of all forms no bin
    if (wgs > 0x7fffffffll) return fail(IVJ_EINVAL, "depth_profile: " + std::to_string(n) + " windows x " + std::to_string(n_bins) + " bins exceed one launch");
    IndexView v = view_of(ix);
    const unsigned long long *pa = ix->psum, *pe = ix->psum + ix->psum_stride;
    with_bool(opts->filter_op == IVJ_FILTER_STRICT, ix->n_contigs <= CM_LDS, [&](auto S, auto LM) {
        LAUNCH(ctx, "depth_profile", (k_depth_profile<S, LM>), wgs, PROBE_THREADS, v, pa, pe, (const int32_t*)windows->contig,
               (const int32_t*)windows->start, (const int32_t*)windows->end, reverse, n, (int)n_bins, (long long*)bases);
    });
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
}

// host buffers: the windows travel whole (12 bytes per row, + 1 with the flags), the matrix in chunks of rows so that it never
// takes more than DPROF_CHUNK_BYTES of device memory
constexpr size_t DPROF_CHUNK_BYTES = (size_t)256 << 20;

// what both profile host entries send first: the windows (J.dp) and the build side, the reverse flags (NULL stays NULL), then the index
int profile_upload(ivj_ctx* ctx, const ivj_side* windows, const uint8_t* reverse, const ivj_side* build, const ivj_opts* opts, JoinHost& J,
                   DevBuf& rev) {
    IVJ_TRY(upload_sides(ctx, windows, build, J));
    if (reverse) {
        IVJ_TRY(devbuf_alloc(rev, (size_t)windows->n, "reverse"));
        HostXfer copy(ctx->stream, &ctx->xfer);
        copy.h2d(rev.p, reverse, (size_t)windows->n);
        HIP_TRY(copy.finish());
    }
    return index_build(ctx, &J.db.s, opts, 0, &J.h.ix);
}

int depth_profile_host(ivj_ctx* ctx, const ivj_side* windows, const uint8_t* reverse, int32_t n_bins, const ivj_side* build,
                       const ivj_opts* opts, int64_t* bases) {
    JoinHost J;
    DevBuf rev;
    IVJ_TRY(profile_upload(ctx, windows, reverse, build, opts, J, rev));
    const int64_t n = windows->n;
    const size_t row_bytes = (size_t)n_bins * 8;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(DPROF_CHUNK_BYTES / row_bytes)));
    DevBuf out;
    IVJ_TRY(devbuf_alloc(out, (size_t)chunk * row_bytes, "profile"));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        ivj_side part = J.dp.s;
        part.contig += r0; part.start += r0; part.end += r0; part.n = m;
        IVJ_TRY(depth_profile_dev(ctx, J.h.ix, &part, reverse ? (const uint8_t*)rev.p + r0 : nullptr, n_bins, opts, (int64_t*)out.p));
        HostXfer copy(ctx->stream, &ctx->xfer);
        copy.d2h(bases + (size_t)r0 * n_bins, out.p, (size_t)m * row_bytes);
        HIP_TRY(copy.finish());                               // the next chunk's kernel writes the same device buffer
    }
    return IVJ_OK;
}

}  // namespace
