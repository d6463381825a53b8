// ivjoin.hip -- host driver + C ABI (include/ivjoin.h) of the MI355X interval-join engine.
//
// Replaces, for the range-operation hot path, what the reference reaches through
//   range_operation_frame        /root/reference/src/lib.rs:79-145
//   do_range_operation & co      /root/reference/src/operation.rs:27-350
//   IntervalJoinExec + COITrees  (datafusion-bio-function-ranges v0.11.0, call sites
//                                 /root/reference/src/operation.rs:146-158,253-263,331-340)
// gfx950 only: no CUDA paths, no CPU fallback -- every entry point fails with IVJ_EHIP when
// no device is usable.
#include "../../include/ivjoin.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>
#include <thread>
#include <type_traits>

#include "probe.hip.h"
#include "slice.hip.h"
#include "cslice.hip.h"
#include "onesweep.hip.h"
#include "ixsort3.hip.h"
#include "scan.hip.h"
#include "group.hip.h"
#include "depth.hip.h"
#include "depth_sum.hip.h"
#include "depth_profile.hip.h"
#include "depth_query.hip.h"
#include "depth_hist.hip.h"
#include "depth_quant.hip.h"
#include "setop.hip.h"
#include "multi.hip.h"
#include "pairwise.hip.h"
#include "thresh.hip.h"
#include "window.hip.h"
#include "select.hip.h"
#include "merge_agg.hip.h"
#include "overlap_agg.hip.h"
#include "overlap_quant.hip.h"
#include "signal.hip.h"
#include "permute.hip.h"

using namespace ivj;

#include "host_core.hip.h"
#include "host_mem.hip.h"
#include "host_index.hip.h"
#include "host_slice.hip.h"
#include "host_cslice.hip.h"
#include "host_join.hip.h"
#include "host_sortscan.hip.h"
#include "host_merge_agg.hip.h"
#include "host_depth.hip.h"
#include "host_depth_sum.hip.h"
#include "host_depth_profile.hip.h"
#include "host_depth_query.hip.h"
#include "host_depth_hist.hip.h"
#include "host_depth_quant.hip.h"
#include "host_setop.hip.h"
#include "host_multi.hip.h"
#include "host_pairwise.hip.h"
#include "host_thresh.hip.h"
#include "host_window.hip.h"
#include "host_select.hip.h"
#include "host_overlap_agg.hip.h"
#include "host_overlap_quant.hip.h"
#include "host_signal.hip.h"
#include "host_permute.hip.h"
#include "host_stream.hip.h"
#include "host_comm.hip.h"
#include "host_group.hip.h"

// =============================================================================== C ABI

extern "C" {

const char* ivj_last_error(void) { return g_err.c_str(); }
const char* ivj_version(void) { return "ivjoin-hip 0.1 (gfx950)"; }
int ivj_abi_version(void) { return IVJ_ABI_VERSION; }
int64_t ivj_host_mem_available(void) { return (int64_t)host_mem_available(); }

int ivj_device_count(int* n) try {
    if (!n) return fail(IVJ_EINVAL, "n is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return fail(IVJ_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    *n = c;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_ctx_create(int device, ivj_ctx** out) try {
    if (!out) return fail(IVJ_EINVAL, "out is NULL");
    int cnt = 0;
    IVJ_TRY(ivj_device_count(&cnt));
    if (device < 0 || device >= cnt) return fail(IVJ_EHIP, "no usable HIP device " + std::to_string(device) + " (device count " + std::to_string(cnt) + ")");
    HIP_TRY(hipSetDevice(device));
    ivj_ctx* ctx = new ivj_ctx();
    ctx->device = device;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess) ctx->n_cus = cus; }
    hipError_t e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete ctx; return fail(IVJ_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
    ctx->stream = ctx->own_stream;
    if (const char* ev = std::getenv("IVJ_SLICE_ITEMS")) ctx->sl_items = std::atoi(ev) == 4 ? 4 : 2;
    if (const char* ev = std::getenv("IVJ_SLICE_ROWS")) ctx->sl_env_rows = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_SLICE_CHUNK")) ctx->sl_env_chunk = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_SLICE_NOTAB")) ctx->sl_env_notab = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_SLICE_NOBINS")) ctx->sl_env_nobins = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_SLICE_ABLATE")) ctx->sl_env_ablate = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_SLICE_AUTO")) ctx->sl_env_auto = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_SLICE_STABLE")) ctx->sl_env_stable = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_SLICE_SCATTER_THREADS")) ctx->sl_env_sthreads = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS")) ctx->cs_env_off = std::atoi(ev) == 0 ? 1 : 0;
    if (const char* ev = std::getenv("IVJ_CS_PTILE")) ctx->cs_env_ptile = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_NOCACHE")) ctx->cs_env_nocache = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_PERSIST")) ctx->cs_env_persist = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_PCHUNKS")) ctx->cs_env_pchunks = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_PMAX")) ctx->cs_env_pmax = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_PGRAIN")) ctx->cs_env_pgrain = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_WGTRACE")) ctx->cs_env_wgtrace = ev[0] ? ev : nullptr;
    if (const char* ev = std::getenv("IVJ_CS_SAMPLED")) ctx->cs_env_sampled = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_SLACK")) ctx->cs_env_slack = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_REC8")) ctx->cs_env_rec8 = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_FUSE_SAMPLE")) ctx->cs_env_fuse_sample = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_FILL_TWO")) ctx->cs_env_fill_two = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_CS_WALK")) ctx->cs_env_walk = std::atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = std::getenv("IVJ_JOINT_BINS")) ctx->env_joint_bins = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_COUNT_ABLATE")) ctx->env_count_ablate = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_NEAREST_LINES")) ctx->env_nearest_lines = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_COUNT_NOLDS")) ctx->env_count_nolds = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_IX_V3")) ctx->env_ix_v3 = std::atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = std::getenv("IVJ_SPIN_US")) ctx->env_spin_us = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_IX_MERGE")) ctx->env_ix_merge = std::atoi(ev);
    if (const char* ev = std::getenv("IVJ_IX_STAGE")) ctx->env_ix_stage = std::atoi(ev) != 0 ? 1 : 0;
    e = hipHostMalloc((void**)&ctx->h_total, 64, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipStreamDestroy(ctx->own_stream); delete ctx; return fail(IVJ_EHIP, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
    {
        // host words (host_core.hip.h): optional -- without them every value travels by copy as before
        const char* ev = std::getenv("IVJ_HOST_WORDS");
        if (!(ev && std::atoi(ev) == 0)) {
            void* hp = nullptr;
            void* dp = nullptr;
            if (hipHostMalloc(&hp, 256, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
                if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess && dp) {
                    std::memset(hp, 0, 256);
                    ctx->hw = (uint32_t*)hp; ctx->hw_dev = (uint32_t*)dp;
                } else (void)hipHostFree(hp);
            }
            (void)hipGetLastError();
        }
    }
    *out = ctx;
    return IVJ_OK;
} IVJ_ABI_CATCH

namespace {
void stream_release(ivj_stream* st, bool keep_cache);
void free_stream_bufs(ivj_ctx::StreamBufs& b) {
    if (b.h_in) (void)hipHostFree(b.h_in);
    if (b.d_in) (void)hipFree(b.d_in);
    if (b.d_out) (void)hipFree(b.d_out);
    if (b.h_out) (void)hipHostFree(b.h_out);
    b = ivj_ctx::StreamBufs();
}
}  // namespace

void ivj_ctx_destroy(ivj_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    while (!ctx->streams.empty()) stream_release(ctx->streams.back(), false);   // live streaming sessions: released and detached (their handles stay closable)
    for (ivj_index* ix : ctx->live) ix->ctx = nullptr;          // detached: they keep (and later free) their slabs
    for (ivj_comm* cm : ctx->comms) comm_detach(cm);            // detached: no call runs on them any more, ivj_comm_destroy still releases them
    if (ctx->arena.base) (void)hipFree(ctx->arena.base);
    if (ctx->ov_buf) (void)hipFree(ctx->ov_buf);
    if (ctx->sl_buf) (void)hipFree(ctx->sl_buf);
    if (ctx->cs_trace_buf) (void)hipFree(ctx->cs_trace_buf);
    if (ctx->lb_buf) (void)hipFree(ctx->lb_buf);
    if (ctx->sel_buf) (void)hipFree(ctx->sel_buf);
    for (auto& cb : ctx->st_cache) free_stream_bufs(cb);
    if (ctx->ix_cache) (void)hipFree(ctx->ix_cache);
    if (ctx->nl_cache) (void)hipFree(ctx->nl_cache);
    if (ctx->ix3_event) (void)hipEventDestroy(ctx->ix3_event);
    if (ctx->cs_event) (void)hipEventDestroy(ctx->cs_event);
    if (ctx->h_total) (void)hipHostFree(ctx->h_total);
    if (std::getenv("IVJ_DEBUG_REDO")) std::fprintf(stderr, "[ivj] context: host words %s, %lld misses of %u; ix3 fallbacks %lld\n", ctx->hw ? "on" : "off", (long long)ctx->hw_misses, ctx->hw_seq, (long long)ctx->ix3_fallbacks);
    if (ctx->hw) (void)hipHostFree(ctx->hw);
    ctx->xfer.release();
    for (hipEvent_t ev : ctx->pool) (void)hipEventDestroy(ev);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int ivj_ctx_set_stream(ivj_ctx* ctx, void* hip_stream) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->stream = (hip_stream == (void*)-1) ? ctx->own_stream : (hipStream_t)hip_stream;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_ctx_sync(ivj_ctx* ctx) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return IVJ_OK;
} IVJ_ABI_CATCH

namespace ivj { __global__ void k_profile_mark() {} }

int ivj_ctx_profile_mark(ivj_ctx* ctx) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    DeviceGuard g(ctx->device);
    hipLaunchKernelGGL(ivj::k_profile_mark, dim3(1), dim3(1), 0, ctx->stream);
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_ctx_enable_timing(ivj_ctx* ctx, int on) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->timing = on < 0 ? 0 : (on > 2 ? 2 : on);
    ctx->recs.clear();
    ctx->pool_used = 0;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_ctx_get_timings(ivj_ctx* ctx, ivj_timing* out, int cap, int* n) try {
    if (!ctx || !n) return fail(IVJ_EINVAL, "ctx or n is NULL");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<ivj_timing> agg;
    for (const TimingRec& r : ctx->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
        size_t j = 0;
        for (; j < agg.size(); ++j) if (std::strcmp(agg[j].name, r.name) == 0) break;
        if (j == agg.size()) {
            ivj_timing t; std::memset(&t, 0, sizeof t);
            std::strncpy(t.name, r.name, sizeof(t.name) - 1);
            agg.push_back(t);
        }
        agg[j].launches += 1; agg[j].ms += ms;
    }
    *n = (int)agg.size();
    for (int i = 0; i < (int)agg.size() && i < cap; ++i) out[i] = agg[i];
    ctx->recs.clear();
    ctx->pool_used = 0;
    return IVJ_OK;
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- device-resident API

int ivj_index_build_dev(ivj_ctx* ctx, const ivj_side* build_dev, const ivj_opts* opts, int with_end_order, ivj_index** out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(build_dev, "build"));
    DeviceGuard g(ctx->device);
    return index_build(ctx, build_dev, opts, with_end_order, out);
} IVJ_ABI_CATCH

void ivj_index_free(ivj_index* ix) {
    if (!ix) return;
    ivj_ctx* ctx = ix->ctx;
    if (ctx) {
        if (ctx->ov_ix == ix) { ctx->ov_ix = nullptr; ctx->ov_n = -1; }
        for (size_t k = 0; k < ctx->live.size(); ++k)
            if (ctx->live[k] == ix) { ctx->live[k] = ctx->live.back(); ctx->live.pop_back(); break; }
    }
    if (ix->nline) {
        if (ctx && ix->nline_cap > ctx->nl_cache_cap) {
            char* old = ctx->nl_cache;
            ctx->nl_cache = reinterpret_cast<char*>(ix->nline); ctx->nl_cache_cap = ix->nline_cap;
            if (old) { DeviceGuard g(ctx->device); (void)hipFree(old); }
        } else {
            DeviceGuard g(ix->device);
            (void)hipFree(ix->nline);
        }
    }
    if (ix->psum) {
        DeviceGuard g(ix->device);
        (void)hipFree(ix->psum);
    }
    if (ix->slab) {
        if (ctx && ix->slab_cap > ctx->ix_cache_cap) {
            // keep the larger slab for the next index on this context (same stream => ordered reuse)
            char* old = ctx->ix_cache;
            ctx->ix_cache = ix->slab; ctx->ix_cache_cap = ix->slab_cap;
            if (old) { DeviceGuard g(ctx->device); (void)hipFree(old); }
        } else {
            DeviceGuard g(ix->device);
            (void)hipFree(ix->slab);
        }
    }
    delete ix;
}

int ivj_overlap_count_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int64_t* n_pairs) try {
    if (!ctx || !ix || !n_pairs) return fail(IVJ_EINVAL, "ctx, index or n_pairs is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    DeviceGuard g(ctx->device);
    return overlap_count(ctx, ix, probe_dev, opts, n_pairs);
} IVJ_ABI_CATCH

int ivj_overlap_fill_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts,
                         int32_t* probe_idx_dev, int32_t* build_idx_dev, int64_t capacity) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    DeviceGuard g(ctx->device);
    return overlap_fill(ctx, ix, probe_dev, opts, probe_idx_dev, build_idx_dev, capacity);
} IVJ_ABI_CATCH

int ivj_overlap_fused_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts,
                          int32_t* probe_idx_dev, int32_t* build_idx_dev, int64_t capacity, int64_t* n_pairs) try {
    if (!ctx || !ix || !n_pairs) return fail(IVJ_EINVAL, "ctx, index or n_pairs is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    if (capacity < 0 || (capacity > 0 && (!probe_idx_dev || !build_idx_dev))) return fail(IVJ_EINVAL, "bad output buffers");
    DeviceGuard g(ctx->device);
    return overlap_fused(ctx, ix, probe_dev, opts, probe_idx_dev, build_idx_dev, capacity, n_pairs);
} IVJ_ABI_CATCH

// ---- multi-GPU: communicator, all-gatherv, sharded overlap with the exchange overlapping the join (host_comm.hip.h) ----

int ivj_comm_unique_id(void* id_out) try {
    if (!id_out) return fail(IVJ_EINVAL, "id_out is NULL");
    const RcclApi* api = rccl_api();
    if (!api) return fail(IVJ_EHIP, g_rccl.error);
    RcclUniqueId id;
    RCCL_TRY(api, api->GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_comm_create(ivj_ctx* ctx, const void* unique_id, int rank, int world, ivj_comm** out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    if (world < 1 || rank < 0 || rank >= world) return fail(IVJ_EINVAL, "rank / world out of range");
    if (world > 1 && !unique_id) return fail(IVJ_EINVAL, "unique_id is NULL");
    DeviceGuard g(ctx->device);
    ivj_comm* c = new ivj_comm();
    c->ctx = ctx; c->rank = rank; c->world = world;
    // IVJ_COMM_NO_SHORTCUT=1: also a single rank gets a real RCCL communicator and exchanges with itself through it (tests:
    // the dlopen'ed entry points, the exchange stream's ordering and the error mapping run on a 1-GPU box)
    const char* ns = std::getenv("IVJ_COMM_NO_SHORTCUT");
    c->self_rccl = ns && std::atoi(ns) != 0;
    if (world > 1 || c->self_rccl) {
        const RcclApi* api = rccl_api();
        if (!api) { delete c; return fail(IVJ_EHIP, g_rccl.error); }
        RcclUniqueId id;
        if (unique_id) std::memcpy(&id, unique_id, sizeof(id));
        else {
            const int ur = api->GetUniqueId(&id);
            if (ur != 0) { delete c; return fail(IVJ_EHIP, std::string("ncclGetUniqueId: ") + api->GetErrorString(ur)); }
        }
        const int r = api->CommInitRank(&c->comm, world, id, rank);
        if (r != 0) { delete c; return fail(IVJ_EHIP, std::string("ncclCommInitRank: ") + api->GetErrorString(r)); }
    }
    const int rc = comm_finish_create(c);
    if (rc != IVJ_OK) { ivj_comm_destroy(c); return rc; }
    *out = c;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_comm_create_local(ivj_ctx* const* ctxs, int n, ivj_comm** out) try {
    if (!ctxs || !out || n < 1) return fail(IVJ_EINVAL, "ctxs / out is NULL or n < 1");
    std::vector<RcclComm> comms((size_t)n, nullptr);
    LoopGroup* loop = nullptr;
    if (n > 1) {
        std::vector<int> devs((size_t)n);
        bool shared = false;
        for (int i = 0; i < n; ++i) {
            if (!ctxs[i]) return fail(IVJ_EINVAL, "a context is NULL");
            devs[i] = ctxs[i]->device;
            for (int j = 0; j < i; ++j) if (devs[j] == devs[i]) shared = true;
        }
        const char* ev = std::getenv("IVJ_COMM_LOOPBACK");
        if (shared || (ev && std::atoi(ev) != 0)) {
            // RCCL needs one device per rank; ranks that share a device (a 1-GPU box running the world-n protocol), or a host
            // that asks for it, get the in-process transport
            loop = new LoopGroup();
            loop->world = n; loop->refs = n;
            loop->vals.assign((size_t)n * 2, 0);
            loop->send.assign((size_t)n * LoopGroup::MAX_COLS, nullptr);
            loop->cnt.assign((size_t)n, 0);
        } else {
            const RcclApi* api = rccl_api();
            if (!api) return fail(IVJ_EHIP, g_rccl.error);
            RCCL_TRY(api, api->CommInitAll(comms.data(), n, devs.data()));
        }
    }
    for (int i = 0; i < n; ++i) {
        ivj_comm* c = new ivj_comm();
        c->ctx = ctxs[i]; c->rank = i; c->world = n; c->comm = comms[i]; c->loop = loop;
        const int rc = comm_finish_create(c);
        if (rc != IVJ_OK) {
            const std::string why = g_err;
            ivj_comm_destroy(c);
            for (int j = 0; j < i; ++j) { ivj_comm_destroy(out[j]); out[j] = nullptr; }
            if (loop && n - 1 - i > 0) {                 // the communicators never made: drop their references too
                bool last;
                { std::lock_guard<std::mutex> lk(loop->mu); loop->refs -= n - 1 - i; last = loop->refs == 0; }
                if (last) delete loop;
            }
            g_err = why;
            return rc;
        }
        out[i] = c;
    }
    return IVJ_OK;
} IVJ_ABI_CATCH

void ivj_comm_destroy(ivj_comm* c) {
    if (!c) return;
    DeviceGuard g(c->device);
    if (c->ctx) { auto& v = c->ctx->comms; v.erase(std::remove(v.begin(), v.end(), c), v.end()); }
    if (c->xstream) { (void)hipStreamSynchronize(c->xstream); }
    if (c->comm && rccl_api()) (void)rccl_api()->CommDestroy(c->comm);
    if (c->loop) {
        bool last;
        { std::lock_guard<std::mutex> lk(c->loop->mu); last = --c->loop->refs == 0; }
        if (last) delete c->loop;
    }
    for (auto& b : c->stage) if (b) (void)hipFree(b);
    if (c->iota) (void)hipFree(c->iota);
    if (c->pp_buf) (void)hipFree(c->pp_buf);
    if (c->d_counts) (void)hipFree(c->d_counts);
    if (c->h_counts) (void)hipHostFree(c->h_counts);
    if (c->xstream) (void)hipStreamDestroy(c->xstream);
    delete c;
}

int ivj_comm_info(const ivj_comm* c, int* rank, int* world) try {
    if (!c) return fail(IVJ_EINVAL, "comm is NULL");
    if (rank) *rank = c->rank;
    if (world) *world = c->world;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_allgather_counts(ivj_comm* c, int64_t n_local, int64_t* counts) try {
    if (!c || !counts || n_local < 0) return fail(IVJ_EINVAL, "comm / counts is NULL or n_local < 0");
    if (!c->ctx) return fail(IVJ_ESTATE, "the communicator's context was destroyed");
    DeviceGuard g(c->ctx->device);
    return comm_allgather_counts(c, n_local, counts);
} IVJ_ABI_CATCH

int ivj_allgatherv_dev(ivj_comm* c, const void* const* send_cols, void* const* recv_cols, int n_cols, int elem_bytes, const int64_t* counts) try {
    if (!c || !send_cols || !recv_cols || !counts || n_cols < 1 || elem_bytes < 1) return fail(IVJ_EINVAL, "bad all-gatherv arguments");
    if (!c->ctx) return fail(IVJ_ESTATE, "the communicator's context was destroyed");
    DeviceGuard g(c->ctx->device);
    HIP_TRY(hipStreamSynchronize(c->ctx->stream));                   // the payload is whatever the context's stream produced
    IVJ_TRY(comm_exchange(c, send_cols, recv_cols, n_cols, elem_bytes, counts, 0));
    HIP_TRY(hipStreamSynchronize(c->xstream));
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_overlap_allgather_dev(ivj_comm* c, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int n_chunks,
                              int32_t* probe_idx_dev, int32_t* build_idx_dev, int64_t capacity, int64_t* n_total, int64_t* n_local) try {
    if (!c || !ix || !n_total) return fail(IVJ_EINVAL, "comm, index or n_total is NULL");
    if (!c->ctx) return fail(IVJ_ESTATE, "the communicator's context was destroyed");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    if (n_chunks < 1 || n_chunks > 64) return fail(IVJ_EINVAL, "n_chunks must be in 1 .. 64");
    if (capacity < 0 || (capacity > 0 && (!probe_idx_dev || !build_idx_dev))) return fail(IVJ_EINVAL, "bad output buffers");
    DeviceGuard g(c->ctx->device);
    return overlap_allgather(c, ix, probe_dev, opts, n_chunks, probe_idx_dev, build_idx_dev, capacity, n_total, n_local);
} IVJ_ABI_CATCH

int ivj_count_overlaps_allgather_dev(ivj_comm* c, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int64_t n_total,
                                     int64_t* counts_dev) try {
    if (!c || !ix) return fail(IVJ_EINVAL, "comm or index is NULL");
    if (!c->ctx) return fail(IVJ_ESTATE, "the communicator's context was destroyed");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    if (n_total < 0 || (n_total > 0 && !counts_dev)) return fail(IVJ_EINVAL, "n_total < 0 or counts is NULL");
    DeviceGuard g(c->ctx->device);
    return per_probe_allgather(c, ix, probe_dev, opts, IVJ_STREAM_COUNT, n_total, counts_dev, nullptr, nullptr, nullptr);
} IVJ_ABI_CATCH

int ivj_nearest_allgather_dev(ivj_comm* c, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int64_t n_total,
                              int32_t* idx_dev, int64_t* dist_dev, int32_t* n_found_dev) try {
    if (!c || !ix) return fail(IVJ_EINVAL, "comm or index is NULL");
    if (!c->ctx) return fail(IVJ_ESTATE, "the communicator's context was destroyed");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    if (opts->nearest_k > 1024) return fail(IVJ_EINVAL, "nearest_k > 1024");
    if (n_total < 0 || (n_total > 0 && (!idx_dev || !dist_dev || !n_found_dev))) return fail(IVJ_EINVAL, "n_total < 0 or nearest output buffers are NULL");
    DeviceGuard g(c->ctx->device);
    return per_probe_allgather(c, ix, probe_dev, opts, IVJ_STREAM_NEAREST, n_total, nullptr, idx_dev, dist_dev, n_found_dev);
} IVJ_ABI_CATCH

int ivj_overlap_fused_rows_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_rows* rows_dev,
                               int64_t* n_pairs) try {
    if (!ctx || !ix || !rows_dev || !n_pairs) return fail(IVJ_EINVAL, "ctx, index, rows or n_pairs is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    if (rows_dev->n_pairs < 0) return fail(IVJ_EINVAL, "capacity (rows->n_pairs) < 0");
    if (opts->partition_mode == 5) return fail(IVJ_EINVAL, "partition_mode 5 is not available for the rows path");
    DeviceGuard g(ctx->device);
    return overlap_fused_rows(ctx, ix, probe_dev, opts, rows_dev, n_pairs);
} IVJ_ABI_CATCH

int ivj_count_overlaps_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int64_t* counts_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    if (probe_dev->n > 0 && !counts_dev) return fail(IVJ_EINVAL, "counts is NULL");
    DeviceGuard g(ctx->device);
    return count_overlaps_dev(ctx, ix, probe_dev, opts, counts_dev);
} IVJ_ABI_CATCH

int ivj_nearest_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int32_t* idx_dev,
                    int64_t* dist_dev, int32_t* n_found_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    if (probe_dev->n > 0 && (!idx_dev || !dist_dev || !n_found_dev)) return fail(IVJ_EINVAL, "nearest output buffers are NULL");
    if (opts->nearest_k > 1024) return fail(IVJ_EINVAL, "nearest_k > 1024");
    DeviceGuard g(ctx->device);
    return nearest_dev(ctx, ix, probe_dev, opts, idx_dev, dist_dev, n_found_dev);
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- host-buffer API

int ivj_overlap(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, ivj_pairs* out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    out->n_pairs = 0; out->probe_idx = nullptr; out->build_idx = nullptr;
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    DeviceGuard g(ctx->device);
    JoinHost J;
    IVJ_TRY(upload_join(ctx, probe, build, opts, 0, J));
    int64_t total = 0;
    IVJ_TRY(overlap_count(ctx, J.h.ix, &J.dp.s, opts, &total));
    if (total == 0) return IVJ_OK;
    DevPairs P;
    IVJ_TRY(alloc_pairs(total, 8, "; use the streaming entry points (ivj_stream_*) or the *_dev ones", P));
    IVJ_TRY(overlap_fill(ctx, J.h.ix, &J.dp.s, opts, (int32_t*)P.p.p, (int32_t*)P.b.p, total));
    return pairs_to_host(ctx, total, P, out);
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- merge / cluster / coverage

int ivj_cluster_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int64_t min_dist, int64_t* cluster_dev, int32_t* cluster_start_dev,
                    int32_t* cluster_end_dev, int64_t* n_clusters) try {
    if (!ctx || !ix || !n_clusters) return fail(IVJ_EINVAL, "ctx, index or n_clusters is NULL");
    IVJ_TRY(check_opts(opts));
    if (min_dist < 0) return fail(IVJ_EINVAL, "min_dist < 0");
    if (ix->n > 0 && (!cluster_dev || !cluster_start_dev || !cluster_end_dev)) return fail(IVJ_EINVAL, "cluster output buffers are NULL");
    DeviceGuard g(ctx->device);
    Clusters cl;
    IVJ_TRY(cluster_core(ctx, ix, opts->filter_op == IVJ_FILTER_STRICT, (long long)min_dist, 0, cl));
    *n_clusters = cl.n;
    if (ix->n == 0) return IVJ_OK;
    LAUNCH(ctx, "cluster_scatter", k_cluster_scatter, grid1d(ix->n, 256), 256, (const int32_t*)ix->b_row, (const uint32_t*)cl.cid1, (const int32_t*)cl.m_start,
           (const int32_t*)cl.m_end, ix->n, (long long*)cluster_dev, cluster_start_dev, cluster_end_dev);
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_merge_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int64_t min_dist, int64_t capacity, int32_t* contig_dev, int32_t* start_dev,
                  int32_t* end_dev, int64_t* n_intervals_dev, int64_t* n_merged) try {
    if (!ctx || !ix || !n_merged) return fail(IVJ_EINVAL, "ctx, index or n_merged is NULL");
    IVJ_TRY(check_opts(opts));
    if (min_dist < 0 || capacity < 0) return fail(IVJ_EINVAL, "min_dist or capacity < 0");
    DeviceGuard g(ctx->device);
    Clusters cl;
    IVJ_TRY(cluster_core(ctx, ix, opts->filter_op == IVJ_FILTER_STRICT, (long long)min_dist, 0, cl));
    *n_merged = cl.n;
    if (cl.n == 0) return IVJ_OK;
    if (cl.n > capacity) return fail(IVJ_ECAPACITY, "merge output capacity " + std::to_string(capacity) + " < " + std::to_string(cl.n) + " intervals");
    if (!contig_dev || !start_dev || !end_dev || !n_intervals_dev) return fail(IVJ_EINVAL, "merge output buffers are NULL");
    HIP_TRY(hipMemcpyAsync(contig_dev, cl.m_contig, (size_t)cl.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(start_dev, cl.m_start, (size_t)cl.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(end_dev, cl.m_end, (size_t)cl.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    LAUNCH(ctx, "cluster_counts", k_cluster_counts, grid1d(cl.n, 256), 256, (const int32_t*)cl.m_first, cl.n, (long long*)n_intervals_dev);
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_coverage_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int64_t* coverage_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    if (probe_dev->n > 0 && !coverage_dev) return fail(IVJ_EINVAL, "coverage is NULL");
    DeviceGuard g(ctx->device);
    return coverage_core(ctx, ix, probe_dev, opts, coverage_dev);
} IVJ_ABI_CATCH

int ivj_overlap_bases_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int64_t* bases_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    if (probe_dev->n > 0 && !bases_dev) return fail(IVJ_EINVAL, "bases is NULL");
    DeviceGuard g(ctx->device);
    return depth_sum_dev(ctx, ix, probe_dev, opts, bases_dev);
} IVJ_ABI_CATCH

void ivj_merged_free(ivj_merged* m) {
    if (!m) return;
    std::free(m->contig); std::free(m->start); std::free(m->end); std::free(m->n_intervals);
    m->contig = m->start = m->end = nullptr; m->n_intervals = nullptr; m->n = 0;
}

int ivj_merge(ivj_ctx* ctx, const ivj_side* side, const ivj_opts* opts, int64_t min_dist, ivj_merged* out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    std::memset(out, 0, sizeof(*out));
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(side, "frame"));
    if (min_dist < 0) return fail(IVJ_EINVAL, "min_dist < 0");
    if (side->n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    FrameHost F;
    IVJ_TRY(upload_frame(ctx, side, opts, 2, F));          // sweep only: no lookup tables
    Clusters cl;
    IVJ_TRY(cluster_core(ctx, F.h.ix, opts->filter_op == IVJ_FILTER_STRICT, (long long)min_dist, align_up((size_t)(side->n + 1) * 8), cl));
    long long* cnt = arena_take<long long>(ctx, side->n + 1);
    LAUNCH(ctx, "cluster_counts", k_cluster_counts, grid1d(cl.n, 256), 256, (const int32_t*)cl.m_first, cl.n, cnt);
    IVJ_TRY(copy_out_columns(ctx, cl.n, {{(void**)&out->contig, cl.m_contig, 4}, {(void**)&out->start, cl.m_start, 4}, {(void**)&out->end, cl.m_end, 4},
                                         {(void**)&out->n_intervals, cnt, 8}}, "merged", [&] { ivj_merged_free(out); }));
    out->n = cl.n;
    return IVJ_OK;
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- merge with aggregates (merge_agg.hip.h)

int ivj_merge_agg_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int64_t min_dist, int64_t capacity, int32_t* contig_dev, int32_t* start_dev,
                      int32_t* end_dev, int64_t* n_intervals_dev, int64_t n_values, int32_t n_cols, const ivj_agg_in* cols,
                      const ivj_agg_out* agg_out, int64_t* n_merged) try {
    if (!ctx || !ix || !n_merged) return fail(IVJ_EINVAL, "ctx, index or n_merged is NULL");
    IVJ_TRY(check_opts(opts));
    if (min_dist < 0 || capacity < 0 || n_values < 0) return fail(IVJ_EINVAL, "min_dist, capacity or n_values < 0");
    IVJ_TRY(check_agg_cols(n_cols, cols, ix->n > 0 && n_values > 0));
    DeviceGuard g(ctx->device);
    Clusters cl;
    IVJ_TRY(cluster_core(ctx, ix, opts->filter_op == IVJ_FILTER_STRICT, (long long)min_dist, merge_agg_bytes(ix->n), cl));
    *n_merged = cl.n;
    if (cl.n == 0) return IVJ_OK;
    if (cl.n > capacity) return fail(IVJ_ECAPACITY, "merge output capacity " + std::to_string(capacity) + " < " + std::to_string(cl.n) + " intervals");
    if (!contig_dev || !start_dev || !end_dev || !n_intervals_dev || !agg_out) return fail(IVJ_EINVAL, "merge output buffers are NULL");
    IVJ_TRY(check_agg_outs(n_cols, cols, agg_out));
    void* part = arena_take<AggState<double>>(ctx, 2 * magg_num_tiles(ix->n) + 1);
    HIP_TRY(hipMemcpyAsync(contig_dev, cl.m_contig, (size_t)cl.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(start_dev, cl.m_start, (size_t)cl.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(end_dev, cl.m_end, (size_t)cl.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    LAUNCH(ctx, "cluster_counts", k_cluster_counts, grid1d(cl.n, 256), 256, (const int32_t*)cl.m_first, cl.n, (long long*)n_intervals_dev);
    for (int32_t k = 0; k < n_cols; ++k) IVJ_TRY(merge_agg_col(ctx, ix, cl, cols[k], n_values, agg_out[k], part));
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
} IVJ_ABI_CATCH

void ivj_merge_agg_free(ivj_merged* m, ivj_agg_out* agg_out, int32_t n_cols) {
    ivj_merged_free(m);
    if (!agg_out) return;
    for (int32_t k = 0; k < n_cols; ++k) {
        std::free(agg_out[k].sum); std::free(agg_out[k].min); std::free(agg_out[k].max); std::free(agg_out[k].mean); std::free(agg_out[k].count);
        std::memset(&agg_out[k], 0, sizeof(agg_out[k]));
    }
}

int ivj_merge_agg(ivj_ctx* ctx, const ivj_side* side, const ivj_opts* opts, int64_t min_dist, int32_t n_cols, const ivj_agg_in* cols,
                  ivj_merged* out, ivj_agg_out* agg_out) try {
    if (!ctx || !out || !agg_out) return fail(IVJ_EINVAL, "ctx, out or agg_out is NULL");
    std::memset(out, 0, sizeof(*out));
    if (n_cols >= 1 && n_cols <= IVJ_MAX_AGG_COLS) std::memset(agg_out, 0, sizeof(*agg_out) * (size_t)n_cols);
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(side, "frame"));
    if (min_dist < 0) return fail(IVJ_EINVAL, "min_dist < 0");
    IVJ_TRY(check_agg_cols(n_cols, cols, side->n > 0));
    if (side->row_id) return fail(IVJ_EINVAL, "ivj_merge_agg reads the values by frame position: row_id must be NULL");
    if (side->n == 0) return IVJ_OK;
    const int64_t n = side->n;
    DeviceGuard g(ctx->device);
    FrameHost F;
    IVJ_TRY(upload_frame(ctx, side, opts, 2, F));          // sweep only: no lookup tables
    // arena: the count column, the tile parts, one value column with its validity bytes, the five result columns of one value column
    const size_t col8 = align_up((size_t)(n + 1) * 8);
    Clusters cl;
    IVJ_TRY(cluster_core(ctx, F.h.ix, opts->filter_op == IVJ_FILTER_STRICT, (long long)min_dist,
                         col8 + merge_agg_bytes(n) + col8 + align_up((size_t)n + 1) + 5 * col8, cl));
    long long* cnt = arena_take<long long>(ctx, n + 1);
    void* part = arena_take<AggState<double>>(ctx, 2 * magg_num_tiles(n) + 1);
    long long* d_val = arena_take<long long>(ctx, n + 1);
    uint8_t* d_valid = arena_take<uint8_t>(ctx, n + 1);
    void* d_res[5];
    for (int r = 0; r < 5; ++r) d_res[r] = arena_take<long long>(ctx, n + 1);
    LAUNCH(ctx, "cluster_counts", k_cluster_counts, grid1d(cl.n, 256), 256, (const int32_t*)cl.m_first, cl.n, cnt);
    const size_t m4 = (size_t)cl.n * 4, m8 = (size_t)cl.n * 8;
    out->contig = (int32_t*)host_result_alloc(m4);
    out->start = (int32_t*)host_result_alloc(m4);
    out->end = (int32_t*)host_result_alloc(m4);
    out->n_intervals = (int64_t*)host_result_alloc(m8);
    bool alloc_ok = out->contig && out->start && out->end && out->n_intervals;
    for (int32_t k = 0; k < n_cols && alloc_ok; ++k) {
        const uint32_t ops = cols[k].ops;
        ivj_agg_out& o = agg_out[k];
        if (ops & IVJ_AGG_SUM) alloc_ok = alloc_ok && (o.sum = host_result_alloc(m8));
        if (ops & IVJ_AGG_MIN) alloc_ok = alloc_ok && (o.min = host_result_alloc(m8));
        if (ops & IVJ_AGG_MAX) alloc_ok = alloc_ok && (o.max = host_result_alloc(m8));
        if (ops & IVJ_AGG_MEAN) alloc_ok = alloc_ok && (o.mean = (double*)host_result_alloc(m8));
        if (ops & IVJ_AGG_COUNT) alloc_ok = alloc_ok && (o.count = (int64_t*)host_result_alloc(m8));
    }
    if (!alloc_ok) { ivj_merge_agg_free(out, agg_out, n_cols); return fail(IVJ_ENOMEM, "host malloc(merged aggregates)"); }
    int rc = IVJ_OK;
    hipError_t e = hipSuccess;
    {
        HostXfer copy(ctx->stream, &ctx->xfer);
        copy.d2h(out->contig, cl.m_contig, m4);
        copy.d2h(out->start, cl.m_start, m4);
        copy.d2h(out->end, cl.m_end, m4);
        copy.d2h(out->n_intervals, cnt, m8);
        const ivj_agg_out dev{d_res[0], d_res[1], d_res[2], (double*)d_res[3], (int64_t*)d_res[4]};
        for (int32_t k = 0; k < n_cols && rc == IVJ_OK; ++k) {
            // the copies and the launches are ordered by the stream: column k + 1 overwrites the buffers after column k's copies left
            copy.h2d(d_val, cols[k].values, (size_t)n * 8);
            if (cols[k].valid) copy.h2d(d_valid, cols[k].valid, (size_t)n);
            const ivj_agg_in in{d_val, cols[k].valid ? d_valid : nullptr, cols[k].dtype, cols[k].ops};
            rc = merge_agg_col(ctx, F.h.ix, cl, in, n, dev, part);
            const ivj_agg_out& o = agg_out[k];
            if (o.sum) copy.d2h(o.sum, dev.sum, m8);
            if (o.min) copy.d2h(o.min, dev.min, m8);
            if (o.max) copy.d2h(o.max, dev.max, m8);
            if (o.mean) copy.d2h(o.mean, dev.mean, m8);
            if (o.count) copy.d2h(o.count, dev.count, m8);
        }
        e = copy.finish();
    }
    if (rc != IVJ_OK) { ivj_merge_agg_free(out, agg_out, n_cols); return rc; }
    if (e != hipSuccess) { ivj_merge_agg_free(out, agg_out, n_cols); return fail(IVJ_EHIP, std::string("copies(merged aggregates): ") + hipGetErrorString(e)); }
    out->n = cl.n;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_cluster(ivj_ctx* ctx, const ivj_side* side, const ivj_opts* opts, int64_t min_dist, int64_t* cluster, int32_t* cluster_start,
                int32_t* cluster_end, int64_t* n_clusters) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(side, "frame"));
    if (side->row_id) return fail(IVJ_EINVAL, "ivj_cluster reports per input row: row_id must be NULL");
    if (n_clusters) *n_clusters = 0;
    if (side->n == 0) return IVJ_OK;
    if (!cluster || !cluster_start || !cluster_end) return fail(IVJ_EINVAL, "cluster output buffers are NULL");
    DeviceGuard g(ctx->device);
    FrameHost F;
    IVJ_TRY(upload_frame(ctx, side, opts, 2, F));          // sweep only: no lookup tables
    DevBuf out;
    const size_t n = (size_t)side->n;
    IVJ_TRY(devbuf_alloc(out, align_up(n * 8) + 2 * align_up(n * 4), "cluster"));
    int64_t* d_c = (int64_t*)out.p;
    int32_t* d_s = (int32_t*)((char*)out.p + align_up(n * 8));
    int32_t* d_e = (int32_t*)((char*)d_s + align_up(n * 4));
    int64_t ncl = 0;
    IVJ_TRY(ivj_cluster_dev(ctx, F.h.ix, opts, min_dist, d_c, d_s, d_e, &ncl));
    IVJ_TRY(d2h_finish(ctx, {{cluster, d_c, n * 8}, {cluster_start, d_s, n * 4}, {cluster_end, d_e, n * 4}}));
    if (n_clusters) *n_clusters = ncl;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_coverage(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, int64_t* coverage) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    if (probe->n == 0) return IVJ_OK;
    if (!coverage) return fail(IVJ_EINVAL, "coverage is NULL");
    DeviceGuard g(ctx->device);
    JoinHost J;
    IVJ_TRY(upload_join(ctx, probe, build, opts, 0, J));
    DevBuf out;
    IVJ_TRY(devbuf_alloc(out, (size_t)probe->n * 8, "coverage"));
    IVJ_TRY(coverage_core(ctx, J.h.ix, &J.dp.s, opts, (int64_t*)out.p));
    return d2h_finish(ctx, {{coverage, out.p, (size_t)probe->n * 8}});
} IVJ_ABI_CATCH

int ivj_overlap_bases(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, int64_t* bases) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    if (probe->n == 0) return IVJ_OK;
    if (!bases) return fail(IVJ_EINVAL, "bases is NULL");
    DeviceGuard g(ctx->device);
    JoinHost J;
    IVJ_TRY(upload_join(ctx, probe, build, opts, 0, J));
    DevBuf out;
    IVJ_TRY(devbuf_alloc(out, (size_t)probe->n * 8, "bases"));
    IVJ_TRY(depth_sum_dev(ctx, J.h.ix, &J.dp.s, opts, (int64_t*)out.p));
    return d2h_finish(ctx, {{bases, out.p, (size_t)probe->n * 8}});
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- depth profile (per-bin base sums of every window row)

int ivj_depth_profile_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* windows_dev, const uint8_t* reverse_dev, int32_t n_bins,
                          const ivj_opts* opts, int64_t* bases_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(windows_dev, "windows"));
    IVJ_TRY(depth_profile_check(n_bins));
    if (windows_dev->n > 0 && !bases_dev) return fail(IVJ_EINVAL, "bases is NULL");
    DeviceGuard g(ctx->device);
    return depth_profile_dev(ctx, ix, windows_dev, reverse_dev, n_bins, opts, bases_dev);
} IVJ_ABI_CATCH

int ivj_depth_profile(ivj_ctx* ctx, const ivj_side* windows, const uint8_t* reverse, int32_t n_bins, const ivj_side* build,
                      const ivj_opts* opts, int64_t* bases) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_args(opts, windows, "windows", build, "build"));
    IVJ_TRY(depth_profile_check(n_bins));
    if (windows->n == 0) return IVJ_OK;
    if (!bases) return fail(IVJ_EINVAL, "bases is NULL");
    DeviceGuard g(ctx->device);
    return depth_profile_host(ctx, windows, reverse, n_bins, build, opts, bases);
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- depth (run-length coverage blocks)

int ivj_depth_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int64_t capacity, int32_t* contig_dev, int32_t* start_dev,
                  int32_t* end_dev, int32_t* depth_dev, int64_t* n_blocks) try {
    if (!ctx || !ix || !n_blocks) return fail(IVJ_EINVAL, "ctx, index or n_blocks is NULL");
    IVJ_TRY(check_opts(opts));
    if (capacity < 0) return fail(IVJ_EINVAL, "capacity < 0");
    DeviceGuard g(ctx->device);
    return depth_core(ctx, ix, opts, capacity, &contig_dev, &start_dev, &end_dev, &depth_dev, nullptr, n_blocks);
} IVJ_ABI_CATCH

void ivj_blocks_free(ivj_blocks* b) {
    if (!b) return;
    std::free(b->contig); std::free(b->start); std::free(b->end); std::free(b->depth);
    b->contig = b->start = b->end = b->depth = nullptr; b->n = 0;
}

int ivj_depth(ivj_ctx* ctx, const ivj_side* frame, const ivj_opts* opts, ivj_blocks* out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    std::memset(out, 0, sizeof(*out));
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(frame, "frame"));
    if (frame->n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    FrameHost F;
    IVJ_TRY(upload_frame(ctx, frame, opts, 3, F));         // sweep only (no lookup tables) + the end order
    DevBuf own;
    int32_t *d_contig = nullptr, *d_start = nullptr, *d_end = nullptr, *d_depth = nullptr;
    int64_t total = 0;
    IVJ_TRY(depth_core(ctx, F.h.ix, opts, -1, &d_contig, &d_start, &d_end, &d_depth, &own, &total));
    if (total == 0) return IVJ_OK;
    IVJ_TRY(copy_out_columns(ctx, total, {{(void**)&out->contig, d_contig, 4}, {(void**)&out->start, d_start, 4}, {(void**)&out->end, d_end, 4},
                                          {(void**)&out->depth, d_depth, 4}}, "blocks", [&] { ivj_blocks_free(out); }));
    out->n = total;
    return IVJ_OK;
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- depth summary (max depth, bases at depth thresholds)

int ivj_depth_summary_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const int32_t* thresholds,
                          int32_t n_thresholds, int32_t* max_depth_dev, int64_t* bases_ge_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    IVJ_TRY(depth_query_check(thresholds, n_thresholds, max_depth_dev, bases_ge_dev));
    DeviceGuard g(ctx->device);
    return depth_query_dev(ctx, ix, probe_dev, opts, thresholds, n_thresholds, max_depth_dev, bases_ge_dev);
} IVJ_ABI_CATCH

int ivj_depth_summary(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const int32_t* thresholds,
                      int32_t n_thresholds, int32_t* max_depth, int64_t* bases_ge) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    IVJ_TRY(depth_query_check(thresholds, n_thresholds, max_depth, bases_ge));
    if (probe->n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    JoinHost J;
    IVJ_TRY(upload_join(ctx, probe, build, opts, 3, J));   // sweep only (no lookup tables) + the end order: what depth_core reads
    const size_t n = (size_t)probe->n, md_bytes = align_up(n * 4), col_bytes = n * 8;
    DevBuf out;
    IVJ_TRY(devbuf_alloc(out, md_bytes + (size_t)n_thresholds * col_bytes + 256, "depth summary"));
    int32_t* d_md = max_depth ? (int32_t*)out.p : nullptr;
    int64_t* d_bg = n_thresholds > 0 ? (int64_t*)((char*)out.p + md_bytes) : nullptr;
    IVJ_TRY(depth_query_dev(ctx, J.h.ix, &J.dp.s, opts, thresholds, n_thresholds, d_md, d_bg));
    return d2h_finish(ctx, {{max_depth, d_md, d_md ? n * 4 : 0}, {bases_ge, d_bg, d_bg ? (size_t)n_thresholds * col_bytes : 0}});
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- depth histogram (positions at each depth, per row / per contig)

int ivj_depth_hist_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int32_t max_depth, int64_t* hist_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    IVJ_TRY(depth_hist_check(max_depth, hist_dev));
    DeviceGuard g(ctx->device);
    return depth_hist_dev(ctx, ix, probe_dev, opts, max_depth, hist_dev);
} IVJ_ABI_CATCH

int ivj_depth_hist(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, int32_t max_depth, int64_t* hist) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    IVJ_TRY(depth_hist_check(max_depth, hist));
    if (probe->n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    JoinHost J;
    IVJ_TRY(upload_join(ctx, probe, build, opts, 3, J));   // sweep only (no lookup tables) + the end order: what depth_core reads
    const size_t bytes = (size_t)probe->n * (size_t)(max_depth + 1) * 8;
    DevBuf out;
    IVJ_TRY(devbuf_alloc(out, bytes, "depth histogram"));
    IVJ_TRY(depth_hist_dev(ctx, J.h.ix, &J.dp.s, opts, max_depth, (int64_t*)out.p));
    return d2h_finish(ctx, {{hist, out.p, bytes}});
} IVJ_ABI_CATCH

int ivj_depth_hist_contigs_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int32_t max_depth, int64_t* hist_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(depth_hist_check(max_depth, hist_dev));
    DeviceGuard g(ctx->device);
    return depth_hist_contigs_dev(ctx, ix, opts, max_depth, hist_dev);
} IVJ_ABI_CATCH

int ivj_depth_hist_contigs(ivj_ctx* ctx, const ivj_side* frame, const ivj_opts* opts, int32_t max_depth, int64_t* hist) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(frame, "frame"));
    IVJ_TRY(depth_hist_check(max_depth, hist));
    if (opts->n_contigs <= 0) return IVJ_OK;
    const size_t bytes = (size_t)opts->n_contigs * (size_t)(max_depth + 1) * 8;
    if (frame->n == 0) { std::memset(hist, 0, bytes); return IVJ_OK; }
    DeviceGuard g(ctx->device);
    FrameHost F;
    IVJ_TRY(upload_frame(ctx, frame, opts, 3, F));         // sweep only (no lookup tables) + the end order
    DevBuf out;
    IVJ_TRY(devbuf_alloc(out, bytes, "depth histogram"));
    IVJ_TRY(depth_hist_contigs_dev(ctx, F.h.ix, opts, max_depth, (int64_t*)out.p));
    return d2h_finish(ctx, {{hist, out.p, bytes}});
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- depth quantiles (order statistics of the depth, per row)

int ivj_depth_quantiles_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int32_t n_ranks,
                            const int64_t* ranks_dev, int32_t* out_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    IVJ_TRY(depth_quant_check(n_ranks, ranks_dev, out_dev));
    DeviceGuard g(ctx->device);
    return depth_quant_dev(ctx, ix, probe_dev, opts, n_ranks, ranks_dev, out_dev);
} IVJ_ABI_CATCH

int ivj_depth_quantiles(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, int32_t n_ranks, const int64_t* ranks,
                        int32_t* out) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    IVJ_TRY(depth_quant_check(n_ranks, ranks, out));
    if (probe->n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    JoinHost J;
    IVJ_TRY(upload_join(ctx, probe, build, opts, 3, J));   // sweep only (no lookup tables) + the end order: what depth_core reads
    const size_t cells = (size_t)probe->n * (size_t)n_ranks;
    DevBuf buf;                                            // the ranks, then the answers
    IVJ_TRY(devbuf_alloc(buf, cells * 12, "depth quantiles"));
    int64_t* d_ranks = (int64_t*)buf.p;
    int32_t* d_out = (int32_t*)(d_ranks + cells);
    {
        HostXfer copy(ctx->stream, &ctx->xfer);
        copy.h2d(d_ranks, ranks, cells * 8);
        HIP_TRY(copy.finish());
    }
    IVJ_TRY(depth_quant_dev(ctx, J.h.ix, &J.dp.s, opts, n_ranks, d_ranks, d_out));
    return d2h_finish(ctx, {{out, d_out, cells * 4}});
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- set operations on two frames, and their stats

int ivj_setop_dev(ivj_ctx* ctx, ivj_index* ix_a, ivj_index* ix_b, const ivj_opts* opts, int32_t op, int64_t capacity, int32_t* contig_dev,
                  int32_t* start_dev, int32_t* end_dev, int64_t* n_regions) try {
    if (!ctx || !n_regions) return fail(IVJ_EINVAL, "ctx or n_regions is NULL");
    IVJ_TRY(check_opts(opts));
    if (capacity < 0) return fail(IVJ_EINVAL, "capacity < 0");
    DeviceGuard g(ctx->device);
    return setop_core(ctx, ix_a, ix_b, opts, op, capacity, &contig_dev, &start_dev, &end_dev, nullptr, n_regions);
} IVJ_ABI_CATCH

int ivj_set_stats_dev(ivj_ctx* ctx, ivj_index* ix_a, ivj_index* ix_b, const ivj_opts* opts, int64_t bases[3], int64_t* n_intersections) try {
    if (!ctx || !bases || !n_intersections) return fail(IVJ_EINVAL, "ctx, bases or n_intersections is NULL");
    IVJ_TRY(check_opts(opts));
    DeviceGuard g(ctx->device);
    return set_stats_core(ctx, ix_a, ix_b, opts, bases, n_intersections);
} IVJ_ABI_CATCH

void ivj_regions_free(ivj_regions* r) {
    if (!r) return;
    std::free(r->contig); std::free(r->start); std::free(r->end);
    r->contig = r->start = r->end = nullptr; r->n = 0;
}

namespace {
// both sides of a host-path set operation: uploaded and indexed (sweep only + the end order); an empty side stays without an index
struct SetSides {
    FrameHost a, b;
};
int setop_sides(ivj_ctx* ctx, const ivj_side* a, const ivj_side* b, const ivj_opts* opts, SetSides& s) {
    if (a->n > 0) IVJ_TRY(upload_frame(ctx, a, opts, 3, s.a));
    if (b->n > 0) IVJ_TRY(upload_frame(ctx, b, opts, 3, s.b));
    return IVJ_OK;
}
}  // namespace

int ivj_setop(ivj_ctx* ctx, const ivj_side* a, const ivj_side* b, const ivj_opts* opts, int32_t op, ivj_regions* out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    std::memset(out, 0, sizeof(*out));
    IVJ_TRY(check_args(opts, a, "a", b, "b"));
    DeviceGuard g(ctx->device);
    SetSides s;
    IVJ_TRY(setop_sides(ctx, a, b, opts, s));
    DevBuf own;
    int32_t *d_contig = nullptr, *d_start = nullptr, *d_end = nullptr;
    int64_t total = 0;
    IVJ_TRY(setop_core(ctx, s.a.h.ix, s.b.h.ix, opts, op, -1, &d_contig, &d_start, &d_end, &own, &total));
    if (total == 0) return IVJ_OK;
    IVJ_TRY(copy_out_columns(ctx, total, {{(void**)&out->contig, d_contig, 4}, {(void**)&out->start, d_start, 4}, {(void**)&out->end, d_end, 4}},
                             "regions", [&] { ivj_regions_free(out); }));
    out->n = total;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_set_stats(ivj_ctx* ctx, const ivj_side* a, const ivj_side* b, const ivj_opts* opts, int64_t bases[3], int64_t* n_intersections) try {
    if (!ctx || !bases || !n_intersections) return fail(IVJ_EINVAL, "ctx, bases or n_intersections is NULL");
    IVJ_TRY(check_args(opts, a, "a", b, "b"));
    DeviceGuard g(ctx->device);
    SetSides s;
    IVJ_TRY(setop_sides(ctx, a, b, opts, s));
    return set_stats_core(ctx, s.a.h.ix, s.b.h.ix, opts, bases, n_intersections);
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- N frames as position sets (segments, consensus)

int ivj_multi_inter_dev(ivj_ctx* ctx, ivj_index* const* ix, int32_t n_frames, const ivj_opts* opts, int32_t min_frames, int32_t mode,
                        int64_t capacity, int32_t* contig_dev, int32_t* start_dev, int32_t* end_dev, uint64_t* mask_dev, int64_t* n) try {
    if (!ctx || !n) return fail(IVJ_EINVAL, "ctx or n is NULL");
    *n = 0;
    IVJ_TRY(check_opts(opts));
    if (capacity < 0) return fail(IVJ_EINVAL, "capacity < 0");
    DeviceGuard g(ctx->device);
    unsigned long long* mask = (unsigned long long*)mask_dev;
    return multi_core(ctx, ix, n_frames, opts, min_frames, mode, capacity, &contig_dev, &start_dev, &end_dev, &mask, nullptr, n);
} IVJ_ABI_CATCH

void ivj_segments_free(ivj_segments* s) {
    if (!s) return;
    std::free(s->contig); std::free(s->start); std::free(s->end); std::free(s->mask);
    s->contig = s->start = s->end = nullptr; s->mask = nullptr; s->n = 0;
}

namespace {
// the frames of a host-path multi-frame call: uploaded and indexed (sweep only + the end order); an empty frame stays without an
// index (ix[f] stays NULL)
using MultiSides = std::vector<FrameHost>;
int multi_sides(ivj_ctx* ctx, const ivj_side* frames, int32_t n_frames, const ivj_opts* opts, MultiSides& s, std::vector<ivj_index*>& ix) {
    s = MultiSides((size_t)n_frames);
    for (int32_t f = 0; f < n_frames; ++f) {
        if (frames[f].n == 0) continue;
        IVJ_TRY(upload_frame(ctx, &frames[f], opts, 3, s[f]));
        ix[f] = s[f].h.ix;
    }
    return IVJ_OK;
}
}  // namespace

int ivj_multi_inter(ivj_ctx* ctx, const ivj_side* frames, int32_t n_frames, const ivj_opts* opts, int32_t min_frames, int32_t mode,
                    ivj_segments* out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    std::memset(out, 0, sizeof(*out));
    IVJ_TRY(check_opts(opts));
    if (n_frames < 1 || n_frames > IVJ_MAX_FRAMES || !frames)
        return fail(IVJ_EINVAL, "multi_inter: n_frames must be in 1 .. " + std::to_string(IVJ_MAX_FRAMES) + " and frames not NULL");
    for (int32_t f = 0; f < n_frames; ++f) IVJ_TRY(check_side(&frames[f], "frame"));
    std::vector<ivj_index*> ix((size_t)n_frames, nullptr);
    // (the indexes do not exist yet: this call only refuses bad n_frames / min_frames / mode before anything is uploaded)
    IVJ_TRY(multi_check(ix.data(), n_frames, opts, min_frames, mode));
    DeviceGuard g(ctx->device);
    MultiSides s;
    IVJ_TRY(multi_sides(ctx, frames, n_frames, opts, s, ix));
    DevBuf own;
    int32_t *d_contig = nullptr, *d_start = nullptr, *d_end = nullptr;
    unsigned long long* d_mask = nullptr;
    int64_t total = 0;
    IVJ_TRY(multi_core(ctx, ix.data(), n_frames, opts, min_frames, mode, -1, &d_contig, &d_start, &d_end, &d_mask, &own, &total));
    if (total == 0) return IVJ_OK;
    IVJ_TRY(copy_out_columns(ctx, total, {{(void**)&out->contig, d_contig, 4}, {(void**)&out->start, d_start, 4}, {(void**)&out->end, d_end, 4},
                                          {(void**)&out->mask, d_mask, 8, mode == IVJ_MULTI_SEGMENTS}}, "segments", [&] { ivj_segments_free(out); }));
    out->n = total;
    return IVJ_OK;
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- N frames pair by pair (pairwise.hip.h)

int ivj_multi_pairwise_dev(ivj_ctx* ctx, ivj_index* const* ix, int32_t n_frames, const ivj_opts* opts, int64_t* bases_dev, int64_t* runs_dev) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_opts(opts));
    DeviceGuard g(ctx->device);
    return pairwise_core(ctx, ix, n_frames, opts, bases_dev, runs_dev);
} IVJ_ABI_CATCH

int ivj_multi_pairwise(ivj_ctx* ctx, const ivj_side* frames, int32_t n_frames, const ivj_opts* opts, int64_t* bases, int64_t* runs) try {
    if (!ctx || !bases || !runs) return fail(IVJ_EINVAL, "ctx, bases or runs is NULL");
    IVJ_TRY(check_opts(opts));
    if (n_frames < 1 || n_frames > IVJ_MAX_FRAMES || !frames)
        return fail(IVJ_EINVAL, "multi_pairwise: n_frames must be in 1 .. " + std::to_string(IVJ_MAX_FRAMES) + " and frames not NULL");
    for (int32_t f = 0; f < n_frames; ++f) IVJ_TRY(check_side(&frames[f], "frame"));
    std::vector<ivj_index*> ix((size_t)n_frames, nullptr);
    DeviceGuard g(ctx->device);
    MultiSides s;
    IVJ_TRY(multi_sides(ctx, frames, n_frames, opts, s, ix));
    const size_t bytes = (size_t)n_frames * (size_t)n_frames * 8;
    DevBuf out;
    IVJ_TRY(devbuf_alloc(out, 2 * align_up(bytes), "pairwise matrices"));
    int64_t* d_bases = (int64_t*)out.p;
    int64_t* d_runs = (int64_t*)((char*)out.p + align_up(bytes));
    IVJ_TRY(pairwise_core(ctx, ix.data(), n_frames, opts, d_bases, d_runs));
    HostXfer copy(ctx->stream, &ctx->xfer);                // (not d2h_finish: this entry words its copy failure itself)
    copy.d2h(bases, d_bases, bytes);
    copy.d2h(runs, d_runs, bytes);
    const hipError_t e = copy.finish();
    if (e != hipSuccess) return fail(IVJ_EHIP, std::string("D2H(pairwise matrices): ") + hipGetErrorString(e));
    return IVJ_OK;
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- subtract / complement

int ivj_subtract_dev(ivj_ctx* ctx, ivj_index* right_ix, const ivj_side* left_dev, const ivj_opts* opts, int64_t capacity, int32_t* row_dev,
                     int32_t* start_dev, int32_t* end_dev, int64_t* n_pieces) try {
    if (!ctx || !right_ix || !n_pieces) return fail(IVJ_EINVAL, "ctx, index or n_pieces is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(left_dev, "left"));
    if (capacity < 0) return fail(IVJ_EINVAL, "capacity < 0");
    DeviceGuard g(ctx->device);
    return subtract_core(ctx, right_ix, left_dev, opts, capacity, &row_dev, &start_dev, &end_dev, nullptr, n_pieces);
} IVJ_ABI_CATCH

void ivj_pieces_free(ivj_pieces* p) {
    if (!p) return;
    std::free(p->row); std::free(p->start); std::free(p->end);
    p->row = p->start = p->end = nullptr; p->n = 0;
}

int ivj_subtract(ivj_ctx* ctx, const ivj_side* left, const ivj_side* right, const ivj_opts* opts, ivj_pieces* out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    std::memset(out, 0, sizeof(*out));
    IVJ_TRY(check_args(opts, left, "left", right, "right"));
    if (left->n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    JoinHost J;                                            // the left rows probe the index of the right ones
    IVJ_TRY(upload_join(ctx, left, right, opts, 0, J));
    DevBuf own;
    int32_t *d_row = nullptr, *d_start = nullptr, *d_end = nullptr;
    int64_t total = 0;
    IVJ_TRY(subtract_core(ctx, J.h.ix, &J.dp.s, opts, -1, &d_row, &d_start, &d_end, &own, &total));
    if (total == 0) return IVJ_OK;
    IVJ_TRY(copy_out_columns(ctx, total, {{(void**)&out->row, d_row, 4}, {(void**)&out->start, d_start, 4}, {(void**)&out->end, d_end, 4}},
                             "pieces", [&] { ivj_pieces_free(out); }));
    out->n = total;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_complement(ivj_ctx* ctx, const ivj_side* frame, const ivj_side* view, const ivj_opts* opts, ivj_pieces* out) try {
    return ivj_subtract(ctx, view, frame, opts, out);      // the gaps of `frame` inside every view interval
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- row materialisation

int ivj_materialize_dev(ivj_ctx* ctx, const ivj_side* probe_dev, const ivj_side* build_dev, const ivj_rows* rows) try {
    if (!ctx || !rows) return fail(IVJ_EINVAL, "ctx or rows is NULL");
    IVJ_TRY(check_side(probe_dev, "probe"));
    IVJ_TRY(check_side(build_dev, "build"));
    const int64_t n = rows->n_pairs;
    if (n < 0) return fail(IVJ_EINVAL, "n_pairs < 0");
    if (n == 0) return IVJ_OK;
    if (!rows->probe_idx || !rows->build_idx) return fail(IVJ_EINVAL, "pair index columns are NULL");
    DeviceGuard g(ctx->device);
    const bool vec = aligned16(rows->probe_idx) && aligned16(rows->build_idx) && aligned16(rows->contig) && aligned16(rows->start_1) &&
                     aligned16(rows->end_1) && aligned16(rows->start_2) && aligned16(rows->end_2);
    const int64_t per = (int64_t)MAT_THREADS * MAT_ITEMS;
    LAUNCH(ctx, "materialize_keys", k_materialize_keys, (n + per - 1) / per, MAT_THREADS, probe_dev->contig, probe_dev->start, probe_dev->end,
           build_dev->start, build_dev->end, (const int32_t*)rows->probe_idx, (const int32_t*)rows->build_idx, n, vec, rows->contig,
           rows->start_1, rows->end_1, rows->start_2, rows->end_2);
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_take_dev(ivj_ctx* ctx, const void* src_dev, int32_t elem_bytes, const int32_t* idx_dev, int64_t n, void* dst_dev,
                 uint64_t* validity_dev) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    if (elem_bytes != 4 && elem_bytes != 8) return fail(IVJ_EINVAL, "elem_bytes must be 4 or 8");
    if (n < 0) return fail(IVJ_EINVAL, "n < 0");
    if (n == 0) return IVJ_OK;
    if (!src_dev || !idx_dev || !dst_dev) return fail(IVJ_EINVAL, "take: NULL buffer");
    DeviceGuard g(ctx->device);
    if (elem_bytes == 4)
        LAUNCH(ctx, "take", (k_take<uint32_t>), grid1d(n, MAT_THREADS), MAT_THREADS, (const uint32_t*)src_dev, idx_dev, n, (uint32_t*)dst_dev,
               (unsigned long long*)validity_dev);
    else
        LAUNCH(ctx, "take", (k_take<unsigned long long>), grid1d(n, MAT_THREADS), MAT_THREADS, (const unsigned long long*)src_dev, idx_dev, n,
               (unsigned long long*)dst_dev, (unsigned long long*)validity_dev);
    HIP_TRY(hipGetLastError());
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_take(ivj_ctx* ctx, const int32_t* idx, int64_t n, int32_t n_cols, const void* const* src, const int64_t* src_rows,
             const int32_t* elem_bytes, void* const* dst, uint64_t* const* validity) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    if (n < 0 || n_cols < 0) return fail(IVJ_EINVAL, "take: negative size");
    if (n == 0 || n_cols == 0) return IVJ_OK;
    if (!idx || !src || !src_rows || !elem_bytes || !dst) return fail(IVJ_EINVAL, "take: NULL argument");
    size_t max_src = 0, max_dst = 0;
    bool any_valid = false;
    for (int c = 0; c < n_cols; ++c) {
        if (elem_bytes[c] != 4 && elem_bytes[c] != 8) return fail(IVJ_EINVAL, "take: elem_bytes must be 4 or 8");
        if (src_rows[c] < 0 || !dst[c] || (src_rows[c] > 0 && !src[c])) return fail(IVJ_EINVAL, "take: bad column");
        max_src = std::max(max_src, (size_t)src_rows[c] * (size_t)elem_bytes[c]);
        max_dst = std::max(max_dst, (size_t)n * (size_t)elem_bytes[c]);
        any_valid |= validity && validity[c];
    }
    DeviceGuard g(ctx->device);
    const size_t words = (size_t)((n + 63) / 64);
    DevBuf d_idx, d_src, d_dst, d_val;
    IVJ_TRY(devbuf_alloc(d_idx, (size_t)n * 4, "take"));
    IVJ_TRY(devbuf_alloc(d_src, max_src ? max_src : 16, "take"));
    IVJ_TRY(devbuf_alloc(d_dst, max_dst, "take"));
    if (any_valid) IVJ_TRY(devbuf_alloc(d_val, words * 8, "take"));
    HostXfer copy(ctx->stream, &ctx->xfer);
    copy.h2d(d_idx.p, idx, (size_t)n * 4);
    for (int c = 0; c < n_cols; ++c) {
        const size_t sb = (size_t)src_rows[c] * (size_t)elem_bytes[c], db = (size_t)n * (size_t)elem_bytes[c];
        uint64_t* val = validity ? validity[c] : nullptr;
        host_prefault(dst[c], db);
        copy.h2d(d_src.p, src[c], sb);
        HIP_TRY(copy.err);
        int rc = ivj_take_dev(ctx, d_src.p, elem_bytes[c], (const int32_t*)d_idx.p, n, d_dst.p, val ? (uint64_t*)d_val.p : nullptr);
        if (rc != IVJ_OK) return rc;
        copy.d2h(dst[c], d_dst.p, db);
        if (val) copy.d2h(val, d_val.p, words * 8);
        HIP_TRY(copy.finish());                                              // before the device buffers are reused
    }
    HIP_TRY(copy.finish());
    return IVJ_OK;
} IVJ_ABI_CATCH

void ivj_rows_free(ivj_rows* r) {
    if (!r) return;
    int32_t** cols[7] = {&r->probe_idx, &r->build_idx, &r->contig, &r->start_1, &r->end_1, &r->start_2, &r->end_2};
    for (auto c : cols) { std::free(*c); *c = nullptr; }
    r->n_pairs = 0;
}

int ivj_overlap_rows(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, ivj_rows* out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    std::memset(out, 0, sizeof(*out));
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    if (probe->row_id || build->row_id) return fail(IVJ_EINVAL, "ivj_overlap_rows gathers by position: row_id must be NULL");
    DeviceGuard g(ctx->device);
    JoinHost J;
    IVJ_TRY(upload_join(ctx, probe, build, opts, 0, J));
    int64_t total = 0;
    IVJ_TRY(overlap_count(ctx, J.h.ix, &J.dp.s, opts, &total));
    if (total == 0) return IVJ_OK;
    if (!host_result_fits((size_t)total * 28))
        return fail(IVJ_ENOMEM, "the result (" + std::to_string(total) + " rows x 7 columns) does not fit the available host memory");
    DevBuf cols;                                            // 7 columns in one allocation
    const size_t col = align_up((size_t)total * 4);
    IVJ_TRY(devbuf_alloc(cols, 7 * col, "rows"));
    ivj_rows d;
    d.n_pairs = total;
    int32_t** dcols[7] = {&d.probe_idx, &d.build_idx, &d.contig, &d.start_1, &d.end_1, &d.start_2, &d.end_2};
    for (int k = 0; k < 7; ++k) *dcols[k] = (int32_t*)((char*)cols.p + k * col);
    IVJ_TRY(overlap_fill(ctx, J.h.ix, &J.dp.s, opts, d.probe_idx, d.build_idx, total));
    IVJ_TRY(ivj_materialize_dev(ctx, &J.dp.s, &J.db.s, &d));
    int32_t** hcols[7] = {&out->probe_idx, &out->build_idx, &out->contig, &out->start_1, &out->end_1, &out->start_2, &out->end_2};
    HostXfer copy(ctx->stream, &ctx->xfer);
    for (int k = 0; k < 7; ++k) {
        *hcols[k] = (int32_t*)host_result_alloc((size_t)total * 4);
        if (!*hcols[k]) { (void)copy.finish(); ivj_rows_free(out); return fail(IVJ_ENOMEM, "host malloc(rows)"); }
        copy.d2h(*hcols[k], *dcols[k], (size_t)total * 4);
    }
    const hipError_t se = copy.finish();
    if (se != hipSuccess) { ivj_rows_free(out); return fail(IVJ_EHIP, std::string("D2H(rows): ") + hipGetErrorString(se)); }
    out->n_pairs = total;
    return IVJ_OK;
} IVJ_ABI_CATCH

#include "arrow_cdata.hip.h"

void ivj_pairs_free(ivj_pairs* p) {
    if (!p) return;
    std::free(p->probe_idx); std::free(p->build_idx);
    p->probe_idx = nullptr; p->build_idx = nullptr; p->n_pairs = 0;
}

int ivj_count_overlaps(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, int64_t* counts) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    if (probe->n == 0) return IVJ_OK;
    if (!counts) return fail(IVJ_EINVAL, "counts is NULL");
    DeviceGuard g(ctx->device);
    JoinHost J;
    IVJ_TRY(upload_join(ctx, probe, build, opts, 1, J));
    DevBuf dc;
    IVJ_TRY(devbuf_alloc(dc, (size_t)probe->n * 8, "counts"));
    IVJ_TRY(count_overlaps_dev(ctx, J.h.ix, &J.dp.s, opts, (int64_t*)dc.p));
    return d2h_finish(ctx, {{counts, dc.p, (size_t)probe->n * 8}});
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- overlap thresholds (thresh.hip.h, host_thresh.hip.h)

int ivj_overlap_thresh_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_thresholds* thr_dev,
                           int32_t* probe_idx_dev, int32_t* build_idx_dev, int64_t capacity, int64_t* n_pairs) try {
    if (!ctx || !ix || !n_pairs) return fail(IVJ_EINVAL, "ctx, index or n_pairs is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    IVJ_TRY(check_thresholds(thr_dev));
    if (capacity < 0 || (capacity > 0 && (!probe_idx_dev || !build_idx_dev))) return fail(IVJ_EINVAL, "bad output buffers");
    DeviceGuard g(ctx->device);
    return overlap_thresh_dev(ctx, ix, probe_dev, opts, thr_dev, probe_idx_dev, build_idx_dev, capacity, n_pairs);
} IVJ_ABI_CATCH

int ivj_count_overlaps_thresh_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_thresholds* thr_dev,
                                  int64_t* counts_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    IVJ_TRY(check_thresholds(thr_dev));
    if (probe_dev->n > 0 && !counts_dev) return fail(IVJ_EINVAL, "counts is NULL");
    DeviceGuard g(ctx->device);
    ThreshPlan plan;
    return thresh_count(ctx, ix, probe_dev, opts, thr_dev, counts_dev, false, plan, nullptr);
} IVJ_ABI_CATCH

int ivj_overlap_thresh(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr,
                       ivj_pairs* out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    out->n_pairs = 0; out->probe_idx = nullptr; out->build_idx = nullptr;
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    IVJ_TRY(check_thresholds(thr));
    DeviceGuard g(ctx->device);
    ThreshHost H;
    IVJ_TRY(thresh_upload(ctx, probe, build, opts, thr, H));
    ThreshPlan plan;
    int64_t total = 0;
    IVJ_TRY(thresh_count(ctx, H.h.ix, &H.dp.s, opts, &H.dthr, nullptr, true, plan, &total));
    if (total == 0) return IVJ_OK;
    DevPairs P;
    IVJ_TRY(alloc_pairs(total, 8, "; use ivj_overlap_thresh_dev", P));
    IVJ_TRY(thresh_emit(ctx, H.h.ix, plan, (int32_t*)P.p.p, (int32_t*)P.b.p));
    return pairs_to_host(ctx, total, P, out);
} IVJ_ABI_CATCH

int ivj_count_overlaps_thresh(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr,
                              int64_t* counts) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    IVJ_TRY(check_thresholds(thr));
    if (probe->n == 0) return IVJ_OK;
    if (!counts) return fail(IVJ_EINVAL, "counts is NULL");
    DeviceGuard g(ctx->device);
    ThreshHost H;
    IVJ_TRY(thresh_upload(ctx, probe, build, opts, thr, H));
    DevBuf dc;
    IVJ_TRY(devbuf_alloc(dc, (size_t)probe->n * 8, "counts"));
    ThreshPlan plan;
    IVJ_TRY(thresh_count(ctx, H.h.ix, &H.dp.s, opts, &H.dthr, (int64_t*)dc.p, false, plan, nullptr));
    return d2h_finish(ctx, {{counts, dc.p, (size_t)probe->n * 8}});
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- distance window (window.hip.h, host_window.hip.h)

int ivj_overlap_window_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_window* win_dev,
                           int32_t* probe_idx_dev, int32_t* build_idx_dev, int64_t* dist_dev, int64_t capacity, int64_t* n_pairs) try {
    if (!ctx || !ix || !n_pairs) return fail(IVJ_EINVAL, "ctx, index or n_pairs is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    IVJ_TRY(check_window(win_dev));
    if (capacity < 0 || (capacity > 0 && (!probe_idx_dev || !build_idx_dev))) return fail(IVJ_EINVAL, "bad output buffers");
    DeviceGuard g(ctx->device);
    return overlap_window_dev(ctx, ix, probe_dev, opts, win_dev, probe_idx_dev, build_idx_dev, dist_dev, capacity, n_pairs);
} IVJ_ABI_CATCH

int ivj_count_window_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_window* win_dev,
                         int64_t* counts_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    IVJ_TRY(check_window(win_dev));
    if (probe_dev->n > 0 && !counts_dev) return fail(IVJ_EINVAL, "counts is NULL");
    DeviceGuard g(ctx->device);
    WindowPlan plan;
    return window_count(ctx, ix, probe_dev, opts, win_dev, counts_dev, false, plan, nullptr);
} IVJ_ABI_CATCH

void ivj_window_dist_free(int64_t* dist) { std::free(dist); }

int ivj_overlap_window(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_window* win,
                       ivj_pairs* out, int64_t** dist) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    out->n_pairs = 0; out->probe_idx = nullptr; out->build_idx = nullptr;
    if (dist) *dist = nullptr;
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    IVJ_TRY(check_window(win));
    DeviceGuard g(ctx->device);
    WindowHost H;
    IVJ_TRY(window_upload(ctx, probe, build, opts, win, H));
    WindowPlan plan;
    int64_t total = 0;
    IVJ_TRY(window_count(ctx, H.h.ix, &H.dp.s, opts, &H.dwin, nullptr, true, plan, &total));
    if (total == 0) return IVJ_OK;
    DevPairs P;
    IVJ_TRY(alloc_pairs(total, dist ? 16 : 8, "; use ivj_overlap_window_dev", P));
    IVJ_TRY(window_emit(ctx, H.h.ix, plan, (int32_t*)P.p.p, (int32_t*)P.b.p, (int64_t*)P.d.p));
    return pairs_to_host(ctx, total, P, out, dist);
} IVJ_ABI_CATCH

int ivj_count_window(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_window* win,
                     int64_t* counts) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    IVJ_TRY(check_window(win));
    if (probe->n == 0) return IVJ_OK;
    if (!counts) return fail(IVJ_EINVAL, "counts is NULL");
    DeviceGuard g(ctx->device);
    WindowHost H;
    IVJ_TRY(window_upload(ctx, probe, build, opts, win, H));
    DevBuf dc;
    IVJ_TRY(devbuf_alloc(dc, (size_t)probe->n * 8, "counts"));
    WindowPlan plan;
    IVJ_TRY(window_count(ctx, H.h.ix, &H.dp.s, opts, &H.dwin, (int64_t*)dc.p, false, plan, nullptr));
    return d2h_finish(ctx, {{counts, dc.p, (size_t)probe->n * 8}});
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- join kinds: semi, anti, left outer (select.hip.h, host_select.hip.h)

int ivj_overlap_select_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_thresholds* thr_dev,
                           int32_t mode, int32_t* rows_dev, int32_t* pad_dev, int64_t capacity, int64_t* n_rows) try {
    if (!ctx || !ix || !n_rows) return fail(IVJ_EINVAL, "ctx, index or n_rows is NULL");
    *n_rows = 0;
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(probe_dev, "probe"));
    if (thr_dev) IVJ_TRY(check_thresholds(thr_dev));
    IVJ_TRY(check_select_mode(mode));
    if (capacity < 0 || (capacity > 0 && !rows_dev)) return fail(IVJ_EINVAL, "bad output buffers");
    DeviceGuard g(ctx->device);
    return overlap_select_dev(ctx, ix, probe_dev, opts, thr_dev, mode, rows_dev, pad_dev, capacity, n_rows);
} IVJ_ABI_CATCH

void ivj_rowsel_free(ivj_rowsel* r) {
    if (!r) return;
    std::free(r->rows);
    r->rows = nullptr; r->n = 0;
}

int ivj_overlap_select(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr,
                       int32_t mode, ivj_rowsel* out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    out->rows = nullptr; out->n = 0;
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    if (thr) IVJ_TRY(check_thresholds(thr));
    IVJ_TRY(check_select_mode(mode));
    if (probe->n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    SelectHost U;
    IVJ_TRY(select_upload(ctx, probe, build, opts, thr, U));
    SelectPlan S;
    int64_t total = 0;
    IVJ_TRY(select_count(ctx, U.H.h.ix, &U.H.dp.s, opts, U.dthr, mode, S, &total));
    if (total == 0) return IVJ_OK;
    DevBuf rows;
    IVJ_TRY(devbuf_alloc(rows, (size_t)total * 4, "rows"));
    IVJ_TRY(select_emit(ctx, S, (int32_t*)rows.p, nullptr));
    IVJ_TRY(copy_out_columns(ctx, total, {{(void**)&out->rows, rows.p, 4}}, "rows", [&] { ivj_rowsel_free(out); }));
    out->n = total;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_overlap_outer(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr,
                      ivj_pairs* out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    out->n_pairs = 0; out->probe_idx = nullptr; out->build_idx = nullptr;
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    if (thr) IVJ_TRY(check_thresholds(thr));
    if (probe->n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    SelectHost U;
    IVJ_TRY(select_upload(ctx, probe, build, opts, thr, U));
    ivj_index* ix = U.H.h.ix;
    const ivj_side* dp = &U.H.dp.s;
    // the anti rows first: their counts and tile bases stay in the selection scratch while the inner join runs
    SelectPlan S;
    ThreshPlan plan;
    int64_t n_anti = 0, n_inner = 0;
    if (thr) IVJ_TRY(select_count(ctx, ix, dp, opts, U.dthr, IVJ_SELECT_ANTI, S, &n_anti, &plan, &n_inner));
    else {
        IVJ_TRY(select_count(ctx, ix, dp, opts, nullptr, IVJ_SELECT_ANTI, S, &n_anti));
        IVJ_TRY(overlap_count(ctx, ix, dp, opts, &n_inner));
    }
    const int64_t total = n_inner + n_anti;
    if (total == 0) return IVJ_OK;
    DevPairs P;
    IVJ_TRY(alloc_pairs(total, 8, "", P));
    int32_t *op = (int32_t*)P.p.p, *ob = (int32_t*)P.b.p;
    if (n_inner > 0) {
        if (thr) IVJ_TRY(thresh_emit(ctx, ix, plan, op, ob));
        else IVJ_TRY(overlap_fill(ctx, ix, dp, opts, op, ob, n_inner));
    }
    if (n_anti > 0) IVJ_TRY(select_emit(ctx, S, op + n_inner, ob + n_inner));
    return pairs_to_host(ctx, total, P, out);
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- map_overlaps: build-side aggregates per probe row (overlap_agg.hip.h)

int ivj_overlap_agg_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_thresholds* thr_dev,
                        int64_t n_values, int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* agg_out) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    if (n_values < 0) return fail(IVJ_EINVAL, "n_values < 0");
    IVJ_TRY(overlap_agg_check(opts, probe_dev, thr_dev, n_cols, cols, agg_out, ix->n > 0 && n_values > 0));
    DeviceGuard g(ctx->device);
    OaggPlan P;
    IVJ_TRY(overlap_agg_plan(ctx, ix, probe_dev, opts, thr_dev, P));
    for (int32_t k = 0; k < n_cols; ++k) IVJ_TRY(overlap_agg_col(ctx, ix, P, cols[k], n_values, agg_out[k]));
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_overlap_agg(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr,
                    int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* agg_out) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_side(build, "build"));
    IVJ_TRY(overlap_agg_check(opts, probe, thr, n_cols, cols, agg_out, build->n > 0));
    const int64_t n = probe->n, nb = build->n;
    if (n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    SelectHost U;
    IVJ_TRY(select_upload(ctx, probe, build, opts, thr, U));
    ivj_index* ix = U.H.h.ix;
    OaggPlan P;
    IVJ_TRY(overlap_agg_plan(ctx, ix, &U.H.dp.s, opts, U.dthr, P));
    return agg_cols_host(ctx, n, nb, n_cols, cols, agg_out,
                         [&](const ivj_agg_in& in, const ivj_agg_out& dev) { return overlap_agg_col(ctx, ix, P, in, nb, dev); });
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- map_quantiles: order statistics of build values per probe row (overlap_quant.hip.h)

int ivj_overlap_quantiles_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_thresholds* thr_dev,
                              int64_t n_values, const ivj_agg_in* col, int32_t n_q, const double* q, const uint8_t* upper, void* out_dev,
                              int64_t* count_dev) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    if (n_values < 0) return fail(IVJ_EINVAL, "n_values < 0");
    IVJ_TRY(overlap_quant_check(opts, probe_dev, thr_dev, col, n_q, q, out_dev, ix->n > 0 && n_values > 0));
    DeviceGuard g(ctx->device);
    OaggPlan P;
    IVJ_TRY(overlap_agg_plan(ctx, ix, probe_dev, opts, thr_dev, P));
    return overlap_quant_col(ctx, ix, P, *col, n_values, n_q, q, upper, out_dev, count_dev);
} IVJ_ABI_CATCH

int ivj_overlap_quantiles(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr,
                          const ivj_agg_in* col, int32_t n_q, const double* q, const uint8_t* upper, void* out, int64_t* count) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_side(build, "build"));
    IVJ_TRY(overlap_quant_check(opts, probe, thr, col, n_q, q, out, build->n > 0));
    const int64_t n = probe->n, nb = build->n;
    if (n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    SelectHost U;
    IVJ_TRY(select_upload(ctx, probe, build, opts, thr, U));
    ivj_index* ix = U.H.h.ix;
    OaggPlan P;
    IVJ_TRY(overlap_agg_plan(ctx, ix, &U.H.dp.s, opts, U.dthr, P));
    // one block: the value column and its validity bytes, then the answers and the counts
    const size_t val8 = align_up((size_t)(nb + 1) * 8), val1 = align_up((size_t)nb + 1), out8 = align_up((size_t)n * (size_t)n_q * 8);
    DevBuf stage;
    IVJ_TRY(devbuf_alloc(stage, val8 + val1 + out8 + align_up((size_t)n * 8), "value column and quantiles"));
    char* base = (char*)stage.p;
    uint8_t* d_valid = (uint8_t*)(base + val8);
    void* d_out = base + val8 + val1;
    int64_t* d_count = (int64_t*)(base + val8 + val1 + out8);
    const bool with_valid = nb > 0 && col->valid;
    {
        HostXfer copy(ctx->stream, &ctx->xfer);
        if (nb > 0) copy.h2d(base, col->values, (size_t)nb * 8);
        if (with_valid) copy.h2d(d_valid, col->valid, (size_t)nb);
        HIP_TRY(copy.finish());
    }
    const ivj_agg_in in{base, with_valid ? d_valid : nullptr, col->dtype, col->ops};
    IVJ_TRY(overlap_quant_col(ctx, ix, P, in, nb, n_q, q, upper, d_out, d_count));
    return d2h_finish(ctx, {{out, d_out, (size_t)n * (size_t)n_q * 8}, {count, d_count, count ? (size_t)n * 8 : 0}});
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- signal_summary / signal_profile: overlap-weighted build values (signal.hip.h)

int ivj_overlap_wagg_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_thresholds* thr_dev,
                         int64_t n_values, int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* agg_out) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    if (n_values < 0) return fail(IVJ_EINVAL, "n_values < 0");
    IVJ_TRY(overlap_agg_check(opts, probe_dev, thr_dev, n_cols, cols, agg_out, ix->n > 0 && n_values > 0));
    DeviceGuard g(ctx->device);
    OaggPlan P;
    IVJ_TRY(overlap_wagg_plan(ctx, ix, probe_dev, opts, thr_dev, P));
    for (int32_t k = 0; k < n_cols; ++k) IVJ_TRY(overlap_wagg_col(ctx, ix, P, cols[k], n_values, agg_out[k]));
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_overlap_wagg(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr,
                     int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* agg_out) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_side(build, "build"));
    IVJ_TRY(overlap_agg_check(opts, probe, thr, n_cols, cols, agg_out, build->n > 0));
    const int64_t n = probe->n, nb = build->n;
    if (n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    SelectHost U;
    IVJ_TRY(overlap_wagg_upload(ctx, probe, build, opts, thr, U));
    ivj_index* ix = U.H.h.ix;
    OaggPlan P;
    IVJ_TRY(overlap_wagg_plan(ctx, ix, &U.H.dp.s, opts, U.dthr, P));
    return agg_cols_host(ctx, n, nb, n_cols, cols, agg_out,
                         [&](const ivj_agg_in& in, const ivj_agg_out& dev) { return overlap_wagg_col(ctx, ix, P, in, nb, dev); });
} IVJ_ABI_CATCH

int ivj_signal_profile_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* windows_dev, const uint8_t* reverse_dev, int32_t n_bins,
                           const ivj_opts* opts, int64_t n_values, int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* agg_out) try {
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    if (n_values < 0) return fail(IVJ_EINVAL, "n_values < 0");
    IVJ_TRY(signal_profile_check(opts, windows_dev, n_bins, n_cols, cols, agg_out, ix->n > 0 && n_values > 0));
    DeviceGuard g(ctx->device);
    OaggPlan P;
    IVJ_TRY(signal_profile_plan(ctx, ix, windows_dev, n_bins, opts, P));
    for (int32_t k = 0; k < n_cols; ++k)
        IVJ_TRY(signal_profile_col(ctx, ix, P, reverse_dev, windows_dev->n, n_bins, cols[k], n_values, agg_out[k]));
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_signal_profile(ivj_ctx* ctx, const ivj_side* windows, const uint8_t* reverse, int32_t n_bins, const ivj_side* build,
                       const ivj_opts* opts, int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* agg_out) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_side(build, "build"));
    IVJ_TRY(signal_profile_check(opts, windows, n_bins, n_cols, cols, agg_out, build->n > 0));
    if (windows->n == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    return signal_profile_host(ctx, windows, reverse, n_bins, build, opts, n_cols, cols, agg_out);
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- permutation_test: overlap statistics under circular shifts (permute.hip.h)
// (the argument checks come before the context's: they need no device)

int ivj_permute_overlaps_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const int32_t* contig_len_dev,
                             const int32_t* offsets_dev, int64_t n_perm, int64_t* n_pairs_dev, int64_t* n_rows_dev) try {
    IVJ_TRY(permute_check(opts, probe_dev, contig_len_dev, offsets_dev, n_perm, n_pairs_dev, n_rows_dev));
    if (!ctx || !ix) return fail(IVJ_EINVAL, "ctx or index is NULL");
    if (opts->n_contigs != ix->n_contigs) return fail(IVJ_EINVAL, "opts.n_contigs differs from the index's: the tables are laid out by it");
    DeviceGuard g(ctx->device);
    return permute_overlaps_dev(ctx, ix, probe_dev, opts, contig_len_dev, offsets_dev, n_perm, n_pairs_dev, n_rows_dev);
} IVJ_ABI_CATCH

int ivj_permute_overlaps(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const int32_t* contig_len,
                         const int32_t* offsets, int64_t n_perm, int64_t* n_pairs, int64_t* n_rows) try {
    IVJ_TRY(permute_check(opts, probe, contig_len, offsets, n_perm, n_pairs, n_rows));
    IVJ_TRY(check_side(build, "build"));
    const size_t nc = (size_t)opts->n_contigs;
    for (size_t c = 0; c < nc; ++c)
        if (contig_len[c] < 1) return fail(IVJ_EINVAL, "contig_len[" + std::to_string(c) + "] < 1");
    for (int64_t p = 0; p < n_perm; ++p) {
        const int32_t* row = offsets + (size_t)p * nc;
        for (size_t c = 0; c < nc; ++c)
            if (row[c] < 0 || row[c] >= contig_len[c])
                return fail(IVJ_EINVAL, "offsets[" + std::to_string(p) + "][" + std::to_string(c) + "] is outside [0, contig_len)");
    }
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    if (probe->n == 0 || build->n == 0 || nc == 0) {
        std::memset(n_pairs, 0, (size_t)n_perm * 8);
        std::memset(n_rows, 0, (size_t)n_perm * 8);
        return IVJ_OK;
    }
    DeviceGuard g(ctx->device);
    JoinHost J;
    IVJ_TRY(upload_join(ctx, probe, build, opts, 1, J));
    PermPlan P;
    IVJ_TRY(permute_plan(ctx, J.h.ix, &J.dp.s, opts, n_perm, P));
    // the offsets travel in pieces of whole permutations (n_perm x n_contigs may be far more than one allocation should hold)
    const size_t row_bytes = nc * 4;
    int64_t rows_per_piece = (int64_t)(((size_t)64 << 20) / row_bytes);
    rows_per_piece = rows_per_piece < 1 ? 1 : (rows_per_piece > n_perm ? n_perm : rows_per_piece);
    const size_t len_bytes = align_up(row_bytes), out_bytes = align_up((size_t)n_perm * 8), piece_bytes = align_up((size_t)rows_per_piece * row_bytes);
    DevBuf buf;
    IVJ_TRY(devbuf_alloc(buf, len_bytes + 2 * out_bytes + piece_bytes, "permutation tables"));
    int32_t* d_len = (int32_t*)buf.p;
    int64_t* d_pairs = (int64_t*)((char*)buf.p + len_bytes);
    int64_t* d_rows = (int64_t*)((char*)buf.p + len_bytes + out_bytes);
    int32_t* d_off = (int32_t*)((char*)buf.p + len_bytes + 2 * out_bytes);
    HostXfer copy(ctx->stream, &ctx->xfer);
    copy.h2d(d_len, contig_len, row_bytes);
    for (int64_t p0 = 0; p0 < n_perm; p0 += rows_per_piece) {
        // the copies and the launches are ordered by the stream: piece k + 1 overwrites the buffer after piece k's launches ran
        const int64_t np = (n_perm - p0) < rows_per_piece ? (n_perm - p0) : rows_per_piece;
        copy.h2d(d_off, offsets + (size_t)p0 * nc, (size_t)np * row_bytes);
        IVJ_TRY(permute_run(ctx, J.h.ix, P, d_len, d_off, np, d_pairs + p0, d_rows + p0));
    }
    copy.d2h(n_pairs, d_pairs, (size_t)n_perm * 8);
    copy.d2h(n_rows, d_rows, (size_t)n_perm * 8);
    HIP_TRY(copy.finish());
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_nearest(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, int32_t* idx, int64_t* dist,
                int32_t* n_found) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    IVJ_TRY(check_args(opts, probe, "probe", build, "build"));
    if (probe->n == 0) return IVJ_OK;
    if (!idx || !dist || !n_found) return fail(IVJ_EINVAL, "nearest output buffers are NULL");
    const int k = opts->nearest_k < 1 ? 1 : opts->nearest_k;
    if (k > 1024) return fail(IVJ_EINVAL, "nearest_k > 1024");
    DeviceGuard g(ctx->device);
    JoinHost J;
    const bool general = !(k == 1 && opts->include_overlaps);
    IVJ_TRY(upload_join(ctx, probe, build, opts, general ? 1 : 0, J));
    const size_t slots = (size_t)probe->n * (size_t)k;
    DevBuf di, dd, dn;
    IVJ_TRY(devbuf_alloc(di, slots * 4, "nearest"));
    IVJ_TRY(devbuf_alloc(dd, slots * 8, "nearest"));
    IVJ_TRY(devbuf_alloc(dn, (size_t)probe->n * 4, "nearest"));
    IVJ_TRY(nearest_dev(ctx, J.h.ix, &J.dp.s, opts, (int32_t*)di.p, (int64_t*)dd.p, (int32_t*)dn.p));
    return d2h_finish(ctx, {{idx, di.p, slots * 4}, {dist, dd.p, slots * 8}, {n_found, dn.p, (size_t)probe->n * 4}});
} IVJ_ABI_CATCH

// ---------------------------------------------------------------- streaming probe session

int ivj_stream_open(ivj_ctx* ctx, const ivj_side* build, const ivj_opts* opts, int op, int64_t max_batch_rows, ivj_stream** out) try {
    if (!ctx || !out) return fail(IVJ_EINVAL, "ctx or out is NULL");
    *out = nullptr;
    IVJ_TRY(check_opts(opts));
    IVJ_TRY(check_side(build, "build"));
    if (op < IVJ_STREAM_OVERLAP || op > IVJ_STREAM_NEAREST) return fail(IVJ_EINVAL, "op must be IVJ_STREAM_OVERLAP, _COUNT or _NEAREST");
    if (max_batch_rows < 1 || max_batch_rows > 0x7fff0000ll) return fail(IVJ_EINVAL, "max_batch_rows out of range");
    const int k = opts->nearest_k < 1 ? 1 : opts->nearest_k;
    if (op == IVJ_STREAM_NEAREST && k > 1024) return fail(IVJ_EINVAL, "nearest_k > 1024");
    DeviceGuard g(ctx->device);
    ivj_stream* st = new ivj_stream();
    st->ctx = ctx; st->opts = *opts; st->op = op; st->k = k; st->max_rows = max_batch_rows;
    ctx->streams.push_back(st);
    auto bail = [&](int rc) { ivj_stream_close(st); return rc; };
    {
        DevSide db;
        int rc = upload_side(ctx, build, db);
        if (rc != IVJ_OK) return bail(rc);
        const int general = op == IVJ_STREAM_NEAREST && !(k == 1 && opts->include_overlaps);
        rc = index_build(ctx, &db.s, opts, (op == IVJ_STREAM_COUNT || general) ? 1 : 0, &st->ix);
        if (rc != IVJ_OK) return bail(rc);
        hipError_t e = hipStreamSynchronize(ctx->stream);                      // the index copied what it needs: the upload may go
        if (e != hipSuccess) return bail(fail(IVJ_EHIP, std::string("sync(stream open): ") + hipGetErrorString(e)));
    }
    hipError_t e = hipStreamCreateWithFlags(&st->s_h2d, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st->s_d2h, hipStreamNonBlocking);
    const size_t col = align_up((size_t)max_batch_rows * 4);
    for (int s = 0; s < 3 && e == hipSuccess; ++s) {
        ivj_ctx::StreamBufs& cb = ctx->st_cache[s];                            // the staging of the previous session, if it is large enough
        if (cb.h_in && cb.d_in && cb.in_cap >= 3 * col) {
            st->slot[s].h_in = cb.h_in; st->slot[s].d_in = cb.d_in; st->slot[s].in_cap = cb.in_cap;
            st->slot[s].d_out = cb.d_out; st->slot[s].d_out_cap = cb.d_out_cap; st->slot[s].h_out = cb.h_out; st->slot[s].h_out_cap = cb.h_out_cap;
            cb = ivj_ctx::StreamBufs();
        } else {
            e = hipHostMalloc((void**)&st->slot[s].h_in, 3 * col, hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc((void**)&st->slot[s].d_in, 3 * col);
            st->slot[s].in_cap = 3 * col;
        }
        if (e == hipSuccess) e = hipEventCreateWithFlags(&st->slot[s].ev_h2d, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&st->slot[s].ev_join, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&st->slot[s].ev_d2h, hipEventDisableTiming);
    }
    if (e != hipSuccess) return bail(fail(IVJ_ENOMEM, std::string("stream slots: ") + hipGetErrorString(e)));
    *out = st;
    return IVJ_OK;
} IVJ_ABI_CATCH

int ivj_stream_submit(ivj_stream* st, const ivj_side* batch, ivj_stream_result* done) try {
    if (!st || !done) return fail(IVJ_EINVAL, "stream or done is NULL");
    IVJ_TRY(check_side(batch, "batch"));
    if (batch->n > st->max_rows) return fail(IVJ_EINVAL, "batch has more rows than max_batch_rows");
    if (batch->row_id) return fail(IVJ_EINVAL, "stream batches report rows inside the batch: row_id must be NULL");
    if (!st->ctx) return fail(IVJ_ESTATE, "the context of this streaming session was destroyed");
    return stream_turn(st, batch, done);
} IVJ_ABI_CATCH

int ivj_stream_flush(ivj_stream* st, ivj_stream_result* done) try {
    if (!st || !done) return fail(IVJ_EINVAL, "stream or done is NULL");
    if (!st->ctx) return fail(IVJ_ESTATE, "the context of this streaming session was destroyed");
    return stream_turn(st, nullptr, done);
} IVJ_ABI_CATCH

int ivj_stream_set_nearest_ignore(ivj_stream* st, int32_t mask) try {
    if (!st) return fail(IVJ_EINVAL, "stream is NULL");
    if (st->op != IVJ_STREAM_NEAREST) return fail(IVJ_EINVAL, "ivj_stream_set_nearest_ignore needs an IVJ_STREAM_NEAREST session");
    if (mask < 0 || mask > (IVJ_NEAREST_IGNORE_LEFT | IVJ_NEAREST_IGNORE_RIGHT))
        return fail(IVJ_EINVAL, "nearest_ignore must be 0 or a mask of IVJ_NEAREST_IGNORE_LEFT (1) and IVJ_NEAREST_IGNORE_RIGHT (2)");
    st->opts.nearest_ignore = mask;
    return IVJ_OK;
} IVJ_ABI_CATCH

namespace {
// device / pinned resources of a streaming session; the staging goes back to the context's cache when it is still there
void stream_release(ivj_stream* st, bool keep_cache) {
    ivj_ctx* ctx = st->ctx;
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    if (st->s_h2d) (void)hipStreamSynchronize(st->s_h2d);
    if (st->s_d2h) (void)hipStreamSynchronize(st->s_d2h);
    (void)hipStreamSynchronize(ctx->stream);
    for (int s = 0; s < 3; ++s) {
        ivj_stream::Slot& S = st->slot[s];
        ivj_ctx::StreamBufs& cb = ctx->st_cache[s];                            // keep the (larger) staging for the next session
        if (keep_cache && S.h_in && S.d_in && S.in_cap >= cb.in_cap) {
            free_stream_bufs(cb);
            cb.h_in = S.h_in; cb.d_in = S.d_in; cb.in_cap = S.in_cap; cb.d_out = S.d_out; cb.d_out_cap = S.d_out_cap; cb.h_out = S.h_out; cb.h_out_cap = S.h_out_cap;
        } else {
            if (S.h_in) (void)hipHostFree(S.h_in);
            if (S.d_in) (void)hipFree(S.d_in);
            if (S.d_out) (void)hipFree(S.d_out);
            if (S.h_out) (void)hipHostFree(S.h_out);
        }
        if (S.ev_h2d) (void)hipEventDestroy(S.ev_h2d);
        if (S.ev_join) (void)hipEventDestroy(S.ev_join);
        if (S.ev_d2h) (void)hipEventDestroy(S.ev_d2h);
        S = ivj_stream::Slot();
    }
    if (st->s_h2d) (void)hipStreamDestroy(st->s_h2d);
    if (st->s_d2h) (void)hipStreamDestroy(st->s_d2h);
    st->s_h2d = st->s_d2h = nullptr;
    if (st->ix) ivj_index_free(st->ix);
    st->ix = nullptr;
    ctx->streams.erase(std::remove(ctx->streams.begin(), ctx->streams.end(), st), ctx->streams.end());
    st->ctx = nullptr;
}
}  // namespace

void ivj_stream_close(ivj_stream* st) {
    if (!st) return;
    stream_release(st, true);          // no-op when ivj_ctx_destroy already detached the session
    delete st;
}

// ---------------------------------------------------------------- memory helpers

int ivj_dev_alloc(ivj_ctx* ctx, int64_t bytes, void** out) try {
    if (!ctx || !out || bytes < 0) return fail(IVJ_EINVAL, "bad argument");
    DeviceGuard g(ctx->device);
    *out = nullptr;
    if (bytes == 0) return IVJ_OK;
    hipError_t e = hipMalloc(out, (size_t)bytes);
    if (e != hipSuccess) return fail(IVJ_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return IVJ_OK;
} IVJ_ABI_CATCH
int ivj_dev_free(ivj_ctx* ctx, void* p) try {
    if (!ctx) return fail(IVJ_EINVAL, "ctx is NULL");
    if (!p) return IVJ_OK;
    DeviceGuard g(ctx->device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipFree(p));
    return IVJ_OK;
} IVJ_ABI_CATCH
int ivj_memcpy_h2d(ivj_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes) try {
    if (!ctx || bytes < 0) return fail(IVJ_EINVAL, "bad argument");
    if (bytes == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    HostXfer copy(ctx->stream, &ctx->xfer);
    copy.h2d(dst_dev, src_host, (size_t)bytes);
    HIP_TRY(copy.finish());
    return IVJ_OK;
} IVJ_ABI_CATCH
int ivj_memcpy_d2h(ivj_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes) try {
    if (!ctx || bytes < 0) return fail(IVJ_EINVAL, "bad argument");
    if (bytes == 0) return IVJ_OK;
    DeviceGuard g(ctx->device);
    HostXfer copy(ctx->stream, &ctx->xfer);
    copy.d2h(dst_host, src_dev, (size_t)bytes);
    HIP_TRY(copy.finish());
    return IVJ_OK;
} IVJ_ABI_CATCH

}  // extern "C"

#include "host_frontdoor.hip.h"
#include "host_arrow_stream.hip.h"
