/*
 * ivjoin.h -- C ABI of the MI355X-native interval-join engine (libivjoin_hip.so).
 *
 * This is the drop-in boundary for polars-bio's range-operation hot path.  It
 * replaces what the reference reaches through its PyO3 module
 * `polars_bio.polars_bio`:
 *
 *   range_operation_frame(py_ctx, df1, df2, range_options, limit)
 *       /root/reference/src/lib.rs:79-145   (Arrow streams in, joined frame out)
 *   do_range_operation -> do_overlap / do_nearest / do_count_overlaps_coverage_naive
 *       /root/reference/src/operation.rs:27-98, 202-304, 100-200, 306-350
 *   OverlapProvider / NearestProvider / CountOverlapsProvider (IntervalJoinExec + COITrees)
 *       third-party datafusion-bio-function-ranges v0.11.0, call sites
 *       /root/reference/src/operation.rs:146-158, 253-263, 331-340
 *   RangeOptions / FilterOp
 *       /root/reference/src/option.rs:6-41, 95-100
 * and, built on the same sorted index:
 *   the renaming SELECT over the joined batches = row materialisation   src/operation.rs:272-301
 *   do_merge / do_cluster / do_complement / do_subtract / coverage       src/operation.rs:352-510, 86-96
 *       (MergeProvider, ClusterProvider, ComplementProvider, SubtractProvider, CountOverlapsProvider(coverage))
 *   range_operation_lazy + the streaming scan (df1 as an Arrow C stream, lazy result batches, limit)
 *       src/lib.rs:154-214, src/scan.rs:294-357, polars_bio/range_op_io.py:31-174           -> ivj_stream_*
 *
 * Contract: plain pointers and sizes only.  The join keys cross the ABI as
 * three int32 columns per side: `contig` (dictionary id of the chrom string,
 * one dictionary shared by both sides, assigned by the caller), `start`, `end`.
 * Every other column of the user's frames is gathered by the returned row indices
 * (what the reference's SELECT in src/operation.rs:272-301 does with `left_*` /
 * `right_*`): fixed-width columns through HBM (ivj_take, ivj_take_dev), the rest on the host.
 *
 * Side roles (Appendix A of SURVEY.md): probe = df1 (streamed side of the
 * reference), build = df2 (indexed side) for all three operations, i.e. after
 * the swaps in polars_bio/range_op.py:511 and src/operation.rs:143-158.
 *
 * Limits: a side holds at most 0x7fff0000 rows (int32 row indices); the build side at most
 * 2^30 - n_contigs - 32 rows (int32 table offsets).  A context (ivj_ctx) is not thread-safe: use one
 * context per host thread / per device; different contexts may be used concurrently.
 *
 * All entry points return 0 on success, a negative IVJ_E* code otherwise;
 * ivj_last_error() returns the thread-local message of the last failure.
 * The library never retains a caller pointer after the call returns.
 */
#ifndef IVJOIN_H
#define IVJOIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVJ_OK            0
#define IVJ_EINVAL       -1   /* bad argument */
#define IVJ_EHIP         -2   /* HIP runtime error (message has the hipError string) */
#define IVJ_ENOMEM       -3   /* device or host allocation failed */
#define IVJ_ECAPACITY    -4   /* caller-provided output capacity too small */
#define IVJ_ESTATE       -5   /* fill called without a matching count; index lacks what the call needs */
#define IVJ_EPEER        -6   /* multi-rank call: ANOTHER rank failed; this rank's part is complete, the result is not */

/* FilterOp of the reference (src/option.rs:95-100) */
#define IVJ_FILTER_WEAK   0   /* 1-based closed:    a.start <= b.end && b.start <= a.end */
#define IVJ_FILTER_STRICT 1   /* 0-based half-open: a.start <  b.end && b.start <  a.end */

/* ivj_opts.nearest_ignore: the classes of candidate a nearest call leaves out.  For one probe every build row of its contig is in
 * exactly one class -- 0 it overlaps the probe (the filter op's predicate holds), 1 "left": build.start (<) probe.end without an
 * overlap (the row lies before the probe), 2 "right": everything else (it lies after the probe). */
#define IVJ_NEAREST_IGNORE_LEFT  1   /* drop class 1: only overlapping rows and rows after the probe are reported  */
#define IVJ_NEAREST_IGNORE_RIGHT 2   /* drop class 2: only overlapping rows and rows before the probe are reported */

typedef struct ivj_ctx ivj_ctx;      /* one device, one stream, scratch arena */
typedef struct ivj_index ivj_index;  /* sorted build side resident in HBM */

/* One side of the join: three int32 columns of length n.  Host pointers for
 * the host entry points, device pointers for the *_dev entry points.  Rows
 * whose contig id is outside [0, n_contigs) never match anything. */
typedef struct {
    const int32_t* contig;
    const int32_t* start;
    const int32_t* end;
    int64_t n;
    const int32_t* row_id;  /* optional: the row id to report for row i (global ids of a
                               contig shard); NULL = i.  Same memory space as the columns. */
} ivj_side;

/* The subset of RangeOptions (src/option.rs:6-41) that reaches the kernels. */
typedef struct {
    int32_t filter_op;         /* IVJ_FILTER_WEAK | IVJ_FILTER_STRICT */
    int32_t n_contigs;         /* size of the shared chrom dictionary */
    int32_t nearest_k;         /* RangeOptions.nearest_k, >= 1 (default 1) */
    int32_t include_overlaps;  /* RangeOptions.include_overlaps (default 1) */
    int32_t partition_mode;    /* how the probe side is ordered before the join kernels run.  0 auto: overlap (the fused pass and the
                                  count -> fill pair) takes the contig-aligned slice path (6) from 512 Ki probe rows against 64 Ki
                                  build rows on (round 6; rounds 4-5: 1.5 Mi x 256 Ki; dictionaries of <= 256 contigs; tools/policy_sweep.py), large inputs outside
                                  that and the per-probe kernels the 256-bucket path (1), small ones none (2); 1 256 genomic buckets + window-scan kernels (deterministic); 2 never (probe order);
                                  5 flat (256 buckets + load-balanced candidate test, ivj_overlap_fused_dev only; with 0 the
                                  fused entry point picks it by itself when capacity >= 16 pairs per probe row, i.e. for dense
                                  results); 6 LDS-resident index slices: one stable partition into <= 1536 slices of equal
                                  row count + join on the slice held in LDS (overlap count / fill / fused; falls back to 1
                                  when the build side exceeds 1536 x 5120 rows or for the other operations) */
    int32_t table_mode;        /* direct-address table form: 0 auto (16-byte records for build sides >= 2^20 rows; nearest k = 1 over
                                  64-byte LINES -- one fetch per probe, probes in input order -- for build sides >= 2^17 rows once
                                  the probe side is >= 8 x the build side), 1 records, 2 plain 4-byte bins, 3 records + the nearest
                                  lines whatever the sizes (128 bytes of index per build row; other operations: as 1) */
    int32_t slice_rows;        /* slice path: build rows per slice, 0 = auto (rows / 1024, rounded up to 64, <= 5120) */
    int32_t slice_chunk;       /* slice path: probes per work item of the join (round 6: the contig-aligned join's persistent workgroups draw groups of
                                  items and join a bucket's consecutive items as one run; the other slice joins: per workgroup), 0 = auto (multiple of 4096) */
    int32_t deterministic;     /* overlap count -> fill pair on the slice path: 1 = the output is identical from run to run (stable
                                  partition behind a histogram pass, +0.7 ms per 100 M probes); 0 = same pairs, the order of the probe rows inside a
                                  bucket tile may differ between runs (the reference leaves the row order unspecified) */
    int32_t nearest_ignore;    /* nearest only: bit mask of IVJ_NEAREST_IGNORE_LEFT | IVJ_NEAREST_IGNORE_RIGHT, 0 (default) = neither.  The result is
                                  the undirected one -- candidates ordered by (distance, class, build.start, build row) -- with the rows of the
                                  ignored classes removed BEFORE the cut to nearest_k: left still beats right at equal distance, distances
                                  stay non-negative, unused slots are -1.  3 is legal: only overlapping rows can be reported (nothing with
                                  include_overlaps = 0).  Any other value is IVJ_EINVAL.  The mask is uniform over the probe rows of a call:
                                  a caller whose rows differ in orientation (strand) makes one call per orientation, with the mask and its
                                  swap.  Same kernels, same fetches per probe as the undirected call, on every path (partition_mode /
                                  table_mode keep their meaning).  Every entry that runs nearest from an ivj_opts honours it: ivj_nearest,
                                  ivj_nearest_dev, ivj_stream_* (IVJ_STREAM_NEAREST), ivj_nearest_allgather_dev, ivj_nearest_arrow_stream[_lazy] */
} ivj_opts;

/* Result of overlap on the host path: library-owned host buffers. */
typedef struct {
    int64_t n_pairs;
    int32_t* probe_idx;   /* row of df1 */
    int32_t* build_idx;   /* row of df2 */
} ivj_pairs;

/* Per-kernel timing of the last operation (HIP events on the ctx stream). */
typedef struct {
    char name[32];
    int32_t launches;
    float ms;             /* sum over launches */
} ivj_timing;

/* ---- library / context -------------------------------------------------- */
/* The structs of this header carry no size field: a host built against another revision of it would hand the library structs of
 * another length.  IVJ_ABI_VERSION is bumped whenever a struct or a signature changes (5: ivj_opts.deterministic, the lazy Arrow
 * entries, the per-probe all-gathers, ivj_host_scatter; 6: ivj_opts.nearest_ignore appended -- the struct grows from 36 to 40 bytes --
 * and ivj_stream_set_nearest_ignore); a binding checks ivj_abi_version() == the IVJ_ABI_VERSION it was built
 * against right after loading the library (the ctypes binding does: polars_bio_amd/_engine.py::load_library; the Rust sketch in
 * INTEGRATION.md does) and refuses to run otherwise. */
#define IVJ_ABI_VERSION 6
int ivj_abi_version(void);
const char* ivj_last_error(void);
const char* ivj_version(void);
int ivj_device_count(int* n);
/* Host memory (bytes) a result allocation may use right now: MemAvailable of /proc/meminfo (page cache counts as
 * available), MemFree as fallback; the host entry points refuse a result larger than 7/8 of it with IVJ_ENOMEM. */
int64_t ivj_host_mem_available(void);
int ivj_ctx_create(int device, ivj_ctx** out);
void ivj_ctx_destroy(ivj_ctx* ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream; NULL is the
 * HIP legacy default stream, which is what torch uses unless told otherwise).
 * (void*)-1 restores the context's own non-blocking stream. */
int ivj_ctx_set_stream(ivj_ctx* ctx, void* hip_stream);
int ivj_ctx_sync(ivj_ctx* ctx);
/* level 0: off; 1: HIP events around the probe kernels only; 2: around every kernel */
int ivj_ctx_enable_timing(ivj_ctx* ctx, int level);
/* Synchronises, then writes up to cap entries; *n = number of distinct kernels. */
int ivj_ctx_get_timings(ivj_ctx* ctx, ivj_timing* out, int cap, int* n);
/* Launches the empty kernel ivj::k_profile_mark on the context's stream: a step boundary a profiler's kernel trace /
 * counter collection can be cut at (bench.py attributes the PMC bytes of its own run to the timed steps with it). */
int ivj_ctx_profile_mark(ivj_ctx* ctx);

/* ---- host-buffer entry points (what the reference FFI would bind) ------- *
 * Inputs are borrowed host buffers; results come back in host memory.       */

/* pb.overlap: all (probe_row, build_row) pairs.  The pairs of one probe row are contiguous and
 * ordered by (build.start, build row).  Probe rows appear in input order (small inputs, partition_mode 2)
 * or bucket by bucket -- by genomic position of the probe end -- when the probe side was partitioned:
 * with partition_mode 1 (256 buckets) in the stable order of that partition; on the contig-aligned slice
 * path (the automatic choice from 512 Ki probe rows x 64 Ki build rows on) the default partition is the
 * UNORDERED sampled one, so the order of the probe rows inside a bucket (and with it the order of the
 * output) may differ from run to run while the pair SET is exact; opts->deterministic = 1 selects the
 * stable partition there and an output that is identical from run to run.  The reference leaves the row
 * order unspecified (every reference test sorts).  Free with ivj_pairs_free. */
int ivj_overlap(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build,
                const ivj_opts* opts, ivj_pairs* out);
void ivj_pairs_free(ivj_pairs* p);

/* pb.count_overlaps (naive_query=True): counts[i] for every probe row, probe
 * order kept (range_op_helpers.py:315-316: Int64). counts: caller buffer of probe->n. */
int ivj_count_overlaps(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build,
                       const ivj_opts* opts, int64_t* counts);

/* pb.nearest: for every probe row up to k build rows.  idx/dist: caller
 * buffers of probe->n * k (unused slots -1); n_found: probe->n.  Nearest over
 * rows with start > end (on either side) is unspecified. */
int ivj_nearest(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build,
                const ivj_opts* opts, int32_t* idx, int64_t* dist, int32_t* n_found);

/* ---- device-resident entry points (inputs and outputs stay in HBM) ------ *
 * Used by bench.py, the multi-GPU driver and any caller that already holds  *
 * the columns on the GPU.  All work is enqueued on the context stream.      */

/* Sort the build side by (contig, start), derive segment offsets and the
 * prefix-max-of-end array.  with_end_order != 0 additionally sorts the ends
 * (needed by count_overlaps and by nearest with k > 1 or include_overlaps = 0;
 * built on demand otherwise); bit 1 (value 2): sweep-only index for ivj_merge_dev / ivj_cluster_dev -- the
 * lookup tables of the join kernels are not built (every other *_dev call then fails with IVJ_ESTATE).
 * The index copies what it needs: the caller's build columns may be released after the call returns. */
int ivj_index_build_dev(ivj_ctx* ctx, const ivj_side* build_dev, const ivj_opts* opts,
                        int with_end_order, ivj_index** out);
void ivj_index_free(ivj_index* ix);

/* overlap, two calls: count (+ scan, returns the number of pairs after one
 * 8-byte D2H) then fill into caller-allocated device buffers of that size.
 * The per-probe state between the two calls lives in ctx. */
int ivj_overlap_count_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev,
                          const ivj_opts* opts, int64_t* n_pairs);
int ivj_overlap_fill_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev,
                         const ivj_opts* opts, int32_t* probe_idx_dev, int32_t* build_idx_dev,
                         int64_t capacity);

/* overlap in ONE pass for callers that bring an output buffer of known capacity (steady-state /
 * streaming batches: the previous batch sized it): counting and emitting are fused, every tile
 * reserves its output range with one atomic, nothing is written to or re-read from HBM in between.
 * *n_pairs receives the total.  Returns IVJ_ECAPACITY (and writes nothing past the capacity) when
 * the buffer is too small: grow it to *n_pairs and call again, or use the count/fill pair.
 * The pairs of one probe row are contiguous and ordered; the order of the tiles is NOT
 * reproducible from run to run (the count/fill pair is the deterministic path). */
int ivj_overlap_fused_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts,
                          int32_t* probe_idx_dev, int32_t* build_idx_dev, int64_t capacity, int64_t* n_pairs);

int ivj_count_overlaps_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev,
                           const ivj_opts* opts, int64_t* counts_dev);

int ivj_nearest_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev,
                    const ivj_opts* opts, int32_t* idx_dev, int64_t* dist_dev, int32_t* n_found_dev);

/* ---- overlap thresholds: pb.overlap / pb.count_overlaps with min_overlap, min_frac1, min_frac2 -------------------------------------
 * (bedtools intersect -f / -F / -r and a minimum base count).  For a probe (df1) row a and a build (df2) row b of one contig (one
 * group, when the contig column carries group ids):
 *   ov(a, b) = min(a.end, b.end) - max(a.start, b.start)      IVJ_FILTER_STRICT, 0-based half-open;  + 1 for IVJ_FILTER_WEAK, 1-based closed
 *   len(r)   = r.end - r.start                                                                      + 1 for IVJ_FILTER_WEAK
 * The front door offers three optional thresholds, all of which must hold (logical AND):
 *   min_overlap  int >= 1           the pair is kept iff ov >= min_overlap
 *   min_frac1    float in (0, 1]    ... iff ov >= 1 and ov / len(a) >= min_frac1, the division evaluated in IEEE float64 (bedtools -f)
 *   min_frac2    float in (0, 1]    the same test against len(b) (bedtools -F); both = -f X -F Y, both equal = -r
 * Any set threshold implies ov >= 1: rows that cover no position (zero-length rows, start > end) never match on either side,
 * intervals that only touch never match, rows outside the dictionary (a null chrom or on-value) never match.  An "either fraction
 * suffices" mode (bedtools -e) does not exist; the streaming entries (ivj_stream_*, the Arrow-stream entries) and the multi-rank
 * entries take no thresholds.
 * The library sees integers only.  The caller turns each fraction f into a per-row minimum base count m(r) = the smallest integer
 * m >= 1 with m / len(r) >= f in float64 -- ceil(f * len), corrected by one in either direction with the literal division test (IEEE
 * division is monotone in m, so one step each way suffices) -- and "never" for rows with len <= 0.  Minima are uint32: 0 = no
 * requirement, 0xffffffff = never (a closed row can have len = 2^31: ov and the comparison are evaluated in 64 bits).  The test the
 * kernels apply to a pair is the single comparison
 *   ov >= max(1, min_overlap, probe_min[a], build_min[b])           and no match at all where that maximum is 0xffffffff.
 * probe_min: probe->n values, indexed by the row's position in the probe columns (not by row_id).  build_min: one value per build
 * row, indexed by the row the index reports for it (its position in the build columns; for an index built from a side with row_id,
 * ids outside [0, build rows) never match).  The pointers live in the same memory space as the sides.  A struct with nothing set
 * (min_overlap 0, both pointers NULL) is IVJ_EINVAL: the plain entries exist for that.  (New entries and a new struct change no
 * existing struct or signature: IVJ_ABI_VERSION stays.) */
typedef struct {
    uint32_t min_overlap;
    const uint32_t* probe_min;   /* NULL = none */
    const uint32_t* build_min;   /* NULL = none */
} ivj_thresholds;

/* Host path: the pairs as ivj_overlap returns them (library-owned, ivj_pairs_free); count, scan, then emit into an exactly sized
 * buffer.  The pairs of one probe row are contiguous and ordered by (build.start, build row); probe rows appear in input order, or
 * bucket by bucket where the probe side was partitioned (ivj_opts.partition_mode 0 on large inputs, 1, 5, 6; 2 never partitions).
 * The output is identical from run to run. */
int ivj_overlap_thresh(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr,
                       ivj_pairs* out);
/* counts[i] = the kept pairs of probe row i, probe order kept; caller buffer of probe->n. */
int ivj_count_overlaps_thresh(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_thresholds* thr,
                              int64_t* counts);
/* Device path on an index of ivj_index_build_dev (any with_end_order but the sweep-only form).  The capacity contract of
 * ivj_overlap_fused_dev: *n_pairs always receives the total; IVJ_ECAPACITY when it exceeds `capacity`, and nothing is written then.
 * NULL buffers with capacity 0 = count only (IVJ_OK).  Candidate ranges of any length are handled here: there is no hand-over to
 * another kernel.  Blocks until the total is known. */
int ivj_overlap_thresh_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_thresholds* thr_dev,
                           int32_t* probe_idx_dev, int32_t* build_idx_dev, int64_t capacity, int64_t* n_pairs);
/* Per-probe counts only (no pair is enumerated to HBM); enqueued on the context's stream. */
int ivj_count_overlaps_thresh_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_thresholds* thr_dev,
                                  int64_t* counts_dev);

/* ---- distance window: pb.window / pb.count_window -- every build row within a distance of every probe row ------------------------
 * (bedtools window -w / -l / -r / -sw, pyranges join(slack=), bioframe pair_by_distance).  The distance is that of ivj_nearest,
 * evaluated in 64 bits.  For a probe (df1) row a and a build (df2) row b of one contig (one group, when the contig column carries
 * group ids), with (<) = < for IVJ_FILTER_STRICT (0-based half-open) and <= for IVJ_FILTER_WEAK (1-based closed):
 *   gap_right = b.start - a.end      (b lies after a:  !(b.start (<) a.end))
 *   gap_left  = a.start - b.end      (b lies before a: !(a.start (<) b.end))
 *   d(a, b)   = 0 if the rows overlap (b.start (<) a.end && a.start (<) b.end), else max(gap_right, gap_left)
 * Bookended half-open rows do not overlap and have d = 0; adjacent closed rows have d = 1.  Every probe row has a left extent L(a)
 * and a right extent R(a), both in [0, 2^32 - 1]: `left` / `right` for all rows, or -- per pointer, when non-NULL -- probe_left[i] /
 * probe_right[i], indexed by the row's position in the probe columns (not by row_id).  A pair is kept iff ALL of
 *   - both rows cover at least one position (zero-length rows and rows with start > end never pair, on either side);
 *   - d >= min_distance (with min_distance >= 1 overlapping rows drop out);
 *   - the rows overlap, or b lies after a and d <= R(a), or b lies before a and d <= L(a) (a bookended pair, d = 0, counts on the
 *     side it lies on).
 * Rows with a contig id outside [0, n_contigs) (a null chrom or on-value) never pair.  min_distance above both extents is legal
 * and gives the empty result.  On half-open frames `bedtools window -w W` is left = right = W - 1, on closed frames W.
 * The signed distance of a pair is -d when b lies before a in coordinates, d otherwise (0 on overlap); |d| <= 2^32 - 1: int64.
 * Order: the pairs of one probe row are contiguous and ordered by (build.start, build row); probe rows appear in input order, or
 * bucket by bucket where the probe side was partitioned (ivj_opts.partition_mode, as ivj_overlap_thresh).  The output is identical
 * from run to run.  The pointers of the struct live in the same memory space as the sides.  A NULL ivj_window is IVJ_EINVAL; a
 * struct of zeros is valid (overlapping and touching pairs).  The streaming, Arrow-stream and multi-rank entries take no window.
 * (New entries and a new struct change no existing struct or signature: IVJ_ABI_VERSION stays.) */
typedef struct {
    uint32_t left, right;              /* extents of every probe row ...                        */
    const uint32_t* probe_left;        /* ... unless non-NULL: per probe row, by position       */
    const uint32_t* probe_right;
    uint32_t min_distance;             /* 0 = none */
} ivj_window;

/* Host path: the pairs as ivj_overlap returns them (library-owned, ivj_pairs_free); count, scan, then emit into exactly sized
 * buffers.  dist (NULL = not wanted): *dist receives a library-owned column of out->n_pairs signed distances (NULL when there is
 * no pair); free it with ivj_window_dist_free. */
int ivj_overlap_window(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_window* win,
                       ivj_pairs* out, int64_t** dist);
void ivj_window_dist_free(int64_t* dist);
/* counts[i] = the kept pairs of probe row i, probe order kept; caller buffer of probe->n. */
int ivj_count_window(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const ivj_window* win,
                     int64_t* counts);
/* Device path on an index of ivj_index_build_dev (any with_end_order but the sweep-only form).  The capacity contract of
 * ivj_overlap_thresh_dev: *n_pairs always receives the total; IVJ_ECAPACITY when it exceeds `capacity`, and nothing is written then.
 * NULL buffers with capacity 0 = count only (IVJ_OK).  dist_dev (NULL = not wanted): `capacity` int64.  Candidate ranges of any
 * length are handled here.  Blocks until the total is known (one 8-byte D2H). */
int ivj_overlap_window_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_window* win_dev,
                           int32_t* probe_idx_dev, int32_t* build_idx_dev, int64_t* dist_dev, int64_t capacity, int64_t* n_pairs);
/* Per-probe counts only (no pair is enumerated to HBM); enqueued on the context's stream. */
int ivj_count_window_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const ivj_window* win_dev,
                         int64_t* counts_dev);

/* ---- join kinds of pb.overlap other than inner: semi, anti, left outer (bedtools intersect -u / -v / -loj) -------------------------
 * "The predicate" is the plain overlap predicate of ivj_overlap, or -- with a non-NULL ivj_thresholds -- the thresholded one of the
 * section above.  With cnt[i] = what ivj_count_overlaps (ivj_count_overlaps_thresh) returns for probe row i under the very same
 * arguments:
 *   semi   IVJ_SELECT_SEMI   the probe rows with cnt[i] > 0, each once, in ascending row order
 *   anti   IVJ_SELECT_ANTI   the probe rows with cnt[i] == 0, in ascending row order
 *   left   ivj_overlap_outer the inner pairs exactly as the inner join of the same call returns them (ivj_overlap, or
 *                            ivj_overlap_thresh with thresholds), followed by one pair (i, -1) for every anti row i, ascending
 * Rows that can match nothing are anti rows and appear in the left outer join with -1: a null chrom or on-value (contig id < 0), a
 * contig id outside the dictionary (>= n_contigs) and, under thresholds, rows that cover no position or whose own minimum is
 * "never".  An empty build side makes every probe row an anti row.  The semi and anti outputs are identical from run to run.
 * The per-probe counts come from the count kernels as they are, stay in a scratch column of the context and are consumed where they
 * lie by an ordered stream compaction (csrc/select.hip.h): counts and flags never leave the device, no pair is enumerated for semi
 * or anti.  A non-NULL `thr` with nothing set is IVJ_EINVAL, as for the thresholded entries; an unknown `mode` is IVJ_EINVAL.
 * (New entries and a new struct change no existing struct or signature: IVJ_ABI_VERSION stays.) */
#define IVJ_SELECT_SEMI 0
#define IVJ_SELECT_ANTI 1
typedef struct {
    int32_t* rows;     /* selected probe rows, ascending; library-owned (ivj_rowsel_free) */
    int64_t n;
} ivj_rowsel;

/* Host path.  The reported row is the row's position in the probe columns (row_id of a host side is not read, as in ivj_overlap). */
int ivj_overlap_select(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts,
                       const ivj_thresholds* thr /* NULL = plain predicate */, int32_t mode, ivj_rowsel* out);
void ivj_rowsel_free(ivj_rowsel* r);
/* Device path on an index of ivj_index_build_dev (a sweep-only index is IVJ_ESTATE).  The reported id is probe_dev->row_id[position]
 * when the side has row ids, else the position; the ORDER is that of the positions.  The capacity contract of
 * ivj_overlap_thresh_dev: *n_rows always receives the total; IVJ_ECAPACITY when it exceeds `capacity`, and nothing is written then.
 * NULL buffers with capacity 0 = count only (IVJ_OK).  pad_dev (NULL, or `capacity` values) receives -1 at every output position
 * that rows_dev receives a row at: with rows_dev = probe_idx + n_inner and pad_dev = build_idx + n_inner an anti selection appends
 * the unmatched rows of a left outer join behind the inner pairs of the caller's two pair columns.  The two pointers need 4-byte
 * alignment only.  Blocks until the total is known (one 8-byte D2H). */
int ivj_overlap_select_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts,
                           const ivj_thresholds* thr_dev /* NULL = plain predicate */, int32_t mode, int32_t* rows_dev,
                           int32_t* pad_dev /* NULL, or receives -1 */, int64_t capacity, int64_t* n_rows);
/* Left outer join on the host path: the inner pairs from the existing drivers (without thresholds the count -> fill pair of
 * ivj_overlap, with thresholds count -> scan -> emit of ivj_overlap_thresh; their order contracts hold for the inner part), then
 * (row, -1) per anti row, in one buffer sized for both.  Every probe row occurs at least once.  Free with ivj_pairs_free. */
int ivj_overlap_outer(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts,
                      const ivj_thresholds* thr /* NULL = plain predicate */, ivj_pairs* out);

/* ---- row materialisation -------------------- *
 * The step right after the join: gather the columns of both sides for every emitted pair     *
 * (reference: the renaming SELECT of src/operation.rs:272-301 over the joined batches).      *
 * Output columns are Arrow-layout value buffers (fixed-width little-endian values, optional   *
 * validity bitmap, LSB first).                                                               */

/* Key columns of an overlap result, n_pairs values each.  Device pointers for
 * ivj_materialize_dev (caller-allocated; a NULL column is skipped), library-owned host
 * buffers for ivj_overlap_rows (free with ivj_rows_free). */
typedef struct {
    int64_t n_pairs;
    int32_t* probe_idx;   /* row of df1 */
    int32_t* build_idx;   /* row of df2 */
    int32_t* contig;      /* contig id of the pair (equal on both sides) */
    int32_t* start_1;     /* df1.start[probe_idx] */
    int32_t* end_1;
    int32_t* start_2;     /* df2.start[build_idx] */
    int32_t* end_2;
} ivj_rows;

/* Gathers contig / start_1 / end_1 / start_2 / end_2 for the pairs (rows->probe_idx,
 * rows->build_idx) = positions into probe_dev / build_dev, in one pass over the pair list. */
int ivj_materialize_dev(ivj_ctx* ctx, const ivj_side* probe_dev, const ivj_side* build_dev, const ivj_rows* rows);

/* Join AND materialisation in one pass (the fast path: the probe values never leave the workgroup,
 * the build values come with one 16-byte read per row; a separate ivj_materialize_dev over the
 * finished pair list has to fetch the probe columns at random).  rows_dev: device column pointers
 * (NULL = column not wanted), rows_dev->n_pairs = capacity of every column on entry.  Otherwise the
 * contract of ivj_overlap_fused_dev: *n_pairs = total, IVJ_ECAPACITY when it does not fit, rows of one
 * probe contiguous and ordered, tile order not reproducible.  Works with row_id (global ids). */
int ivj_overlap_fused_rows_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts,
                               const ivj_rows* rows_dev, int64_t* n_pairs);

/* Arrow `take` of one fixed-width device column: dst[i] = src[idx[i]]; elem_bytes is 4 or 8.
 * A negative index (the "no candidate" slot of nearest) writes 0 and, when validity_dev is given
 * (ceil(n / 64) 64-bit words), clears that row's validity bit. */
int ivj_take_dev(ivj_ctx* ctx, const void* src_dev, int32_t elem_bytes, const int32_t* idx_dev, int64_t n,
                 void* dst_dev, uint64_t* validity_dev);

/* Host-buffer form of the same `take` for several columns that share ONE index column (the non-key columns of a joined
 * frame: src/operation.rs:272-301 gathers every column of both sides for every pair).  idx (n int32, host) is uploaded
 * once; every column c -- src[c]: src_rows[c] values of elem_bytes[c] = 4 or 8 bytes, host -- is uploaded, gathered in
 * HBM and downloaded into the caller's dst[c] (n values); validity[c] (may be NULL; ceil(n / 64) words) receives the
 * Arrow validity bitmap of the negative-index slots.  The copies go through the context's pinned staging slots (never through
 * hipHostRegister or a pageable hipMemcpy of the caller's pointers); dst is first-touched by a few threads.
 * idx values must be < src_rows[c]. */
int ivj_take(ivj_ctx* ctx, const int32_t* idx, int64_t n, int32_t n_cols, const void* const* src, const int64_t* src_rows,
             const int32_t* elem_bytes, void* const* dst, uint64_t* const* validity);

/* Host-buffer form of overlap + materialisation: index pairs AND the five key columns come back
 * (one H2D of the inputs, join and gathers in HBM, one D2H per column). */
int ivj_overlap_rows(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, ivj_rows* out);
void ivj_rows_free(ivj_rows* rows);

/* Arrow C Data Interface export of an ivj_overlap_rows result as ONE struct array
 * {probe_idx, build_idx, contig, start_1, end_1, start_2, end_2 : int32 not null} without copying:
 * ownership of the host buffers moves to the ArrowArray (its release callback frees them; *rows is
 * cleared).  out_array / out_schema point to caller-allocated `struct ArrowArray` / `struct
 * ArrowSchema` (https://arrow.apache.org/docs/format/CDataInterface.html); a consumer such as
 * pyarrow.RecordBatch._import_from_c takes it from there. */
int ivj_rows_export_arrow(ivj_rows* rows, void* out_array, void* out_schema);

/* ---- sort-scan family: merge / cluster / coverage ---------------- *
 * One sweep over the (contig, start)-sorted index with its prefix max of the ends: a row joins the  *
 * running cluster iff start (<) max end so far + min_dist, (<) = "<" Strict / "<=" Weak.             *
 * Replaces MergeProvider / ClusterProvider / CountOverlapsProvider(coverage = true)               *
 * (src/operation.rs:352-418, 306-350).  min_dist = 0 does not merge bookended half-open intervals   *
 * (tests/_expected.py:174-181).                                                                   */

/* pb.merge result on the host path: library-owned buffers in (contig id, start) order. */
typedef struct {
    int64_t n;
    int32_t* contig;        /* contig id; -1 for the pseudo-contig of rows outside the dictionary */
    int32_t* start;
    int32_t* end;
    int64_t* n_intervals;   /* rows merged into the interval */
} ivj_merged;

int ivj_merge(ivj_ctx* ctx, const ivj_side* frame, const ivj_opts* opts, int64_t min_dist, ivj_merged* out);
void ivj_merged_free(ivj_merged* m);
/* pb.cluster: per input row the cluster id (clusters numbered in (contig id, start) order) and the
 * cluster's bounds; caller buffers of frame->n. */
int ivj_cluster(ivj_ctx* ctx, const ivj_side* frame, const ivj_opts* opts, int64_t min_dist, int64_t* cluster,
                int32_t* cluster_start, int32_t* cluster_end, int64_t* n_clusters);
/* pb.coverage: for every probe row the number of its positions covered by the union of the build
 * intervals of the same contig (Int64, probe order kept; [s, e) Strict, [s, e] Weak). */
int ivj_coverage(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, int64_t* coverage);
/* pb.mean_depth: for every probe row the positions it shares with each build interval of the same contig, summed over the
 * build intervals (Int64, probe order kept; [s, e) Strict, [s, e] Weak) = the integral of the build side's depth over the
 * probe row.  coverage <= bases <= count_overlaps * length.  A row that covers no position gives and receives 0. */
int ivj_overlap_bases(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, int64_t* bases);

/* pb.subtract / pb.complement (SubtractProvider / ComplementProvider, src/operation.rs:420-510): every left
 * interval minus the union of the right intervals of its contig.  Result = the remaining pieces as
 * (left row, start, end), left-row order, ascending inside a row; a fully covered row yields nothing, a row
 * whose contig is absent on the right comes back whole.  Library-owned host buffers. */
typedef struct {
    int64_t n;
    int32_t* row;     /* row of the left side (left->row_id when given) */
    int32_t* start;
    int32_t* end;
} ivj_pieces;

int ivj_subtract(ivj_ctx* ctx, const ivj_side* left, const ivj_side* right, const ivj_opts* opts, ivj_pieces* out);
/* complement = the gaps of `frame` inside every interval of `view` (e.g. one row per chromosome):
 * ivj_subtract(view, frame); row = view row. */
int ivj_complement(ivj_ctx* ctx, const ivj_side* frame, const ivj_side* view, const ivj_opts* opts, ivj_pieces* out);
void ivj_pieces_free(ivj_pieces* p);

/* device-resident forms: the index of the frame / build side is built with ivj_index_build_dev */
/* subtract with the RIGHT side indexed; *n_pieces = total, IVJ_ECAPACITY when it exceeds the capacity of the
 * caller's columns (nothing is written then: grow and call again). */
int ivj_subtract_dev(ivj_ctx* ctx, ivj_index* right_ix, const ivj_side* left_dev, const ivj_opts* opts, int64_t capacity,
                     int32_t* row_dev, int32_t* start_dev, int32_t* end_dev, int64_t* n_pieces);
int ivj_cluster_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int64_t min_dist, int64_t* cluster_dev,
                    int32_t* cluster_start_dev, int32_t* cluster_end_dev, int64_t* n_clusters);
int ivj_merge_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int64_t min_dist, int64_t capacity,
                  int32_t* contig_dev, int32_t* start_dev, int32_t* end_dev, int64_t* n_intervals_dev, int64_t* n_merged);
int ivj_coverage_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int64_t* coverage_dev);
/* The position sums it reads (two uint64 arrays of n + 1 entries) are built on the index's first call and released with it;
 * an index without the end order is completed here.  partition_mode 1 buckets the probes first; 0 and 2 run in probe order. */
int ivj_overlap_bases_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int64_t* bases_dev);

/* pb.depth_profile: every window row cut into n_bins bins, per bin the positions it shares with each build interval of the window's
 * contig, summed over the build intervals -- ivj_overlap_bases of the bin as a probe row -- as a row-major windows->n x n_bins
 * Int64 matrix (caller buffer).  A window covers S .. S + L - 1 ([s, e) Strict: L = e - s, [s, e] Weak: L = e - s + 1); its bin
 * edges in half-open position space are x_j = S + floor(j L / n_bins), j = 0 .. n_bins, bin j = [x_j, x_{j+1}): lengths differ by at
 * most one and sum to L, so a row of the matrix sums to the window's ivj_overlap_bases.  L <= 0: every bin is empty; L < n_bins:
 * some are; an empty bin has 0.  reverse (one byte per window, NULL: none set): a row whose byte is non-zero comes back right to
 * left, column j holding bin n_bins - 1 - j.  1 <= n_bins <= 4096, anything else is IVJ_EINVAL.  Contig ids outside [0, n_contigs)
 * match nothing; build rows that cover no position contribute nothing.  opts->partition_mode is ignored: the windows are read in
 * their own order.  Exact integers; the result is identical from run to run. */
int ivj_depth_profile(ivj_ctx* ctx, const ivj_side* windows, const uint8_t* reverse, int32_t n_bins, const ivj_side* build,
                      const ivj_opts* opts, int64_t* bases);
/* The same on an index already in HBM, windows / reverse / bases in device memory.  An index without the end order or the position
 * sums is completed on its first call, as by ivj_overlap_bases_dev.  Runs on the context's stream; nothing is synchronised. */
int ivj_depth_profile_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* windows_dev, const uint8_t* reverse_dev, int32_t n_bins,
                          const ivj_opts* opts, int64_t* bases_dev);

/* ---- merge with aggregates: a value column reduced per merged interval (bedtools merge -c / -o) -----------------------------------
 * ivj_merge plus, per value column, any of count / sum / min / max / mean over the rows merged into each interval.  The merged
 * table is exactly ivj_merge's for the same input; n_cols value columns share one cluster sweep.  Per column and cluster, over the
 * VALID values only (valid == NULL: all; otherwise valid[row] != 0):
 *   count  int64 number of valid values
 *   sum    int64 columns: accumulated as uint64, i.e. modulo 2^64 (the bits of a wrapping int64 sum); double columns: double.
 *          0 where count == 0.  A NaN value makes the sum and the mean of its cluster NaN.
 *   min / max   the column's type; doubles with fmin / fmax: NaN only where every valid value of the cluster is NaN
 *   mean   (double)sum / (double)count with the sum above (read as int64); float64
 * min, max and mean of a cluster with count == 0 are unspecified (the front door makes them nulls).
 * Values are indexed by the row's position in the frame columns (host form: frame->row_id must be NULL); in the _dev form by the
 * row the index reports (its side's row_id when it had one), and a row outside [0, n_values) contributes nothing, as if invalid.
 * No atomics: integer results are bit-identical from run to run.  A double sum is evaluated in an order fixed by the sorted order
 * of the index, and both index builds (the LSD sort and the balanced bucket build) keep rows of equal (contig, start) in input
 * order, so double sums repeat bit for bit too, for the same input rows in the same order on the same library build.
 * IVJ_EINVAL: n_cols outside [1, IVJ_MAX_AGG_COLS], ops == 0 or with unknown bits, an unknown dtype, NULL values with rows
 * present, a NULL output column of an operation that was asked for (_dev form, once the result fits). */
#define IVJ_AGG_SUM 1u
#define IVJ_AGG_MIN 2u
#define IVJ_AGG_MAX 4u
#define IVJ_AGG_MEAN 8u
#define IVJ_AGG_COUNT 16u
#define IVJ_AGG_I64 0
#define IVJ_AGG_F64 1
#define IVJ_MAX_AGG_COLS 16
typedef struct {
    const void* values;      /* int64 or double, one per row */
    const uint8_t* valid;    /* one byte per row, 1 = use the value; NULL = all valid */
    int32_t dtype;           /* IVJ_AGG_I64 / IVJ_AGG_F64 */
    uint32_t ops;            /* mask of IVJ_AGG_* */
} ivj_agg_in;
typedef struct {
    void* sum;               /* int64 (wrapped) / double */
    void* min;               /* the column's type */
    void* max;
    double* mean;
    int64_t* count;          /* each: NULL where not asked for */
} ivj_agg_out;

/* Host form: out and agg_out[0 .. n_cols) receive library-owned buffers of out->n entries (only the operations asked for),
 * released by ivj_merge_agg_free. */
int ivj_merge_agg(ivj_ctx* ctx, const ivj_side* frame, const ivj_opts* opts, int64_t min_dist, int32_t n_cols,
                  const ivj_agg_in* cols, ivj_merged* out, ivj_agg_out* agg_out);
void ivj_merge_agg_free(ivj_merged* m, ivj_agg_out* agg_out, int32_t n_cols);
/* Device form, the capacity protocol of ivj_merge_dev: *n_merged always receives the total; IVJ_ECAPACITY when it exceeds
 * `capacity`, and nothing is written then.  cols[k].values / valid are device pointers to n_values elements; agg_out[k] holds
 * the caller's device columns of `capacity` elements (operations not asked for are not written). */
int ivj_merge_agg_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int64_t min_dist, int64_t capacity, int32_t* contig_dev,
                      int32_t* start_dev, int32_t* end_dev, int64_t* n_intervals_dev, int64_t n_values, int32_t n_cols,
                      const ivj_agg_in* cols, const ivj_agg_out* agg_out, int64_t* n_merged);

/* ---- map_overlaps: build-side value columns reduced over each probe row's overlaps (bedtools map -c / -o) --------------------------
 * For every probe (df1) row a, over the build (df2) rows b that match a, and per value column of the BUILD side over the VALID
 * values only: count / sum / min / max / mean exactly as ivj_merge_agg defines them per cluster (count int64; an integer sum
 * accumulated as uint64, i.e. a wrapping int64; doubles with fmin / fmax, a NaN value makes sum and mean NaN;
 * mean = (double)sum / (double)count).  sum is 0 and count is 0 where nothing valid matches; min / max / mean are unspecified
 * there (the front door makes them nulls).
 * "Matches" with thr == NULL is the plain join's predicate for opts->filter_op, bit for bit: the count of a column without nulls
 * equals ivj_count_overlaps of the same call, rows that cover no position included.  With an ivj_thresholds it is the thresholded
 * predicate ov >= max(1, min_overlap, probe_min[a], build_min[b]), "never" honoured: the count then equals
 * ivj_count_overlaps_thresh.  A non-NULL thr with nothing set is IVJ_EINVAL.
 * Values are indexed by the row the index reports for a build position (host form: the row's position in the build columns); a
 * row outside [0, n_values) contributes nothing, as in ivj_merge_agg_dev.  Results are written at the probe's position in the
 * caller's columns -- one entry per probe row, in probe order, also where the probes are bucketed internally (partition_mode); a
 * probe row_id is ignored.  A probe row outside the dictionary (null chrom or on-value) gets count 0.  There is no capacity
 * protocol: every output column holds probe->n entries.  Operations not asked for are not written.
 * No pair is enumerated and there is no atomic, floating-point or other: integer results are bit-identical from run to run.  A
 * double sum is evaluated in an order fixed by the sorted order of the index and the kernel's geometry (csrc/overlap_agg.hip.h),
 * and both index builds keep rows of equal (contig, start) in input order, so double sums repeat bit for bit too, for the same
 * input rows in the same order on the same library build.  Which of -0.0 / +0.0 a double min / max returns when both occur is
 * unspecified.  The cost is one sweep over the CANDIDATES (not the matches) per value column.
 * IVJ_EINVAL as for ivj_merge_agg: n_cols outside [1, IVJ_MAX_AGG_COLS], ops == 0 or with unknown bits, an unknown dtype, NULL
 * values with build rows present, a NULL output column of an operation that was asked for (with probe rows present).
 * IVJ_ESTATE: an index without lookup tables (with_end_order & 2).
 * (New entries change no existing struct or signature: IVJ_ABI_VERSION stays.) */
/* Host form: agg_out[k].* are CALLER-owned host columns of probe->n entries (NULL where not asked for). */
int ivj_overlap_agg(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts,
                    const ivj_thresholds* thr /* NULL = plain predicate */, int32_t n_cols, const ivj_agg_in* cols /* over build rows */,
                    const ivj_agg_out* agg_out);
/* Device form on an index of ivj_index_build_dev: values / valid / outputs are device pointers, n_values = rows behind
 * cols[k].values; enqueued on the context's stream. */
int ivj_overlap_agg_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts,
                        const ivj_thresholds* thr_dev /* NULL = plain predicate */, int64_t n_values, int32_t n_cols,
                        const ivj_agg_in* cols, const ivj_agg_out* agg_out);

/* ---- map_quantiles: exact quantiles of a build-side value column over each probe row's overlaps (bedtools map -o median) -------------
 * For a probe (df1) row a take the build (df2) rows that match a -- "match" as ivj_overlap_agg defines it for the same call: the
 * plain predicate with thr == NULL, the thresholded one with an ivj_thresholds -- and whose value is valid (a row outside
 * [0, n_values) is invalid; a probe outside the dictionary matches nothing).  Let m be their number and v[0] <= ... <= v[m - 1]
 * their values in ascending order: int64 columns in signed order, double columns in the order of a numeric sort with NaN last,
 * -inf < ... < -0.0 = +0.0 < ... < +inf < NaN; every NaN is one value and comes back as the canonical quiet NaN; which zero is
 * returned where both signs tie at a rank is unspecified.  For each of the n_q requests (q[j] in [0, 1], upper[j] in {0, 1};
 * upper == NULL: all 0), shared by all rows:
 *     h = q[j] * (double)(m - 1)   (one IEEE round-to-nearest product),   rank = upper[j] ? ceil(h) : floor(h),
 *     out[a * n_q + j] = v[rank],   count[a] = m;
 * where m == 0, out[a * n_q + *] is written as all-zero bits and count[a] = 0.  col is ONE build column (ivj_agg_in; ops is
 * ignored); out holds the column's 8-byte type.  Results are in probe order whatever opts->partition_mode; a probe row_id is
 * ignored.  No pair is enumerated, nothing is sorted and there is no global atomic: results are identical from run to run.
 * The kernel (csrc/overlap_quant.hip.h) is a radix select over the candidates of each row, IVJ_OVQ_BITS bits per pass, with a
 * 2^IVJ_OVQ_BITS-bin 32-bit histogram per (row, request) in LDS; a workgroup owns
 * P = floor(IVJ_OVQ_LDS_BYTES / (n_q * 2^IVJ_OVQ_BITS * 4)) consecutive probe rows, clamped to [1, IVJ_OVQ_MAX_TILE] (informative:
 * the result does not depend on them; IVJ_OVQ_BITS may be set when the library is compiled, 4 .. 8).
 * Cost: per CANDIDATE of the probe's loose range (not per match) one 16-byte record and the predicate, per match 8 value bytes
 * and up to n_q LDS reads and adds -- paid 1 + npass times, npass = the number of IVJ_OVQ_BITS-bit digits in which the keys under
 * a workgroup's rows differ (at most ceil(64 / IVJ_OVQ_BITS); few for small integers and for float32 values of one sign widened to double).
 * IVJ_EINVAL: n_q outside [1, IVJ_MAX_OVQ_RANKS], a q outside [0, 1] or NaN, an unknown dtype, NULL values with build rows
 * present, a NULL out with probe rows present, a non-NULL thr with nothing set.  IVJ_ESTATE: an index without lookup tables
 * (with_end_order & 2).  (New entries change no existing struct or signature: IVJ_ABI_VERSION stays.) */
#define IVJ_MAX_OVQ_RANKS 16
#ifndef IVJ_OVQ_BITS
#define IVJ_OVQ_BITS 4
#endif
#define IVJ_OVQ_LDS_BYTES 49152
#define IVJ_OVQ_MAX_TILE 512
/* Host form: out (probe->n x n_q, row-major) and count (probe->n entries; may be NULL) are CALLER-owned host buffers. */
int ivj_overlap_quantiles(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts,
                          const ivj_thresholds* thr /* NULL = plain predicate */, const ivj_agg_in* col /* ONE build column, ops ignored */,
                          int32_t n_q, const double* q, const uint8_t* upper, void* out, int64_t* count);
/* Device form on an index of ivj_index_build_dev: values / valid / out / count are device pointers, n_values = rows behind
 * col->values; q and upper are HOST arrays of n_q entries; enqueued on the context's stream. */
int ivj_overlap_quantiles_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts,
                              const ivj_thresholds* thr_dev /* NULL = plain predicate */, int64_t n_values, const ivj_agg_in* col,
                              int32_t n_q, const double* q /* HOST */, const uint8_t* upper /* HOST */, void* out_dev, int64_t* count_dev);

/* ---- signal_summary / signal_profile: build-side values weighted by the positions they share with the probe ------------------------
 * The build (df2) side read as a signal track, (contig, start, end, value) rows as in a bedGraph: what bigWigAverageOverBed and
 * deepTools computeMatrix compute.  For a probe row a and a build row b of one contig
 *     ov(a, b) = min(a.end, b.end) - max(a.start, b.start)   (+ 1 for closed frames, Weak), in 64 bits
 * and b CONTRIBUTES to a iff ov >= max(1, min_overlap, probe_min[a], build_min[b]) ("never" honoured) and its value is valid.
 * thr == NULL leaves ov >= 1: rows of either side that cover no position share nothing, as in ivj_overlap_bases.  This is the
 * thresholded predicate, NOT the plain one of ivj_overlap_agg with thr == NULL, which also counts rows that cover no position.
 * Per value column of the build side, over the contributing rows (columns and outputs as ivj_agg_in / ivj_agg_out):
 *   count  receives BASES = the sum of ov, accumulated as uint64 (modulo 2^64).  With a column without nulls and thr == NULL this
 *          is ivj_overlap_bases; build rows that overlap each other count with their multiplicity.
 *   sum    the sum of value * ov.  int64 columns: the product and the sum as uint64, i.e. the bits of a wrapping int64.  double
 *          columns: value * (double)ov rounded once per row (ov <= 2^32 is exact), then added.  0 where bases == 0.
 *   min / max   over the contributing VALUES, unweighted; doubles with fmin / fmax (NaN only where every value is NaN)
 *   mean   (double)sum / (double)bases, the sum read as int64 for integer columns
 * min, max and mean of a probe with bases == 0 are unspecified (the front door makes them nulls).  A NaN value makes sum and mean NaN.
 * Values are indexed, results are placed, probes outside the dictionary are treated and a probe row_id is ignored as by
 * ivj_overlap_agg.  Operations not asked for are not written.
 * No pair is enumerated and there is no atomic: integer results are bit-identical from run to run; a double sum is evaluated in
 * an order fixed by the sorted order of the index and the kernel's geometry (csrc/overlap_agg.hip.h, csrc/signal.hip.h) and
 * repeats bit for bit for the same input rows in the same order on the same library build.
 * Cost: one record, one predicate and one scan step per CANDIDATE of the probe's loose range, per value column.
 * IVJ_EINVAL and IVJ_ESTATE as for ivj_overlap_agg.  (New entries change no existing struct or signature: IVJ_ABI_VERSION stays.) */
int ivj_overlap_wagg(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts,
                     const ivj_thresholds* thr /* NULL = ov >= 1 */, int32_t n_cols, const ivj_agg_in* cols /* over build rows */,
                     const ivj_agg_out* agg_out /* caller-owned host columns of probe->n entries */);
int ivj_overlap_wagg_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts,
                         const ivj_thresholds* thr_dev /* NULL = ov >= 1 */, int64_t n_values, int32_t n_cols,
                         const ivj_agg_in* cols, const ivj_agg_out* agg_out);
/* The same statistics per BIN of every window row: the windows are cut as by ivj_depth_profile (x_j = S + floor(j L / n_bins),
 * bin j = [x_j, x_{j+1}), 1 <= n_bins <= 4096, reverse as there) and every bin is a probe of ivj_overlap_wagg with thr == NULL, made
 * on the device from the 12 bytes of its window: no bin frame exists in memory.  Every output column that was asked for is a
 * row-major windows->n x n_bins matrix (caller buffer); an empty bin gets bases 0 and sum 0.  With a column of ones without nulls
 * the bases matrix is ivj_depth_profile's; a row of the bases / sum matrices adds up to the window's ivj_overlap_wagg.
 * opts->partition_mode is ignored: the windows are read in their own order.  There are no per-bin thresholds.
 * Cost: as above per candidate of every BIN: a build row that spans k bins is visited k times, which suits tracks of short rows
 * and not contig-wide rows.  IVJ_EINVAL: as ivj_overlap_wagg, and n_bins out of range; IVJ_ESTATE: an index without lookup tables. */
int ivj_signal_profile(ivj_ctx* ctx, const ivj_side* windows, const uint8_t* reverse, int32_t n_bins, const ivj_side* build,
                       const ivj_opts* opts, int32_t n_cols, const ivj_agg_in* cols /* over build rows */,
                       const ivj_agg_out* agg_out /* caller-owned host matrices of windows->n * n_bins entries */);
int ivj_signal_profile_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* windows_dev, const uint8_t* reverse_dev, int32_t n_bins,
                           const ivj_opts* opts, int64_t n_values, int32_t n_cols, const ivj_agg_in* cols, const ivj_agg_out* agg_out);

/* ---- permutation_test: overlap statistics of the probe side under circular shifts (regioneR circularRandomizeRegions) ---------------
 * Half-open coordinates: hs = start - (Weak ? 1 : 0), he = end; contig c covers [0, contig_len[c]), contig_len[c] >= 1.
 * offsets is an int32 table, row-major n_perm x opts->n_contigs, 0 <= offsets[p][c] < contig_len[c].
 * A probe row takes part iff its contig is inside the dictionary and 0 <= hs < he <= contig_len[c]; any other row (no position,
 * inverted, beyond the contig's end, outside the dictionary) contributes nothing to any permutation.  In permutation p a row is
 *     s' = (hs + offsets[p][c]) mod L,  e' = s' + (he - hs)      (64-bit: e' reaches 2 L - 1)
 * the single piece [s', e') when e' <= L, otherwise the two pieces [s', L) and [0, e' - L).  A piece matches a build row iff they
 * share at least one position (the thresholded predicate with min_overlap = 1); build rows that cover no position never match.
 *     n_pairs[p] = matches summed over the probe rows and their pieces -- a build row that reaches BOTH pieces of a wrapped row
 *                  counts twice;
 *     n_rows[p]  = probe rows with at least one match in any piece.
 * A row of zero offsets gives the observed statistics.  Nothing per row or per pair exists in device memory, there is no atomic,
 * and the results are identical from run to run.  Every opts->partition_mode routes to the one form.
 * IVJ_EINVAL: n_perm < 1 or > 2^20, a NULL table (with n_contigs > 0) or a NULL output.
 * IVJ_ESTATE: an index without lookup tables (with_end_order & 2).
 * (New entries change no existing struct or signature: IVJ_ABI_VERSION stays.) */
/* Host form: every pointer is host memory, n_pairs / n_rows hold n_perm entries.  Also IVJ_EINVAL for a contig_len < 1 or an
 * offset outside [0, contig_len). */
int ivj_permute_overlaps(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const int32_t* contig_len,
                         const int32_t* offsets, int64_t n_perm, int64_t* n_pairs, int64_t* n_rows);
/* Device form on an index of ivj_index_build_dev (opts->n_contigs must be the index's): every pointer is device memory; enqueued on
 * the context's stream.  Lengths and offsets are NOT validated: with values outside the ranges above the statistics are
 * unspecified, but the kernel never reads outside the tables or the index whatever the values are (they only form 64-bit search
 * targets that are clamped to the index's grid). */
int ivj_permute_overlaps_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const int32_t* contig_len_dev,
                             const int32_t* offsets_dev, int64_t n_perm, int64_t* n_pairs_dev, int64_t* n_rows_dev);

/* ---- depth: run-length coverage blocks of one frame ------------------------------------------------------------------------------
 * The disjoint maximal runs of positions covered by the same number (>= 1) of the frame's rows, in (contig id, start) order: the
 * block form (chrom, start, end, coverage) of the reference's pb.depth (polars_bio/pileup_op.py:94-100), computed from an interval
 * frame instead of an alignment file.  Strict: a row covers [start, end), blocks are half-open.  Weak: a row covers [start, end],
 * blocks are closed (so [1,5] and [6,9] at depth 1 are the one block [1,9]).  Events at one position are netted first: neighbouring
 * blocks differ in depth unless a gap or a contig boundary lies between them.  Zero-depth gaps are not reported (ivj_complement
 * gives them).  Rows that cover no position (Strict start >= end, Weak start > end) and rows outside the dictionary contribute
 * nothing; a frame with a row of start > end is indexed a second time without such rows (slower, same result).  depth is int32
 * (bounded by the row count), at most 2 n blocks come back, and the result is bit-identical from run to run. */
typedef struct {
    int64_t n;
    int32_t* contig;
    int32_t* start;
    int32_t* end;
    int32_t* depth;
} ivj_blocks;

/* Host path: library-owned buffers, released by ivj_blocks_free. */
int ivj_depth(ivj_ctx* ctx, const ivj_side* frame, const ivj_opts* opts, ivj_blocks* out);
void ivj_blocks_free(ivj_blocks* b);
/* Device path, the capacity protocol of ivj_merge_dev: *n_blocks always receives the total; IVJ_ECAPACITY when it exceeds
 * `capacity`, and nothing is written then.  An index built without the end order (with_end_order bit 0) is completed on demand;
 * a sweep-only index (bit 1) is accepted. */
int ivj_depth_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int64_t capacity, int32_t* contig_dev, int32_t* start_dev,
                  int32_t* end_dev, int32_t* depth_dev, int64_t* n_blocks);

/* pb.depth_summary: per probe row how deep the build side's pile gets under it, and how much of it is covered at least T deep (the
 * columns of `mosdepth --thresholds` and of `bedtools map -o max` on a bedGraph).  With d(c, x) = the number of build rows of
 * contig c that cover position x (the depth of ivj_depth, same conventions: [s, e) Strict, [s, e] Weak; rows that cover no
 * position and rows outside the dictionary contribute nothing and, as probes, receive 0 in every column) and Q = the positions of
 * probe row q on contig c:
 *   max_depth[q]   = max over x in Q of d(c, x)                 (int32; 0 when Q is empty or nothing covers it)
 *   bases_ge[k][q] = |{x in Q : d(c, x) >= thresholds[k]}|      (int64: a Weak probe [INT32_MIN, INT32_MAX] has 2^32 positions)
 * bases_ge is COLUMN-MAJOR: n_thresholds columns of probe->n int64, column k belongs to thresholds[k], in the caller's order.
 * Thresholds may come in any order and may repeat; each must be >= 1; n_thresholds in [0, IVJ_MAX_THRESHOLDS].  max_depth may be
 * NULL (thresholds only); bases_ge may be NULL only when n_thresholds == 0.  IVJ_EINVAL: n_thresholds outside its range,
 * thresholds NULL with n_thresholds > 0, a threshold < 1, both outputs NULL, and bases_ge NULL with n_thresholds > 0 (all of
 * them whatever probe->n is).  bases_ge[T = 1] = ivj_coverage; the sum of bases_ge[T] over T = 1 .. max depth = ivj_overlap_bases;
 * max_depth <= ivj_count_overlaps.  Probe order is kept; no atomics, no capacity protocol: bit-identical from run to run. */
#define IVJ_MAX_THRESHOLDS 8
int ivj_depth_summary(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, const int32_t* thresholds,
                      int32_t n_thresholds, int32_t* max_depth, int64_t* bases_ge);
/* The same on an index of ivj_index_build_dev (any form: a missing end order is completed on demand, a sweep-only index is
 * accepted, as ivj_depth_dev); probe columns and outputs in HBM, `thresholds` on the host.  An empty index, or one whose blocks
 * come out empty, zero-fills the outputs.  Every call derives the depth blocks, their index, a 64-bit threshold prefix table and a
 * tree of depth maxima, and releases them before it returns (it waits for the stream): nothing is cached on the index.
 * partition_mode 0, 1 and 2 all run in probe order and return identical arrays.  The blocks (at most 2 n) must fit the index
 * limit of ivj_index_build_dev. */
int ivj_depth_summary_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, const int32_t* thresholds,
                          int32_t n_thresholds, int32_t* max_depth_dev, int64_t* bases_ge_dev);

/* pb.depth_histogram / pb.genome_depth_histogram: the distribution of the build side's depth (bedtools genomecov's default output,
 * bedtools coverage -hist, mosdepth's dist), with d(c, x), the conventions and Q of ivj_depth_summary above, D = max_depth in
 * [1, IVJ_MAX_HIST_DEPTH] and max_depth + 1 bins per row (at most 8 KiB):
 *   region form, per probe row q      hist[q][d] = |{x in Q : d(c, x) == d}| for 0 <= d < D,  hist[q][D] = |{x in Q : d(c, x) >= D}|
 *   contig form, per contig c         hist[c][d] = the same count over all positions of contig c for 1 <= d <= D,  hist[c][0] = 0
 * (the library does not know a contig's length: the caller fills bin 0 of the contig form).  Both are int64, ROW-major: probe->n
 * resp. opts->n_contigs rows of max_depth + 1.  A row of the region form sums to |Q|, bin 0 holds its uncovered positions; a
 * probe that covers no position or lies outside the dictionary gets a row of zeros.  An empty build side, or one whose blocks
 * come out empty, gives zeros, except bin 0 of the region form, which is |Q|.  Identities: with hist of the region form,
 * sum over d >= T of hist[q][d] = bases_ge[T] of ivj_depth_summary for T <= D (T = 1: ivj_coverage); when D exceeds every depth,
 * sum over d of d * hist[q][d] = ivj_overlap_bases and the highest non-zero bin = max_depth of ivj_depth_summary; summing the
 * contig form's rows gives the histogram of the blocks of ivj_depth.  IVJ_EINVAL: max_depth outside its range and hist NULL
 * (whatever the row count).  No capacity protocol; integer adds only: bit-identical from run to run.
 * (New entries change no existing struct or signature: IVJ_ABI_VERSION stays.) */
#define IVJ_MAX_HIST_DEPTH 1023
/* The region form's kernel gives a workgroup P = floor(IVJ_HIST_LDS_BYTES / ((max_depth + 1) * 8)) consecutive probe rows,
 * clamped to [1, IVJ_HIST_MAX_TILE] (informative: the result does not depend on it). */
#define IVJ_HIST_LDS_BYTES 65536
#define IVJ_HIST_MAX_TILE 512
int ivj_depth_hist(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, int32_t max_depth, int64_t* hist);
int ivj_depth_hist_contigs(ivj_ctx* ctx, const ivj_side* frame, const ivj_opts* opts, int32_t max_depth, int64_t* hist);
/* The same on an index of ivj_index_build_dev (any form: a missing end order is completed on demand, a sweep-only index is
 * accepted, as ivj_depth_summary_dev); probe columns and hist in HBM.  Every call derives the depth blocks and, for the region
 * form, their index and 16-byte records, walks the blocks under each row once, and releases them before it returns (it waits for
 * the stream): nothing is cached on the index, and nothing but the output grows with max_depth.  partition_mode 0, 1 and 2 all
 * run in probe order and return identical arrays.  The blocks (at most 2 n) must fit the index limit of ivj_index_build_dev. */
int ivj_depth_hist_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int32_t max_depth, int64_t* hist_dev);
int ivj_depth_hist_contigs_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_opts* opts, int32_t max_depth, int64_t* hist_dev);

/* pb.depth_quantiles / pb.median_depth: exact ORDER STATISTICS of the build side's depth over the positions of every probe row
 * (the median depth of a region, mosdepth --use-median, and its quartiles), with d(c, x), the conventions and Q of
 * ivj_depth_summary above.  For a probe row with L = |Q| >= 1 let v[0] <= v[1] <= ... <= v[L - 1] be the depths d(c, x) of its
 * positions, sorted; uncovered positions are in the list at depth 0.  With n_ranks in [1, IVJ_MAX_QUANT_RANKS] ranks per row:
 *   out[q][j] = v[ranks[q][j]]   for 0 <= ranks[q][j] < L;   -1 for any other rank, and for a probe that covers no position or
 *   lies outside the dictionary.
 * ranks (int64, 0-based) and out (int32) are ROW-major, probe->n rows of n_ranks.  The ranks of a row may come in any order and
 * repeat.  A quantile is the caller's arithmetic on ranks (q (L - 1), its floor and ceiling): the library answers ranks only.
 * Exact for any depth up to 2^31 - 1.  An empty build side, or one whose blocks come out empty, gives 0 for every rank inside
 * [0, L).  Identities: rank L - 1 gives max_depth of ivj_depth_summary; where no depth exceeds max_depth, out[q][j] is the first
 * bin of ivj_depth_hist's row q whose cumulative count exceeds ranks[q][j].  IVJ_EINVAL: n_ranks outside its range, ranks or out
 * NULL (whatever the row count).  No capacity protocol; no global atomics, integer adds only: bit-identical from run to run.
 * (New entries change no existing struct or signature: IVJ_ABI_VERSION stays.) */
#define IVJ_MAX_QUANT_RANKS 16
/* The kernel is a radix select over the depth blocks under each row, IVJ_QUANT_BITS bits per pass, with a
 * 2^IVJ_QUANT_BITS-bin histogram per (row, rank) in LDS; it gives a workgroup
 * P = floor(IVJ_QUANT_LDS_BYTES / (n_ranks * 2^IVJ_QUANT_BITS * 8)) consecutive probe rows, clamped to [1, IVJ_QUANT_MAX_TILE]
 * (informative: the result does not depend on them; IVJ_QUANT_BITS may be set when the library is compiled, 4 .. 8). */
#ifndef IVJ_QUANT_BITS
#define IVJ_QUANT_BITS 4
#endif
#define IVJ_QUANT_LDS_BYTES 65536
#define IVJ_QUANT_MAX_TILE 512
int ivj_depth_quantiles(ivj_ctx* ctx, const ivj_side* probe, const ivj_side* build, const ivj_opts* opts, int32_t n_ranks,
                        const int64_t* ranks /* n x n_ranks, row-major, 0-based */, int32_t* out /* n x n_ranks */);
/* The same on an index of ivj_index_build_dev (any form, as ivj_depth_hist_dev); probe columns, ranks and out in HBM.  Every call
 * derives the depth blocks, their index and 16-byte records (the steps of ivj_depth_hist_dev), walks the blocks under each tile
 * of rows once per pass, and releases them before it returns (it waits for the stream): nothing is cached on the index.
 * partition_mode 0, 1 and 2 all run in probe order and return identical arrays. */
int ivj_depth_quantiles_dev(ivj_ctx* ctx, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int32_t n_ranks,
                            const int64_t* ranks_dev, int32_t* out_dev);

/* ---- set operations on two frames, and their stats (pb.set_intersect / set_union / set_difference / set_symmetric_difference,
 * pb.jaccard) ------------------------------------------------------------------------------------------------------------------
 * U(F) = the (contig, position) pairs at least one row of F covers, under the conventions of ivj_depth: Strict rows cover
 * [start, end), Weak rows [start, end]; rows that cover nothing and rows outside the dictionary contribute nothing.  A set
 * operation returns the MAXIMAL runs of op(U(a), U(b)) as (contig, start, end) in (contig id, start) order, bounds in the mode's
 * own convention: two regions never touch or overlap (Strict [0,5) + [5,9) -> [0,9); Weak [1,5] + [6,9] -> [1,9]).  Both sides
 * share the contig dictionary opts->n_contigs; an empty side is legal; at most runs(a) + runs(b) <= a.n + b.n regions come back;
 * the result is bit-identical from run to run. */
enum {
    IVJ_SETOP_INTERSECTION = 0,          /* U(a) & U(b) */
    IVJ_SETOP_UNION = 1,                 /* U(a) | U(b) */
    IVJ_SETOP_DIFFERENCE = 2,            /* U(a) \ U(b) */
    IVJ_SETOP_SYMMETRIC_DIFFERENCE = 3   /* the positions in exactly one of the two */
};
typedef struct {
    int64_t n;
    int32_t* contig;
    int32_t* start;
    int32_t* end;
} ivj_regions;

/* Host path: library-owned buffers, released by ivj_regions_free. */
int ivj_setop(ivj_ctx* ctx, const ivj_side* a, const ivj_side* b, const ivj_opts* opts, int32_t op, ivj_regions* out);
void ivj_regions_free(ivj_regions* r);
/* bases[0..2] = the positions only U(a), only U(b), both cover (exact; intersection = bases[2], union = the sum of the three);
 * *n_intersections = the regions ivj_setop(IVJ_SETOP_INTERSECTION) would return.  One walk, no regions written. */
int ivj_set_stats(ivj_ctx* ctx, const ivj_side* a, const ivj_side* b, const ivj_opts* opts, int64_t bases[3], int64_t* n_intersections);
/* Device paths over two indexes of ivj_index_build_dev (any with_end_order: a missing end order is completed on demand, sweep-only
 * indexes are accepted; NULL = an empty side).  The capacity protocol of ivj_depth_dev: *n_regions always receives the total;
 * IVJ_ECAPACITY when it exceeds `capacity`, and nothing is written then.  bases / n_intersections are HOST pointers. */
int ivj_setop_dev(ivj_ctx* ctx, ivj_index* ix_a, ivj_index* ix_b, const ivj_opts* opts, int32_t op, int64_t capacity, int32_t* contig_dev,
                  int32_t* start_dev, int32_t* end_dev, int64_t* n_regions);
int ivj_set_stats_dev(ivj_ctx* ctx, ivj_index* ix_a, ivj_index* ix_b, const ivj_opts* opts, int64_t bases[3], int64_t* n_intersections);

/* ---- N frames as position sets (pb.multi_intersect, pb.consensus) ------------------------------------------------------------
 * F frames, 1 <= F <= IVJ_MAX_FRAMES, each read as its set U(F_f) under the conventions of the set operations above.
 * mask(c, x) = the frames that cover position x of contig c, bit f for frame f.  With k = min_frames in 1 .. F:
 *   IVJ_MULTI_SEGMENTS   the maximal runs of positions with ONE mask of at least k bits (bedtools multiinter): neighbouring
 *                        segments differ in mask unless a gap, a dropped segment or a contig boundary lies between them; segments
 *                        that pass the k filter are not merged with each other.  Where a row of frame 0 ends and a row of frame 1
 *                        starts is a segment boundary; two touching rows of one frame are not.
 *   IVJ_MULTI_CONSENSUS  the maximal runs of positions covered by at least k frames (runs that touch are one region): k = 1 is
 *                        the N-way union, k = F the N-way intersection.
 * (contig id, start) order, bounds in the mode's own convention, at most 2 x the summed union runs <= 2 x the summed rows regions;
 * bit-identical from run to run.  IVJ_EINVAL: n_frames outside 1 .. IVJ_MAX_FRAMES, min_frames outside 1 .. n_frames, an unknown
 * mode, an index over another dictionary than opts->n_contigs. */
#define IVJ_MAX_FRAMES 64
#define IVJ_MULTI_SEGMENTS 0
#define IVJ_MULTI_CONSENSUS 1
typedef struct {
    int64_t n;
    int32_t* contig;
    int32_t* start;
    int32_t* end;
    uint64_t* mask;      /* NULL for IVJ_MULTI_CONSENSUS */
} ivj_segments;

/* Host path: `frames` is an array of n_frames sides (an empty side is legal); library-owned buffers, released by ivj_segments_free. */
int ivj_multi_inter(ivj_ctx* ctx, const ivj_side* frames, int32_t n_frames, const ivj_opts* opts, int32_t min_frames, int32_t mode,
                    ivj_segments* out);
void ivj_segments_free(ivj_segments* s);
/* Device path over n_frames indexes of ivj_index_build_dev (any with_end_order: a missing end order is completed on demand, sweep-only
 * indexes are accepted; a NULL entry = an empty frame).  The capacity protocol of ivj_setop_dev: *n always receives the total;
 * IVJ_ECAPACITY when it exceeds `capacity`, and nothing is written then.  mask_dev (capacity x uint64) is written for
 * IVJ_MULTI_SEGMENTS only and may be NULL for IVJ_MULTI_CONSENSUS. */
int ivj_multi_inter_dev(ivj_ctx* ctx, ivj_index* const* ix, int32_t n_frames, const ivj_opts* opts, int32_t min_frames, int32_t mode,
                        int64_t capacity, int32_t* contig_dev, int32_t* start_dev, int32_t* end_dev, uint64_t* mask_dev, int64_t* n);

/* ---- N frames pair by pair (pb.pairwise_jaccard) ---------------------------------------------------------------------------------
 * The two F x F matrices every pairwise similarity of F frames is made of, from ONE walk over all frames (the segments of
 * IVJ_MULTI_SEGMENTS with min_frames = 1, reduced where they lie in HBM: csrc/pairwise.hip.h), F = n_frames in 1 .. IVJ_MAX_FRAMES:
 *   bases[i][j] = |U(F_i) & U(F_j)|              the positions both frames cover; bases[i][i] = |U(F_i)|
 *   runs[i][j]  = the maximal runs of U(F_i) & U(F_j): the regions ivj_setop(IVJ_SETOP_INTERSECTION) of the two frames would return
 *                 (the n_intersections of ivj_set_stats); runs[i][i] = the union runs of frame i
 * so that for a pair intersection = bases[i][j], union = bases[i][i] + bases[j][j] - bases[i][j], jaccard = their quotient.  Both are
 * n_frames * n_frames int64, ROW-MAJOR, full symmetric matrices; exact (a Weak frame [INT32_MIN, INT32_MAX] counts 2^32 positions
 * per contig; runs <= 2^31); the rows and columns of empty frames, and everything when all frames are empty, are 0.  Conventions
 * and limits of the frames are those of ivj_multi_inter.  Integer sums in a fixed order, no global atomics: bit-identical from run
 * to run.  IVJ_EINVAL: n_frames outside 1 .. IVJ_MAX_FRAMES, a NULL frame array or output, an index over another dictionary than
 * opts->n_contigs.  (New entries change no existing struct or signature: IVJ_ABI_VERSION stays.) */
/* Host path: `frames` is an array of n_frames sides (an empty side is legal); bases / runs are CALLER-owned host buffers. */
int ivj_multi_pairwise(ivj_ctx* ctx, const ivj_side* frames, int32_t n_frames, const ivj_opts* opts, int64_t* bases, int64_t* runs);
/* Device path over n_frames indexes of ivj_index_build_dev (any with_end_order: a missing end order is completed on demand, sweep-only
 * indexes are accepted; a NULL entry = an empty frame); bases_dev / runs_dev are n_frames * n_frames int64 in HBM.  Waits for the
 * stream before it returns (the segment list is released). */
int ivj_multi_pairwise_dev(ivj_ctx* ctx, ivj_index* const* ix, int32_t n_frames, const ivj_opts* opts, int64_t* bases_dev, int64_t* runs_dev);

/* ---- group ids: joins keyed on extra columns (on_cols) --------------------------------------------------------------------------
 * Every kernel partitions by one int32 id per row and ignores ids outside [0, n_contigs).  A dense GROUP id over (chrom, on_col
 * values...) passed as `contig`, with n_contigs = the number of groups, makes every operation of this header run within groups.
 * Input per side: the chrom id column plus n_cols (<= 8) int32 code columns, one per on_col, from dictionaries shared by the two
 * sides (codes of column j in [0, cards[j]); a negative code is a null).  key = ((chrom * cards[0] + code_0) * cards[1] + code_1) ...
 * in [0, D), D = n_contigs * prod(cards); D > 2^31 is refused with IVJ_EINVAL (the message names the cardinalities).
 * Numbering rule: gid = rank of the row's key among the keys present in the BUILD side, in ascending key order; -1 for a row with a
 * null / out-of-range component or a key the build side lacks.  *n_groups = G, the number of present keys.  group_keys (optional,
 * NULL: not written): row g = (chrom, code_0, ..., code_{n_cols-1}) of gid g, G x (1 + n_cols) int32 row-major; keys_cap rows are
 * available, IVJ_ECAPACITY (with *n_groups set, the gids complete) when G exceeds it -- min(n_build, D) rows always suffice.
 * With dictionaries sorted the way the caller sorts chrom, gids ascend in (chrom, on values) order.
 * A gid column may alias its side's contig column.  For merge / cluster of one frame pass it as the build side (n_probe = 0). */
/* device pointers for the columns; probe_codes / build_codes are HOST arrays of n_cols device pointers, cards a host array.
 * Passes: mark (one bit per build key; the bitmap privatized in LDS up to 2^18 keys, else a test before the global atomic OR),
 * rank (popcount + exclusive scan of the D / 32 words), remap of both sides, group table.  Blocks until *n_groups is known.
 * Scratch: 12 bytes per 32 keys of D from the context's arena. */
int ivj_group_ids_dev(ivj_ctx* ctx, const int32_t* probe_contig, const int32_t* const* probe_codes, int64_t n_probe,
                      const int32_t* build_contig, const int32_t* const* build_codes, int64_t n_build, int32_t n_cols, const int32_t* cards,
                      int32_t n_contigs, int32_t* probe_gid, int32_t* build_gid, int32_t* group_keys, int64_t keys_cap, int32_t* n_groups);

/* Arrow C Data Interface IMPORT of one side (zero copy): `array` / `schema` describe a struct array (or record
 * batch) whose children named contig / start / end (any order, other children ignored) are int32 without nulls --
 * what the reference hands its executor as an ArrowArrayStream batch after the chrom column has been dictionary
 * encoded (src/lib.rs:89-100 collects the stream; range_op_io.py:398-418 builds it).  Fills *out with pointers INTO
 * the Arrow buffers (offset applied); nothing is copied and nothing is released: the caller keeps the ArrowArray
 * alive for as long as *out is used.  Needs no device. */
int ivj_side_from_arrow(const void* array, const void* schema, ivj_side* out);

/* ---- streaming probe side ----------------------------------------------------- *
 * The reference streams df1 through its executor as an Arrow C stream and yields result batches lazily            *
 * (polars_bio/range_op_io.py:100-174, src/lib.rs:154-214, fan-out with back-pressure src/scan.rs:294-357).         *
 * Here the build side (df2) is indexed once and stays in HBM; the probe side is SUBMITTED batch by batch (e.g. the *
 * record batches of an ArrowArrayStream, columns viewed with ivj_side_from_arrow).  Every submit overlaps the H2D   *
 * copy of the batch it was given (pinned staging slot, copy stream), the join of the batch before it (compute       *
 * stream) and the D2H copy of the batch before that (pinned result slot, copy-back stream), and hands out the        *
 * results of the batch submitted two calls earlier.  ivj_stream_flush drains what is left.                            */
#define IVJ_STREAM_OVERLAP  0   /* pairs (probe row of the batch, build row)                  */
#define IVJ_STREAM_COUNT    1   /* count_overlaps: int64 count per probe row of the batch      */
#define IVJ_STREAM_NEAREST  2   /* nearest: opts->nearest_k build rows, distances, n_found     */

typedef struct ivj_stream ivj_stream;

/* Results of ONE earlier batch; the buffers are pinned host memory owned by the stream, valid until the next call
 * on the stream.  batch = -1: nothing was ready. */
typedef struct {
    int64_t batch;          /* 0-based index of the submitted batch these results belong to, -1 = none      */
    int64_t n_probe;        /* probe rows of that batch                                                     */
    int64_t n;              /* overlap: pairs; count / nearest: n_probe                                     */
    int32_t* probe_idx;     /* overlap: probe row INSIDE the batch                                          */
    int32_t* build_idx;     /* overlap: build row; nearest: n_probe * k build rows (-1 = no candidate)      */
    int64_t* counts;        /* count_overlaps                                                               */
    int64_t* dist;          /* nearest: n_probe * k distances                                               */
    int32_t* n_found;       /* nearest: filled slots per probe row                                          */
} ivj_stream_result;

/* build: host columns (borrowed for the call).  max_batch_rows bounds the probe batches (pinned staging is sized by it). */
int ivj_stream_open(ivj_ctx* ctx, const ivj_side* build, const ivj_opts* opts, int op, int64_t max_batch_rows, ivj_stream** out);
/* batch: host columns of the next probe batch (borrowed for the call; copied into the pinned staging slot). */
int ivj_stream_submit(ivj_stream* st, const ivj_side* batch, ivj_stream_result* done);
/* no more input: call until done->batch == -1 */
int ivj_stream_flush(ivj_stream* st, ivj_stream_result* done);
/* IVJ_STREAM_NEAREST sessions: the direction mask (ivj_opts.nearest_ignore) of the batches submitted AFTER this call; a batch keeps
 * the mask it was submitted under, whenever its join runs.  A host whose probe rows differ in orientation submits the two
 * orientations of a batch as two batches to ONE session -- one copy of the build index in HBM -- with this call in between.
 * IVJ_EINVAL for a mask outside 0 .. 3 or a session of another operation. */
int ivj_stream_set_nearest_ignore(ivj_stream* st, int32_t mask);
void ivj_stream_close(ivj_stream* st);

/* ---- multi-GPU: one rank per GPU, contig sharding, all-gatherv of the result batches over RCCL (xGMI) ---------------- *
 * Replaces the reference's only parallelism -- DataFusion target_partitions over probe rows (src/scan.rs:233-277,
 * polars_bio/context.py:36) -- for a host that drives several GPUs: intervals on different contigs never interact
 * (the reference builds one tree per contig, range_op.py:550), so every rank joins the rows of ITS contigs (global row
 * ids in ivj_side.row_id) with no collective on the data path, and the variable-length results are exchanged with one
 * ncclAllGather of the counts + ONE grouped batch of ncclSend / ncclRecv (every GPU pair on its own xGMI link).
 * RCCL is loaded on first use (librccl.so.1); nothing here needs PyTorch.  A communicator of world 1 never touches RCCL --
 * unless IVJ_COMM_NO_SHORTCUT=1 is set when it is created (round 6; tests): it is then a REAL communicator (ncclGetUniqueId +
 * ncclCommInitRank), its count all-gather an ncclAllGather and its own slice travels through a grouped ncclSend + ncclRecv to
 * itself, so that the RCCL branch of every call below runs on a 1-GPU box (tests/test_comm.py::test_real_rccl_on_one_rank_*). */
typedef struct ivj_comm ivj_comm;
#define IVJ_UNIQUE_ID_BYTES 128
/* rank 0 makes the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks by any channel the host has */
int ivj_comm_unique_id(void* id_out);
/* one process per GPU: ncclCommInitRank on the context's device (collective: every rank calls it) */
int ivj_comm_create(ivj_ctx* ctx, const void* unique_id, int rank, int world, ivj_comm** out);
/* one process, one context per device: ncclCommInitAll; out[i] = communicator of ctxs[i] (rank i).  Calls on the n
 * communicators that belong together (ivj_allgather_counts, ivj_allgatherv_dev, ivj_overlap_allgather_dev) must then
 * come from n host threads, one per rank.  Contexts that SHARE a device (RCCL wants one device per rank), or
 * IVJ_COMM_LOOPBACK=1, get the library's in-process transport instead of RCCL: a host-memory rendezvous + device copies
 * issued by the receiving rank, same calls, same order, same blocking behaviour (a rank that never arrives makes its
 * peers fail with IVJ_EHIP after IVJ_COMM_LOOPBACK_TIMEOUT seconds, default 120, instead of waiting forever) -- a 1-GPU
 * box runs the multi-rank protocol with it. */
int ivj_comm_create_local(ivj_ctx* const* ctxs, int n, ivj_comm** out);
void ivj_comm_destroy(ivj_comm* comm);
int ivj_comm_info(const ivj_comm* comm, int* rank, int* world);
/* counts[r] = n_local of rank r, on every rank (host array of `world` entries) */
int ivj_allgather_counts(ivj_comm* comm, int64_t n_local, int64_t* counts);
/* all-gatherv of n_cols device columns of elem_bytes-wide elements: recv_cols[k] (capacity = sum of counts) receives
 * the concatenation over ranks, in rank order, of every rank's send_cols[k][0 .. counts[rank]).  Ordered after the work
 * queued on the context's stream; returns when the exchange is complete. */
int ivj_allgatherv_dev(ivj_comm* comm, const void* const* send_cols, void* const* recv_cols, int n_cols, int elem_bytes,
                       const int64_t* counts);
/* pb.overlap of this rank's shard + the all-gatherv of the pairs, with the exchange OVERLAPPING the join: the rank's
 * probe rows are cut into n_chunks contiguous chunks (the same number on every rank, 1 .. 64); while chunk i is joined
 * (fused single pass) a helper thread exchanges chunk i - 1 straight into the caller's columns.  Every rank ends up with
 * all *n_total pairs (layout: chunk after chunk, inside a chunk rank after rank; the pairs of one probe row contiguous);
 * *n_local = this rank's share.
 * Failure contract (no rank is left waiting in a collective, whatever happens on another one):
 *   - every rank takes part in the count all-gather of EVERY chunk.  A rank whose own work fails (join, allocation) marks
 *     the failed chunk and all later ones as failed instead of joining them and returns its own error code after the last
 *     chunk; every other rank completes its chunks and returns IVJ_EPEER (the failed rank's pairs from that chunk on are
 *     missing from the columns, *n_total counts what was exchanged);
 *   - IVJ_ECAPACITY on EVERY rank when the pairs outgrow the capacity of ANY rank: the decision is taken from the gathered
 *     counts, so all ranks stop moving pairs at the same chunk (nothing is written past a capacity), the remaining chunks
 *     are still joined and counted, and *n_total = the capacity the call needs -- one regrow step is enough;
 *   - an error of the collective itself (RCCL, the exchange stream) is returned as IVJ_EHIP; nothing can be promised to
 *     the peers then.
 * IVJ_FAULT_ALLGATHER="<rank>:<chunk>" in the environment makes that chunk's join on that rank fail (test knob). */
int ivj_overlap_allgather_dev(ivj_comm* comm, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int n_chunks,
                              int32_t* probe_idx_dev, int32_t* build_idx_dev, int64_t capacity, int64_t* n_total, int64_t* n_local);

/* pb.count_overlaps / pb.nearest of this rank's shard + the exchange of the PER-PROBE results ("the gather is
 * of fixed-width per-probe results scattered back to original probe order (carry probe row id)"; replaces the single-process
 * providers behind src/operation.rs:331-340 and :146-158 for a multi-GPU host).  probe_dev->row_id = the GLOBAL probe rows of the
 * shard (required when world > 1; NULL at world 1 means 0 .. n-1), n_total = probe rows of the whole job (the same on every rank).
 * Every rank ends up with the full-length columns in global probe order: counts_dev[n_total] (int64), or idx_dev[n_total * k] /
 * dist_dev[n_total * k] / n_found_dev[n_total] with k = opts->nearest_k.  Rows no rank reports keep count 0 / build row -1, distance -1,
 * n_found 0.  On the wire: {row int32, count int32} (8 bytes per probe; counts are bounded by the build rows) and
 * {row int32, k x int32, k x int64, int32}: ONE count all-gather + ONE grouped send / receive batch.  The row column on the wire IS
 * probe_dev->row_id and the count column comes straight out of the shard's kernel (no pack pass); this rank's own slice is read where
 * it lies.  Receiver (round 6): a shard whose global rows ASCEND -- what ivj_host_shard and every host that keeps df1's order produce --
 * is MERGED: the rows of an output tile are one contiguous segment of every sender's columns (bound search per (sender, tile)), read
 * coalesced, placed by row in LDS, written coalesced with the defaults filled in (config 5 through this call on one rank: 10.6 -> 2.8 ms).
 * Senders in any other order are detected by the merge's own checks (every placed row belongs to its tile, the placed rows are counted)
 * and take the round-5 form -- defaults, then one store per reported row.  A row id reported twice is IVJ_EINVAL (merge form; the
 * scatter form keeps the later store), a row id outside [0, n_total) IVJ_EINVAL in both.
 * Failure contract: every rank reaches the count all-gather whatever happened to its own shard; a rank whose work failed returns its
 * own error, every other rank IVJ_EPEER, and nothing is sent or received (decided from the gathered values, so nobody waits in a
 * collective); ranks that disagree on n_total, or report more rows than n_total, get IVJ_EINVAL on every rank.
 * IVJ_FAULT_ALLGATHER="<rank>:0" makes that rank's shard fail (test knob). */
int ivj_count_overlaps_allgather_dev(ivj_comm* comm, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int64_t n_total,
                                     int64_t* counts_dev);
int ivj_nearest_allgather_dev(ivj_comm* comm, ivj_index* ix, const ivj_side* probe_dev, const ivj_opts* opts, int64_t n_total,
                              int32_t* idx_dev, int64_t* dist_dev, int32_t* n_found_dev);

/* ---- the one-call Arrow entry: two ArrowArrayStreams in, a stream of joined record batches out -------------------------- *
 * This is the shape of the reference's own FFI: range_operation_frame / range_operation_lazy take df1 and df2 as Arrow C
 * streams with a STRING chrom and start / end of any integer width and answer with a lazy frame of joined rows
 * (/root/reference/src/lib.rs:79-145, 154-214; the renaming SELECT over the joined batches: src/operation.rs:272-301,
 * 170-197).  A host binds ONE call per operation and re-implements nothing: both streams are drained (and released), chrom
 * (utf8 / large_utf8 / a dictionary of those, per batch) is encoded with one dictionary over both sides, start / end
 * (int8 .. int64, signed or unsigned) are narrowed to int32 with the reference's range check
 * (docs/features/operations.md:36-37; nulls in a coordinate column and values beyond int32 are IVJ_EINVAL with the column's
 * name), the join runs on the device through the host entry points above, and `out_stream` -- a caller-allocated
 * `struct ArrowArrayStream` (https://arrow.apache.org/docs/format/CStreamInterface.html) -- yields the result in batches of
 * batch_rows rows (<= 0: 1 Mi) that are assembled WHEN PULLED: every column of df1 named <name><suffix1>, then every
 * column of df2 named <name><suffix2>, gathered by the pair indices (fixed-width primitives of 1 .. 32 bytes, bool,
 * utf8 / large_utf8 / binary / large_binary; dictionary-encoded columns are delivered decoded to their value type; any
 * other column type is refused by name).  cols1 / cols2: {chrom, start, end} column names, NULL = those defaults.
 * opts->n_contigs is ignored (the dictionary is made inside).  limit >= 0 bounds the result rows (src/lib.rs:80-88, 125-130).
 * The stream pointers are `struct ArrowArrayStream*` (void* here so that this header needs no Arrow declarations). */
int ivj_overlap_arrow_stream(ivj_ctx* ctx, void* df1_stream, void* df2_stream, const char* const* cols1, const char* const* cols2,
                             const ivj_opts* opts, const char* suffix1 /* NULL: "_1" */, const char* suffix2 /* NULL: "_2" */,
                             int64_t batch_rows, int64_t limit, void* out_stream);
/* df1 columns (<name><suffix1>, NULL: no suffix) + count: int64, df1 row order (range_op.py:418-511, src/operation.rs:306-350) */
int ivj_count_overlaps_arrow_stream(ivj_ctx* ctx, void* df1_stream, void* df2_stream, const char* const* cols1, const char* const* cols2,
                                    const ivj_opts* opts, const char* suffix1, int64_t batch_rows, int64_t limit, void* out_stream);
/* per df1 row its opts->nearest_k nearest df2 rows (one result row each; a df1 row without any keeps one row with null df2
 * columns), + distance: int64 when with_distance (src/operation.rs:100-200).  opts->nearest_ignore applies to every df1 row alike (here
 * and in the lazy form): the one-call entries take the uniform mask only; a per-row orientation column is the host's to split on. */
int ivj_nearest_arrow_stream(ivj_ctx* ctx, void* df1_stream, void* df2_stream, const char* const* cols1, const char* const* cols2,
                             const ivj_opts* opts, const char* suffix1, const char* suffix2, int32_t with_distance, int64_t batch_rows,
                             int64_t limit, void* out_stream);

/* The LAZY forms (round 5) -- /root/reference/src/lib.rs:154-214 range_operation_lazy, src/scan.rs:294-357, polars_bio/range_op_io.py:100-174:
 * df2 (the build side) is drained, encoded and indexed once; df1 stays a STREAM and is pulled batch by batch from inside the result
 * stream's get_next: a batch is encoded with the session's chrom dictionary, narrowed to int32, submitted to a streaming probe session
 * (ivj_stream_*: its H2D copy overlaps the join of the batch before it and the D2H copy of the batch before that), and the results that
 * come back -- those of the batch submitted two turns earlier -- are assembled into record batches of batch_rows rows.  df1 batches
 * above max_batch_rows (<= 0: 4 Mi; it sizes the session's pinned staging) are submitted in slices; batches BELOW min(max_batch_rows,
 * 2 Mi) rows are coalesced: the library pulls until it holds that many rows (or df1 ends) and treats the group as one batch (a group
 * never exceeds twice that size unless a single batch does).  Host memory: df2 + three such groups + one group's result, whatever the
 * length of df1 (which may pass 2^31 rows).  Result rows come in df1 order.  limit >= 0: df1 is pulled ONE batch at a time (no
 * coalescing: the call may need very little of it) and not at all after the limit is reached.  Errors of a later batch (a coordinate beyond int32, a malformed batch) surface from
 * get_next (errno, text from get_last_error) -- as the reference's surface at collect time.  OWNERSHIP (both forms, eager and lazy): the
 * two input streams are consumed by the call whatever its outcome -- on every error path their release callbacks have run (the lazy
 * form keeps df1 until the result stream is exhausted or released).  The result stream works on `ctx` whenever it is pulled: pull it
 * from one thread at a time and not concurrently with other calls on the same context; release it before the context. */
int ivj_overlap_arrow_stream_lazy(ivj_ctx* ctx, void* df1_stream, void* df2_stream, const char* const* cols1, const char* const* cols2,
                                  const ivj_opts* opts, const char* suffix1, const char* suffix2, int64_t batch_rows, int64_t max_batch_rows,
                                  int64_t limit, void* out_stream);
int ivj_count_overlaps_arrow_stream_lazy(ivj_ctx* ctx, void* df1_stream, void* df2_stream, const char* const* cols1, const char* const* cols2,
                                         const ivj_opts* opts, const char* suffix1, int64_t batch_rows, int64_t max_batch_rows, int64_t limit,
                                         void* out_stream);
int ivj_nearest_arrow_stream_lazy(ivj_ctx* ctx, void* df1_stream, void* df2_stream, const char* const* cols1, const char* const* cols2,
                                  const ivj_opts* opts, const char* suffix1, const char* suffix2, int32_t with_distance, int64_t batch_rows,
                                  int64_t max_batch_rows, int64_t limit, void* out_stream);

/* The two host halves of that call on their own (no device, no context): */
/* ... the key columns the join sees: both streams drained (and released), chrom encoded, coordinates narrowed */
typedef struct {
    int64_t n1, n2;
    int32_t *contig1, *start1, *end1;      /* n1 values each */
    int32_t *contig2, *start2, *end2;      /* n2 values each */
    int32_t n_contigs;
    int64_t* name_offsets;                 /* n_contigs + 1: name v of the shared dictionary = name_bytes[name_offsets[v] .. name_offsets[v + 1]) */
    char* name_bytes;
} ivj_arrow_keys;
int ivj_arrow_encode_keys(void* df1_stream, void* df2_stream, const char* const* cols1, const char* const* cols2, ivj_arrow_keys* out);
void ivj_arrow_keys_free(ivj_arrow_keys* keys);
/* ... the row assembly: rows idx[0 .. n) (negative or out of range: a null row) of the drained stream as a new stream */
int ivj_arrow_take_stream(void* in_stream, const int64_t* idx, int64_t n, int64_t batch_rows, void* out_stream);


/* ---- device memory helpers for callers without a HIP binding ------------ */
int ivj_dev_alloc(ivj_ctx* ctx, int64_t bytes, void** out);
int ivj_dev_free(ivj_ctx* ctx, void* p);
int ivj_memcpy_h2d(ivj_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes);
int ivj_memcpy_d2h(ivj_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes);

/* ---- host-side helpers of the front door (no device work, no context; plain std::thread workers; threads <= 0: 32) ----------
 * What the reference's executor does around the join in Rust -- the dictionary handling of the chrom key and the column gathers
 * of the renaming SELECT (src/operation.rs:272-301), the int32 coordinate limit (docs/features/operations.md:36-37) -- as ONE
 * pass over the rows each; the Python front door (polars_bio_amd/_arrow.py) calls them on the buffers of its Arrow columns. */

/* Coordinate column of src_bytes-wide (1, 2, 4, 8) signed / unsigned integers -> int32, with the column's minimum and maximum
 * (the caller refuses a column that leaves the int32 range; unsigned values beyond INT64_MAX are reported as INT64_MAX). */
int ivj_host_narrow_i32(const void* src, int32_t src_bytes, int32_t is_unsigned, int64_t n, int32_t* dst, int64_t* out_min, int64_t* out_max,
                        int32_t threads);

/* Arrow string / large_string column (n + 1 offsets of offset_bytes = 4 / 8, the value bytes, optional validity bitmap read from
 * bit validity_bit0) -> ids[n] (dictionary ids in first-occurrence order, -1 for a null) and dict_rows[*n_values] (one row that
 * holds each value).  IVJ_ECAPACITY: more than dict_cap (or 4096) distinct values -- the caller falls back to its own encoder. */
int ivj_host_encode_utf8(const void* offsets, int32_t offset_bytes, const uint8_t* data, const uint8_t* validity, int64_t validity_bit0, int64_t n,
                         int32_t* ids, int64_t* dict_rows, int32_t dict_cap, int32_t* n_values, int32_t threads);

/* Column of 64-bit keys -> ids[n] in first-occurrence order and dict_rows[*n_values] (one row that holds each key).  The front
 * door runs it over the object POINTERS of a pandas object-dtype column: rows that share a string object (the CSV parser interns
 * them per column) get one dictionary entry without the string being looked at, and only the few distinct objects are converted.
 * IVJ_ECAPACITY: more than dict_cap (or 4096) distinct keys -- the caller falls back to the ordinary conversion. */
int ivj_host_encode_keys64(const uint64_t* keys, int64_t n, int32_t* ids, int64_t* dict_rows, int32_t dict_cap, int32_t* n_values, int32_t threads);

/* Dictionary indices (idx_bytes = 1, 2, 4, 8, signed; negative = null) -> out[i] = remap[idx[i]] (-1 for a null), and seen[v] = 1
 * for every dictionary entry some row refers to (seen: remap_len bytes, OR-ed into). */
int ivj_host_remap_i32(const void* idx, int32_t idx_bytes, int64_t n, const int32_t* remap, int64_t remap_len, int32_t* out, uint8_t* seen,
                       int32_t threads);

/* dst[i] = src[idx[i]] for 4- or 8-byte values (0 for a negative index): the non-key columns of the joined rows. */
int ivj_host_take(const void* src, int32_t elem_bytes, int64_t n_src, const int32_t* idx, int64_t n, void* dst, int32_t threads);

/* dst[idx[i]] = src[i] for rows of row_bytes bytes: the mirror of ivj_host_take -- a shard's per-probe results (counts, nearest rows and
 * distances) back to their GLOBAL probe rows when one process drives several devices (threaded; the indices of one call are distinct;
 * an index outside [0, n_dst) is refused before anything is written).  remap (rows of int32 values only, NULL: none): the value stored is
 * remap[src value] for a value in [0, remap_len) and -1 otherwise -- a shard's local build rows become global rows on the way. */
int ivj_host_scatter(const void* src, int32_t row_bytes, int64_t n, const int32_t* idx, int64_t n_dst, void* dst, const int32_t* remap, int64_t remap_len,
                     int32_t threads);

/* Contig sharding of one side for `world` ranks ("host buckets both sides by contig id"; the reference's
 * partitioner cuts by row count, src/scan.rs:233-277): owner[c] = rank of contig c (n_contigs entries), a row whose contig lies
 * outside [0, n_contigs) belongs to no rank.  One counting pass fills counts[world]; with output columns (arrays of `world`
 * pointers, each sized from a first counts-only call with all four NULL; any of the four may be NULL) one placing pass writes
 * every rank's rows -- contig / start / end and the GLOBAL row (what ivj_side.row_id carries) -- in input order. */
int ivj_host_shard(const int32_t* contig, const int32_t* start, const int32_t* end, int64_t n, const int32_t* owner, int32_t n_contigs, int32_t world,
                   int64_t* counts, int32_t* const* out_contig, int32_t* const* out_start, int32_t* const* out_end, int32_t* const* out_row, int32_t threads);
/* rows per contig (the weights of the LPT contig -> rank assignment): hist[n_contigs] */
int ivj_host_contig_hist(const int32_t* contig, int64_t n, int32_t n_contigs, int64_t* hist, int32_t threads);
/* ivj_group_ids_dev on host columns (threaded; no device, no context): the same numbering rule, bit for bit.  The front door
 * composes group ids here, where the chrom ids already are: no extra bytes cross to the device. */
int ivj_host_group_ids(const int32_t* probe_contig, const int32_t* const* probe_codes, int64_t n_probe, const int32_t* build_contig,
                       const int32_t* const* build_codes, int64_t n_build, int32_t n_cols, const int32_t* cards, int32_t n_contigs,
                       int32_t* probe_gid, int32_t* build_gid, int32_t* group_keys, int64_t keys_cap, int32_t* n_groups, int32_t threads);

/* int32 -> int64: key columns materialised in HBM back to the dtype of the caller's frame. */
int ivj_host_widen_i32(const int32_t* src, int64_t n, int64_t* dst, int32_t threads);

#ifdef __cplusplus
}
#endif
#endif /* IVJOIN_H */
