"""The frame every host-buffer entry shares (argument checks -> early-out on empty -> upload -> index -> result -> copy-out),
pinned from outside: which message a refused call reports (and so the order of the checks), what a refused call leaves in its
result struct, and the results at the edges of the frame (an empty side, one row, a result without rows) against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from polars_bio_amd import _engine as E
from _util import OracleEngine, random_side
import _depth_hist_util as DH
import _depth_profile_util as DP
import _depth_quant_util as DQ
import _depth_sum_util as DSU
import _depth_summary_util as DSM
import _depth_util as DU
import _merge_agg_util as MA
import _multi_util as MU
import _overlap_agg_util as OA
import _pairwise_util as PW
import _permutation_util as PM
import _signal_util as SG
import _thresholds_util as T
import _window_util as WU

pytestmark = pytest.mark.gpu

EINVAL = -1
NC = 3


@pytest.fixture(scope="module")
def eng():
    if E.device_count() < 1:
        pytest.skip("no HIP device")
    e = E.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------------------------- refusals

def _side(n=1, null_column=False):
    a = np.zeros(max(n, 1), np.int32)
    s = E._Side(None if null_column else a.ctypes.data, a.ctypes.data, a.ctypes.data, n, None)
    s._keep = a
    return s


def _opts(bad=False):
    o = E.make_opts(True, NC)
    if bad:
        o.filter_op = 7
    return o


BAD_OPTS = "filter_op must be 0 (Weak) or 1 (Strict)"
_buf = np.zeros(64, np.int64)
BUF = _buf.ctypes.data
THR = E.make_thresholds(1)
NO_THR = E._Thresholds(0, None, None)
WIN = E.make_window(5, 5)
R = C.byref


def _out_struct(kind):
    """A result struct with rubbish in it: a refused call has to leave it empty."""
    out = kind()
    for name, ctype in kind._fields_:
        setattr(out, name, 7 if ctype is C.c_int64 else C.cast(BUF, ctype))
    return out


def _is_empty(out):
    return all((getattr(out, name) == 0) if ctype is C.c_int64 else not getattr(out, name) for name, ctype in out._fields_)


# name -> (side names, call(L, h, a, b, o, res) with res = the result pointer / struct reference or None,
#          result struct or None, message of a NULL result given non-empty sides)
TWO_SIDED = {
    "ivj_overlap": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_overlap(h, a, b, o, res), E._Pairs, "ctx or out is NULL"),
    "ivj_overlap_thresh": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_overlap_thresh(h, a, b, o, R(THR), res), E._Pairs,
                           "ctx or out is NULL"),
    "ivj_overlap_window": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_overlap_window(h, a, b, o, R(WIN), res, None), E._Pairs,
                           "ctx or out is NULL"),
    "ivj_overlap_outer": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_overlap_outer(h, a, b, o, None, res), E._Pairs,
                          "ctx or out is NULL"),
    "ivj_overlap_select": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_overlap_select(h, a, b, o, None, 0, res), E._RowSel,
                           "ctx or out is NULL"),
    "ivj_subtract": (("left", "right"), lambda L, h, a, b, o, res: L.ivj_subtract(h, a, b, o, res), E._Pieces, "ctx or out is NULL"),
    "ivj_setop": (("a", "b"), lambda L, h, a, b, o, res: L.ivj_setop(h, a, b, o, 0, res), E._Regions, "ctx or out is NULL"),
    "ivj_coverage": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_coverage(h, a, b, o, res), None, "coverage is NULL"),
    "ivj_overlap_bases": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_overlap_bases(h, a, b, o, res), None, "bases is NULL"),
    "ivj_count_overlaps": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_count_overlaps(h, a, b, o, res), None, "counts is NULL"),
    "ivj_count_overlaps_thresh": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_count_overlaps_thresh(h, a, b, o, R(THR), res), None,
                                  "counts is NULL"),
    "ivj_count_window": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_count_window(h, a, b, o, R(WIN), res), None, "counts is NULL"),
    "ivj_nearest": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_nearest(h, a, b, o, res, res, res), None,
                    "nearest output buffers are NULL"),
    "ivj_depth_hist": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_depth_hist(h, a, b, o, 4, res), None, "hist is NULL"),
    "ivj_depth_quantiles": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_depth_quantiles(h, a, b, o, 1, BUF, res), None, "out is NULL"),
    "ivj_depth_summary": (("probe", "build"), lambda L, h, a, b, o, res: L.ivj_depth_summary(h, a, b, o, None, 0, res, None), None,
                          "max_depth and bases_ge are both NULL"),
    "ivj_depth_profile": (("windows", "build"), lambda L, h, a, b, o, res: L.ivj_depth_profile(h, a, None, 4, b, o, res), None, "bases is NULL"),
}


def _refused(eng, rc, message):
    assert rc == EINVAL
    assert eng.L.ivj_last_error().decode() == message


@pytest.mark.parametrize("name", sorted(TWO_SIDED))
def test_two_sided_refusals(eng, name):
    (na, nb), call, kind, null_message = TWO_SIDED[name]
    L, h = eng.L, eng.h

    def run(a, b, o, null_result=False):
        out = _out_struct(kind) if kind else None
        res = None if null_result else (R(out) if kind else BUF)
        rc = call(L, h, R(a) if a is not None else None, R(b) if b is not None else None, R(o) if o is not None else None, res)
        return rc, out

    good = _side(1)
    cases = [
        # one bad argument
        ((good, good, None), "opts is NULL"),
        ((good, good, _opts(bad=True)), BAD_OPTS),
        ((None, good, _opts()), f"{na} is NULL"),
        ((_side(-1), good, _opts()), f"{na}.n < 0"),
        ((good, _side(-1), _opts()), f"{nb}.n < 0"),
        ((_side(2, null_column=True), good, _opts()), f"{na} has a NULL column"),
        ((good, _side(2, null_column=True), _opts()), f"{nb} has a NULL column"),
        # two bad arguments: the options are looked at first, then the first side, then the second
        ((_side(-1), good, _opts(bad=True)), BAD_OPTS),
        ((_side(-1), _side(2, null_column=True), _opts()), f"{na}.n < 0"),
        ((good, None, None), "opts is NULL"),
    ]
    for args, message in cases:
        rc, out = run(*args)
        _refused(eng, rc, message)
        if out is not None:
            assert _is_empty(out), (name, message)
    # a NULL result: a struct is refused before anything else is read, a buffer after the sides and only with rows to report
    rc, _ = run(good, _side(-1), _opts(), null_result=True)
    _refused(eng, rc, null_message if kind else f"{nb}.n < 0")
    rc, _ = run(good, good, _opts(bad=True), null_result=True)
    _refused(eng, rc, null_message if kind else BAD_OPTS)
    rc, _ = run(good, good, _opts(), null_result=True)
    _refused(eng, rc, null_message)
    if kind is None and name not in ("ivj_depth_hist", "ivj_depth_quantiles", "ivj_depth_summary"):
        rc, _ = run(_side(0), good, _opts(), null_result=True)           # no rows: the buffer is never looked at
        assert rc == 0


def test_per_entry_refusals(eng):
    L, h = eng.L, eng.h
    g, o, bad_o = _side(1), _opts(), _opts(bad=True)
    neg = _side(-1)
    pairs = _out_struct(E._Pairs)
    # thresholds / window / mode come after the sides
    _refused(eng, L.ivj_overlap_thresh(h, R(g), R(g), R(o), R(NO_THR), R(pairs)),
             "no threshold is set (min_overlap 0, probe_min and build_min NULL): use the plain entry points")
    assert _is_empty(pairs)
    _refused(eng, L.ivj_overlap_thresh(h, R(g), R(neg), R(o), R(NO_THR), R(pairs)), "build.n < 0")
    _refused(eng, L.ivj_overlap_thresh(h, R(g), R(g), R(o), None, R(pairs)), "thresholds is NULL")
    _refused(eng, L.ivj_count_overlaps_thresh(h, R(g), R(g), R(o), None, None), "thresholds is NULL")
    _refused(eng, L.ivj_count_overlaps_thresh(h, R(neg), R(g), R(o), None, None), "probe.n < 0")
    pairs = _out_struct(E._Pairs)
    _refused(eng, L.ivj_overlap_window(h, R(g), R(g), R(o), None, R(pairs), None), "window is NULL")
    assert _is_empty(pairs)
    _refused(eng, L.ivj_overlap_window(h, R(g), R(g), R(bad_o), None, R(pairs), None), BAD_OPTS)
    _refused(eng, L.ivj_count_window(h, R(g), R(g), R(o), None, None), "window is NULL")
    _refused(eng, L.ivj_count_window(h, R(g), R(neg), R(o), None, BUF), "build.n < 0")
    rows = _out_struct(E._RowSel)
    _refused(eng, L.ivj_overlap_select(h, R(g), R(g), R(o), None, 2, R(rows)), "mode must be IVJ_SELECT_SEMI (0) or IVJ_SELECT_ANTI (1)")
    assert _is_empty(rows)
    _refused(eng, L.ivj_overlap_select(h, R(g), R(g), R(o), R(NO_THR), 2, R(rows)),
             "no threshold is set (min_overlap 0, probe_min and build_min NULL): use the plain entry points")
    _refused(eng, L.ivj_overlap_select(h, R(g), R(neg), R(o), None, 2, R(rows)), "build.n < 0")
    # the depth family checks its sizes before the row count and before the output
    _refused(eng, L.ivj_depth_hist(h, R(_side(0)), R(g), R(o), 0, None), f"max_depth must be in 1 .. {E.MAX_HIST_DEPTH}")
    _refused(eng, L.ivj_depth_hist(h, R(_side(0)), R(g), R(o), 4, None), "hist is NULL")
    _refused(eng, L.ivj_depth_hist(h, R(neg), R(g), R(o), 0, None), "probe.n < 0")
    _refused(eng, L.ivj_depth_hist_contigs(h, R(g), R(o), 0, None), f"max_depth must be in 1 .. {E.MAX_HIST_DEPTH}")
    _refused(eng, L.ivj_depth_hist_contigs(h, R(neg), R(o), 0, None), "frame.n < 0")
    _refused(eng, L.ivj_depth_hist_contigs(h, R(g), R(bad_o), 0, None), BAD_OPTS)
    _refused(eng, L.ivj_depth_quantiles(h, R(_side(0)), R(g), R(o), 0, None, None), f"n_ranks must be in 1 .. {E.MAX_QUANT_RANKS}")
    _refused(eng, L.ivj_depth_quantiles(h, R(_side(0)), R(g), R(o), 1, None, None), "ranks is NULL")
    _refused(eng, L.ivj_depth_quantiles(h, R(g), R(neg), R(o), 0, None, None), "build.n < 0")
    _refused(eng, L.ivj_depth_summary(h, R(_side(0)), R(g), R(o), None, 9, None, None), "n_thresholds must be in 0 .. 8")
    _refused(eng, L.ivj_depth_summary(h, R(_side(0)), R(g), R(o), None, 1, None, None), "thresholds is NULL")
    _refused(eng, L.ivj_depth_summary(h, R(neg), R(g), R(o), None, 9, None, None), "probe.n < 0")
    _refused(eng, L.ivj_depth_profile(h, R(g), None, 0, R(g), R(o), None), f"n_bins must be in [1, {E.DEPTH_PROFILE_MAX_BINS}], got 0")
    _refused(eng, L.ivj_depth_profile(h, R(g), None, 0, R(neg), R(o), None), "build.n < 0")
    # nearest: the buffers before k, both after the early-out on an empty probe side
    k_opts = E.make_opts(True, NC, 2000)
    _refused(eng, L.ivj_nearest(h, R(g), R(g), R(k_opts), BUF, BUF, BUF), "nearest_k > 1024")
    _refused(eng, L.ivj_nearest(h, R(g), R(g), R(k_opts), None, BUF, BUF), "nearest output buffers are NULL")
    assert L.ivj_nearest(h, R(_side(0)), R(g), R(k_opts), None, None, None) == 0
    # one-sided entries
    merged = _out_struct(E._Merged)
    _refused(eng, L.ivj_merge(h, R(g), R(o), -1, R(merged)), "min_dist < 0")
    assert _is_empty(merged)
    _refused(eng, L.ivj_merge(h, R(neg), R(o), -1, R(merged)), "frame.n < 0")
    _refused(eng, L.ivj_merge(h, R(neg), R(bad_o), -1, R(merged)), BAD_OPTS)
    _refused(eng, L.ivj_merge(h, R(g), R(o), 0, None), "ctx or out is NULL")
    blocks = _out_struct(E._Blocks)
    _refused(eng, L.ivj_depth(h, R(_side(2, null_column=True)), R(o), R(blocks)), "frame has a NULL column")
    assert _is_empty(blocks)
    _refused(eng, L.ivj_depth(h, R(neg), R(bad_o), R(blocks)), BAD_OPTS)
    _refused(eng, L.ivj_depth(h, R(neg), R(bad_o), None), "ctx or out is NULL")
    _refused(eng, L.ivj_cluster(h, R(g), R(o), 0, None, None, None, None), "cluster output buffers are NULL")
    _refused(eng, L.ivj_cluster(h, R(neg), R(o), 0, None, None, None, None), "frame.n < 0")
    _refused(eng, L.ivj_cluster(h, R(neg), R(bad_o), 0, None, None, None, None), BAD_OPTS)
    assert L.ivj_cluster(h, R(_side(0)), R(o), 0, None, None, None, None) == 0
    # multi-frame entries
    seg = _out_struct(E._Segments)
    frames = (E._Side * 2)(_side(1), _side(-1))
    _refused(eng, L.ivj_multi_inter(h, frames, 2, R(o), 1, 0, R(seg)), "frame.n < 0")
    assert _is_empty(seg)
    _refused(eng, L.ivj_multi_inter(h, frames, 0, R(o), 1, 0, R(seg)), f"multi_inter: n_frames must be in 1 .. {E.MAX_FRAMES} and frames not NULL")
    _refused(eng, L.ivj_multi_inter(h, frames, 2, R(bad_o), 1, 0, R(seg)), BAD_OPTS)
    ok_frames = (E._Side * 2)(_side(1), _side(1))
    _refused(eng, L.ivj_multi_inter(h, ok_frames, 2, R(o), 3, 0, R(seg)), "multi_inter: min_frames must be in 1 .. n_frames (2), got 3")
    _refused(eng, L.ivj_multi_inter(h, ok_frames, 2, R(o), 3, 5, R(seg)), "multi_inter: min_frames must be in 1 .. n_frames (2), got 3")
    _refused(eng, L.ivj_multi_inter(h, ok_frames, 2, R(o), 1, 5, R(seg)), "multi_inter: mode must be 0 (segments) or 1 (consensus)")
    _refused(eng, L.ivj_multi_pairwise(h, ok_frames, 2, R(o), None, BUF), "ctx, bases or runs is NULL")
    _refused(eng, L.ivj_multi_pairwise(h, frames, 2, R(o), BUF, BUF), "frame.n < 0")
    _refused(eng, L.ivj_multi_pairwise(h, frames, 0, R(bad_o), BUF, BUF), BAD_OPTS)

    # more two-fault cases of the one-sided and multi-frame entries
    _refused(eng, L.ivj_cluster(h, R(g), R(bad_o), -1, None, None, None, None), BAD_OPTS)
    _refused(eng, L.ivj_depth(h, R(_side(2, null_column=True)), R(bad_o), R(blocks)), BAD_OPTS)
    assert _is_empty(blocks)
    _refused(eng, L.ivj_depth_hist_contigs(h, R(neg), R(bad_o), 4, None), BAD_OPTS)
    _refused(eng, L.ivj_depth_hist_contigs(h, R(neg), R(o), 4, None), "frame.n < 0")
    _refused(eng, L.ivj_depth_hist_contigs(h, R(g), R(o), 4, None), "hist is NULL")
    _refused(eng, L.ivj_multi_pairwise(h, frames, 2, R(bad_o), None, BUF), "ctx, bases or runs is NULL")
    _refused(eng, L.ivj_multi_pairwise(h, None, 2, R(o), BUF, BUF), f"multi_pairwise: n_frames must be in 1 .. {E.MAX_FRAMES} and frames not NULL")
    _refused(eng, L.ivj_multi_pairwise(h, frames, 0, R(o), BUF, BUF), f"multi_pairwise: n_frames must be in 1 .. {E.MAX_FRAMES} and frames not NULL")
    # the window's distance column: NULL after every refusal
    dist = C.cast(BUF, C.POINTER(C.c_int64))
    pairs = _out_struct(E._Pairs)
    _refused(eng, L.ivj_overlap_window(h, R(g), R(neg), R(o), None, R(pairs), R(dist)), "build.n < 0")
    assert _is_empty(pairs) and not dist
    dist = C.cast(BUF, C.POINTER(C.c_int64))
    _refused(eng, L.ivj_overlap_window(h, R(g), R(g), R(o), None, R(pairs), R(dist)), "window is NULL")
    assert not dist
    # set_stats, complement (the frame is the right side of the subtraction), overlap_rows
    three, ni = (C.c_int64 * 3)(), C.c_int64(0)
    _refused(eng, L.ivj_set_stats(h, R(g), R(g), R(o), None, R(ni)), "ctx, bases or n_intersections is NULL")
    _refused(eng, L.ivj_set_stats(h, R(neg), R(g), R(bad_o), None, R(ni)), "ctx, bases or n_intersections is NULL")
    _refused(eng, L.ivj_set_stats(h, R(neg), R(g), R(bad_o), three, R(ni)), BAD_OPTS)
    _refused(eng, L.ivj_set_stats(h, R(neg), R(_side(2, null_column=True)), R(o), three, R(ni)), "a.n < 0")
    _refused(eng, L.ivj_set_stats(h, R(g), R(neg), R(o), three, R(ni)), "b.n < 0")
    pieces = _out_struct(E._Pieces)
    _refused(eng, L.ivj_complement(h, R(neg), R(g), R(o), R(pieces)), "right.n < 0")
    assert _is_empty(pieces)
    _refused(eng, L.ivj_complement(h, R(neg), R(neg), R(o), R(pieces)), "left.n < 0")
    _refused(eng, L.ivj_complement(h, R(neg), R(neg), R(bad_o), R(pieces)), BAD_OPTS)
    _refused(eng, L.ivj_complement(h, R(neg), R(g), R(o), None), "ctx or out is NULL")
    rows = _out_struct(E._Rows)
    with_ids = _side(1)
    with_ids.row_id = BUF
    _refused(eng, L.ivj_overlap_rows(h, R(with_ids), R(g), R(o), R(rows)), "ivj_overlap_rows gathers by position: row_id must be NULL")
    assert _is_empty(rows)
    _refused(eng, L.ivj_overlap_rows(h, R(with_ids), R(neg), R(o), R(rows)), "build.n < 0")
    _refused(eng, L.ivj_overlap_rows(h, R(neg), R(neg), R(bad_o), R(rows)), BAD_OPTS)
    _refused(eng, L.ivj_overlap_rows(h, R(neg), R(g), R(o), None), "ctx or out is NULL")
    # permute_overlaps looks at its arguments before the context
    lens, offs = (C.c_int32 * NC)(*([100] * NC)), (C.c_int32 * NC)(*([5] * NC))
    perm = lambda ctx, a, b, opts, ln, of, n_perm, res: L.ivj_permute_overlaps(ctx, R(a), R(b), R(opts), ln, of, n_perm, res, res)
    _refused(eng, perm(None, g, g, o, lens, offs, 1, BUF), "ctx is NULL")
    _refused(eng, perm(None, g, neg, o, lens, offs, 1, BUF), "build.n < 0")
    _refused(eng, perm(None, neg, neg, bad_o, lens, offs, 0, None), BAD_OPTS)
    _refused(eng, perm(h, neg, g, o, lens, offs, 0, None), "probe.n < 0")
    _refused(eng, perm(h, g, neg, o, lens, offs, 0, None), "n_perm must be in [1, 2^20]")
    _refused(eng, perm(h, g, neg, o, None, offs, 1, None), "n_pairs or n_rows is NULL")
    _refused(eng, perm(h, g, neg, o, None, offs, 1, BUF), "contig_len or offsets is NULL")
    lens[1] = 0
    _refused(eng, perm(None, g, g, o, lens, offs, 1, BUF), "contig_len[1] < 1")
    lens[1] = 100
    offs[2] = 100
    _refused(eng, perm(None, g, g, o, lens, offs, 1, BUF), "offsets[0][2] is outside [0, contig_len)")
    # the value-column entries
    col = (E._AggIn * 1)(E._AggIn(BUF, None, E.AGG_I64, E.AGG_SUM))
    no_ops = (E._AggIn * 1)(E._AggIn(BUF, None, E.AGG_I64, 0))
    no_values = (E._AggIn * 1)(E._AggIn(None, None, E.AGG_I64, E.AGG_SUM))
    outs = (E._AggOut * 1)(E._AggOut(BUF, None, None, None, None))
    no_outs = (E._AggOut * 1)()
    merged = _out_struct(E._Merged)
    _refused(eng, L.ivj_merge_agg(h, R(g), R(o), 0, 1, col, R(merged), None), "ctx, out or agg_out is NULL")
    _refused(eng, L.ivj_merge_agg(h, R(neg), R(bad_o), 0, 1, col, R(merged), outs), BAD_OPTS)
    assert _is_empty(merged)
    _refused(eng, L.ivj_merge_agg(h, R(neg), R(o), -1, 0, col, R(merged), outs), "frame.n < 0")
    _refused(eng, L.ivj_merge_agg(h, R(g), R(o), -1, 0, col, R(merged), outs), "min_dist < 0")
    _refused(eng, L.ivj_merge_agg(h, R(g), R(o), 0, 0, col, R(merged), outs), f"n_cols must be in [1, {E.MAX_AGG_COLS}]")
    _refused(eng, L.ivj_merge_agg(h, R(g), R(o), 0, 1, None, R(merged), outs), "cols is NULL")
    _refused(eng, L.ivj_merge_agg(h, R(g), R(o), 0, 1, no_ops, R(merged), outs), "value column 0: ops must be a non-empty mask of IVJ_AGG_*")
    _refused(eng, L.ivj_merge_agg(h, R(g), R(o), 0, 1, no_values, R(merged), outs), "value column 0: values is NULL")
    _refused(eng, L.ivj_merge_agg(h, R(with_ids), R(o), 0, 1, no_values, R(merged), outs), "value column 0: values is NULL")
    _refused(eng, L.ivj_merge_agg(h, R(with_ids), R(o), 0, 1, col, R(merged), outs), "ivj_merge_agg reads the values by frame position: row_id must be NULL")
    assert _is_empty(merged)
    for entry in (L.ivj_overlap_agg, L.ivj_overlap_wagg):
        _refused(eng, entry(h, R(g), R(neg), R(bad_o), None, 1, col, outs), "build.n < 0")         # the build side first here
        _refused(eng, entry(h, R(neg), R(g), R(bad_o), None, 1, col, outs), BAD_OPTS)
        _refused(eng, entry(h, R(neg), R(g), R(o), R(NO_THR), 1, col, outs), "probe.n < 0")
        _refused(eng, entry(h, R(g), R(g), R(o), R(NO_THR), 0, col, outs),
                 "no threshold is set (min_overlap 0, probe_min and build_min NULL): use the plain entry points")
        _refused(eng, entry(h, R(g), R(g), R(o), None, 0, col, None), f"n_cols must be in [1, {E.MAX_AGG_COLS}]")
        _refused(eng, entry(h, R(g), R(g), R(o), None, 1, no_values, None), "value column 0: values is NULL")
        _refused(eng, entry(h, R(g), R(g), R(o), None, 1, col, None), "agg_out is NULL")
        _refused(eng, entry(h, R(g), R(g), R(o), None, 1, col, no_outs), "value column 0: an output column of a requested operation is NULL")
        assert entry(h, R(_side(0)), R(g), R(o), None, 1, col, no_outs) == 0                        # no probe rows: the outputs are not looked at
    sig = L.ivj_signal_profile
    _refused(eng, sig(h, R(g), None, 0, R(neg), R(bad_o), 1, col, outs), "build.n < 0")
    _refused(eng, sig(h, R(neg), None, 0, R(g), R(bad_o), 1, col, outs), BAD_OPTS)
    _refused(eng, sig(h, R(neg), None, 0, R(g), R(o), 1, col, outs), "windows.n < 0")
    _refused(eng, sig(h, R(g), None, 0, R(g), R(o), 0, col, outs), f"n_bins must be in [1, {E.DEPTH_PROFILE_MAX_BINS}], got 0")
    _refused(eng, sig(h, R(g), None, 2, R(g), R(o), 0, col, None), f"n_cols must be in [1, {E.MAX_AGG_COLS}]")
    _refused(eng, sig(h, R(g), None, 2, R(g), R(o), 1, col, None), "agg_out is NULL")
    _refused(eng, sig(h, R(g), None, 2, R(g), R(o), 1, col, no_outs), "value column 0: an output column of a requested operation is NULL")
    # take
    one_ptr, one_rows, four, eight = (C.c_void_p * 1)(BUF), (C.c_int64 * 1)(1), (C.c_int32 * 1)(4), (C.c_int32 * 1)(3)
    _refused(eng, L.ivj_take(None, BUF, 1, 1, one_ptr, one_rows, four, one_ptr, None), "ctx is NULL")
    _refused(eng, L.ivj_take(h, None, -1, 1, one_ptr, one_rows, four, one_ptr, None), "take: negative size")
    _refused(eng, L.ivj_take(h, None, 1, 1, one_ptr, one_rows, eight, one_ptr, None), "take: NULL argument")
    _refused(eng, L.ivj_take(h, BUF, 1, 1, one_ptr, one_rows, eight, (C.c_void_p * 1)(None), None), "take: elem_bytes must be 4 or 8")
    _refused(eng, L.ivj_take(h, BUF, 1, 1, one_ptr, one_rows, four, (C.c_void_p * 1)(None), None), "take: bad column")
    assert L.ivj_take(h, None, 0, 1, None, None, None, None, None) == 0


# ---------------------------------------------------------------------------------------------- edges of the frame, vs the oracle

EMPTY = tuple(np.empty(0, np.int32) for _ in range(3))


def _one(contig, start, end):
    return tuple(np.array([v], np.int32) for v in (contig, start, end))


def _sides():
    rng = np.random.default_rng(11)
    big_p, big_b = random_side(rng, 1000, NC, 20_000, 300), random_side(rng, 300, NC, 20_000, 300)
    return {
        "probe0_build300": (EMPTY, big_b),
        "probe300_build0": (big_b, EMPTY),
        "both_empty": (EMPTY, EMPTY),
        "one_one_overlapping": (_one(1, 100, 200), _one(1, 150, 250)),
        "one_one_other_contig": (_one(1, 100, 200), _one(2, 150, 250)),
        "probe1000_build300": (big_p, big_b),
    }


SIDES = _sides()
ORACLE = OracleEngine()
_reference = {}


def reference(op, case, strict):
    """The oracle's answer, computed once per (operation, case, mode) and shared."""
    key = (op, case, strict)
    if key not in _reference:
        p, b = SIDES[case]
        if op in ("merge", "cluster"):
            _reference[key] = getattr(ORACLE, op)(p, strict, NC)
        else:
            _reference[key] = getattr(ORACLE, op)(p, b, strict, NC)
    return _reference[key]


def _sorted_pairs(p, b):
    o = np.lexsort((b, p))
    return np.asarray(p)[o], np.asarray(b)[o]


def _same(got, exp):
    assert len(got) == len(exp)
    for g, x in zip(got, exp):
        g, x = np.asarray(g), np.asarray(x)
        assert g.size == x.size and (g.ravel() == x.ravel()).all()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "weak"])
@pytest.mark.parametrize("case", sorted(SIDES))
def test_edges_against_oracle(eng, case, strict):
    probe, build = SIDES[case]
    n = len(probe[0])
    ep, eb = _sorted_pairs(*reference("overlap", case, strict))
    counts = reference("count_overlaps", case, strict)
    non_empty = case == "probe1000_build300"
    if non_empty:
        assert len(ep) > 0 and (counts == 0).any() and (counts > 0).any()

    p, b = eng.overlap(probe, build, strict, NC)
    assert p.dtype == np.int32 and b.dtype == np.int32
    _same(_sorted_pairs(p, b), (ep, eb))
    got = eng.count_overlaps(probe, build, strict, NC)
    assert got.dtype == np.int64
    _same([got], [counts])
    _same(eng.nearest(probe, build, strict, NC), reference("nearest", case, strict))
    _same([eng.coverage(probe, build, strict, NC)], [reference("coverage", case, strict)])
    _same(eng.subtract(probe, build, strict, NC), reference("subtract", case, strict))
    _same(eng.complement(build, probe, strict, NC), reference("subtract", case, strict))
    _same(eng.merge(probe, strict, NC), reference("merge", case, strict))
    cid, cs, ce, ncl = eng.cluster(probe, strict, NC)
    xcid, xcs, xce, xn = reference("cluster", case, strict)
    _same((cid, cs, ce), (xcid, xcs, xce))
    assert ncl == xn

    # join kinds, from the oracle's counts and pairs: semi / anti rows ascending, outer = the inner pairs then (row, -1)
    semi, anti = np.nonzero(counts > 0)[0].astype(np.int32), np.nonzero(counts == 0)[0].astype(np.int32)
    _same([eng.overlap_select(probe, build, strict, NC, "semi")], [semi])
    _same([eng.overlap_select(probe, build, strict, NC, "anti")], [anti])
    op_, ob_ = eng.overlap_outer(probe, build, strict, NC)
    assert len(op_) == len(ep) + len(anti)
    _same(_sorted_pairs(op_[:len(ep)], ob_[:len(ep)]), (ep, eb))
    _same((op_[len(ep):], ob_[len(ep):]), (anti, np.full(len(anti), -1, np.int32)))

    # rows: the pairs with both sides' key columns
    rows = eng.overlap_rows(probe, build, strict, NC)
    o = np.lexsort((rows["build_idx"], rows["probe_idx"]))
    _same((rows["probe_idx"][o], rows["build_idx"][o]), (ep, eb))
    _same((rows["contig"][o], rows["start_1"][o], rows["end_2"][o]), (probe[0][ep], probe[1][ep], build[2][eb]))

    # thresholds and the distance window against their brute-force forms; the window in both distance modes
    tp, tb, tcounts = T.brute(probe, build, NC, strict, min_overlap=2)
    _same(_sorted_pairs(*eng.overlap_thresh(probe, build, strict, NC, min_overlap=2)), (tp, tb))
    _same([eng.count_overlaps_thresh(probe, build, strict, NC, min_overlap=2)], [tcounts])
    xp, xb, xd, wcounts = WU.brute(probe, build, NC, strict, 50, 30, 0)
    wp, wb, wd = eng.overlap_window(probe, build, strict, NC, left=50, right=30, distance=True)
    assert wd.dtype == np.int64
    _same(WU.sort_pairs(wp, wb, wd), (xp, xb, xd))
    wp, wb, none = eng.overlap_window(probe, build, strict, NC, left=50, right=30, distance=False)
    assert none is None
    _same(_sorted_pairs(wp, wb), (xp, xb))
    _same([eng.count_window(probe, build, strict, NC, left=50, right=30)], [wcounts])
    if non_empty:
        assert len(tp) > 0 and len(xp) > len(ep)

    # the depth family
    bases = eng.overlap_bases(probe, build, strict, NC)
    DSU.assert_bases_equal(bases, DSU.pair_form(probe, build, strict, NC))
    summary = DSM.block_form(probe, build, strict, NC, (1, 2))
    DSM.assert_summary_equal(eng.depth_summary(probe, build, strict, NC, thresholds=(1, 2)), summary)
    none, bg = eng.depth_summary(probe, build, strict, NC, thresholds=(1, 2), want_max=False)
    assert none is None
    DSM.assert_summary_equal((None, bg), summary)
    md, bg0 = eng.depth_summary(probe, build, strict, NC, thresholds=())
    assert bg0.shape == (0, n) and bg0.dtype == np.int64
    DSM.assert_summary_equal((md, summary[1]), summary)
    DH.assert_hist_equal(eng.depth_hist(probe, build, strict, NC, 4), DH.block_form(probe, build, strict, NC, 4))
    DH.assert_hist_equal(eng.depth_hist_contigs(build, strict, NC, 4), DH.contig_form(build, strict, NC, 4))
    ranks = DQ.ranks_for(probe, strict, NC, 2, 1)
    DQ.assert_quant_equal(eng.depth_quantiles(probe, build, strict, NC, ranks), DQ.dense_form(probe, build, strict, NC, ranks))
    reverse = (np.arange(n) % 2).astype(bool)
    for rev in (None, reverse):
        DP.assert_profile_equal(eng.depth_profile(probe, rev, 2, build, strict, NC), DP.expected_bases(probe, build, strict, NC, 2, rev))
    DU.assert_blocks_equal(eng.depth(probe, strict, NC), DU.depth_events(*probe, strict, NC))

    # value columns: merge_agg over the frame, map / signal over the build side, the profile over the bins
    ops = ["sum", "min", "max", "mean", "count"]
    pv, pok = (np.arange(n, dtype=np.int64) * 7 - 300), (np.arange(n) % 3 != 0)
    bv, bok = (np.arange(len(build[0]), dtype=np.int64) * 5 - 200), (np.arange(len(build[0])) % 4 != 0)
    *table, (res,) = eng.merge_agg(probe, strict, NC, [(pv, pok, ops)])
    cid, xtable = MA.clusters(probe, NC, strict)
    _same(table, xtable)
    MA.assert_column(res, MA.group_by(cid, len(xtable[0]), pv, pok), np.int64, "merge_agg")
    (res,) = eng.overlap_agg(probe, build, strict, NC, [(bv, bok, ops)])
    OA.assert_column(res, OA.expected(probe, build, NC, strict, bv, bok), np.int64, "overlap_agg")
    (res,) = eng.overlap_agg(probe, build, strict, NC, [(bv, bok, ops)], min_overlap=2)
    OA.assert_column(res, OA.expected(probe, build, NC, strict, bv, bok, min_overlap=2), np.int64, "overlap_agg, thresholds")
    (res,) = eng.overlap_wagg(probe, build, strict, NC, [(bv, bok, ops)])
    SG.assert_column(res, SG.summary(probe, build, NC, strict, bv, bok), np.int64, "overlap_wagg")
    (res,) = eng.signal_profile(probe, reverse, 2, build, strict, NC, [(bv, bok, ops)])
    assert all(a.shape == (n, 2) for a in res.values())
    SG.assert_column({k: a.reshape(-1) for k, a in res.items()}, SG.profile(probe, build, NC, strict, 2, bv, bok, reverse), np.int64, "signal_profile")

    # permutations and take
    lengths = np.full(NC, 50_000, np.int32)
    offsets = np.random.default_rng(5).integers(0, 50_000, (2, NC)).astype(np.int32)
    _same(eng.permute_overlaps(probe, build, strict, NC, lengths, offsets), PM.expected(probe, build, NC, strict, lengths, offsets))
    (t32, none), (t64, none2) = eng.take_columns(ep, [probe[1], pv])
    assert none is None and none2 is None and t32.dtype == np.int32 and t64.dtype == np.int64
    _same((t32, t64), (probe[1][ep], pv[ep]))

    # position sets of two and of three frames (one of them empty); segments with and without the mask
    only_a, only_b, both, n_inter = eng.set_stats(probe, build, strict, NC)
    two = [probe, build]
    xb2, xr2 = PW.pairwise_events(two, strict, NC)
    assert (only_a + both, only_b + both, both, n_inter) == (xb2[0, 0], xb2[1, 1], xb2[0, 1], xr2[0, 1])
    MU.assert_equal((*eng.setop(probe, build, "union", strict, NC), None), MU.multi_events(two, strict, NC, 1, True))
    MU.assert_equal((*eng.setop(probe, build, "intersection", strict, NC), None), MU.multi_events(two, strict, NC, 2, True))
    for frames in (two, [probe, EMPTY, build]):
        MU.assert_equal(eng.multi_inter(frames, 1, E.MULTI_SEGMENTS, strict, NC), MU.multi_events(frames, strict, NC, 1, False))
        MU.assert_equal(eng.multi_inter(frames, 2, E.MULTI_CONSENSUS, strict, NC), MU.multi_events(frames, strict, NC, 2, True))
        _same(eng.multi_pairwise(frames, strict, NC), PW.pairwise_events(frames, strict, NC))


def test_columns_that_need_converting(eng):
    """Lists, int64 and strided columns are converted to contiguous int32 copies that only the call's keep-alive holds: every host
    method has to give what it gives for the int32 columns (a copy released before the library read it would not)."""
    probe, build = SIDES["probe1000_build300"]
    wide = lambda side: tuple(a.astype(np.int64) for a in side)
    strided = lambda side: tuple(np.repeat(a, 2)[::2] for a in side)
    ranks = DQ.ranks_for(probe, True, NC, 2, 1)
    calls = {
        "overlap": lambda p, b: _sorted_pairs(*eng.overlap(p, b, True, NC)),
        "count_overlaps": lambda p, b: [eng.count_overlaps(p, b, True, NC)],
        "nearest": lambda p, b: eng.nearest(p, b, True, NC),
        "depth_hist": lambda p, b: [eng.depth_hist(p, b, True, NC, 4)],
        "depth_hist_contigs": lambda p, b: [eng.depth_hist_contigs(b, True, NC, 4)],
        "depth_quantiles": lambda p, b: [eng.depth_quantiles(p, b, True, NC, ranks)],
        "depth_summary": lambda p, b: eng.depth_summary(p, b, True, NC, thresholds=(1, 2)),
        "depth_profile": lambda p, b: [eng.depth_profile(p, None, 2, b, True, NC)],
        "overlap_window": lambda p, b: WU.sort_pairs(*eng.overlap_window(p, b, True, NC, left=50, right=30)),
        "overlap_thresh": lambda p, b: _sorted_pairs(*eng.overlap_thresh(p, b, True, NC, min_overlap=2)),
        "subtract": lambda p, b: eng.subtract(p, b, True, NC),
        "setop": lambda p, b: eng.setop(p, b, "union", True, NC),
        "merge": lambda p, b: eng.merge(p, True, NC),
        "multi_inter": lambda p, b: eng.multi_inter([p, b], 1, E.MULTI_SEGMENTS, True, NC),
        "multi_pairwise": lambda p, b: eng.multi_pairwise([p, b], True, NC),
    }
    for name, call in calls.items():
        want = call(probe, build)
        for form in (wide, strided, lambda side: tuple(a.tolist() for a in side)):
            _same(call(form(probe), form(build)), want)
