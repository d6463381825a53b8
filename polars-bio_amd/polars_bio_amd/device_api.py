"""Device-resident range operations on torch CUDA(=HIP) tensors.

torch is plumbing here (device memory, the current stream, torch.distributed); the
work is done by libivjoin_hip.so through the ``*_dev`` entry points of include/ivjoin.h.
Columns are int32 torch tensors already resident in HBM; results stay in HBM.

Import order: torch wheels bundle their own ROCm runtime; in a process that uses both, import
torch BEFORE the first ``Engine`` is created (this module does so itself), otherwise torch may not
see its GPUs ("No HIP GPUs are available").
"""

from __future__ import annotations

import torch  # noqa: F401  (must precede the dlopen of libivjoin_hip.so in this process)

from typing import Optional, Tuple

from ._engine import (AGG_F64, AGG_I64, AGG_OPS, MULTI_CONSENSUS, MULTI_SEGMENTS, DeviceIndex, Engine, agg_ops_mask, check_multi, make_opts,
                      make_thresholds, make_window, select_mode)


class DeviceSide:
    """(contig, start, end[, row_id]) int32 CUDA tensors of one side."""

    def __init__(self, contig, start, end, row_id=None):
        import torch
        for t in (contig, start, end) + ((row_id,) if row_id is not None else ()):
            if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError("columns must be contiguous int32 CUDA tensors")
        self.contig, self.start, self.end, self.row_id = contig, start, end, row_id
        self.n = int(contig.shape[0])

    def as_c(self):
        return Engine.dev_side(self.contig.data_ptr(), self.start.data_ptr(), self.end.data_ptr(), self.n,
                               self.row_id.data_ptr() if self.row_id is not None else 0)


class DeviceJoin:
    """One engine bound to torch's current stream on ``device``."""

    def __init__(self, device: int = 0):
        import torch
        self.torch = torch
        self.device = device
        torch.cuda.set_device(device)
        self.engine = Engine(device)
        self.engine.set_stream(torch.cuda.current_stream(device).cuda_stream)

    def group(self, probe: DeviceSide, build: DeviceSide, probe_codes, build_codes, cards, n_contigs: int):
        """Joins keyed on extra columns (on_cols) in HBM: ivj_group_ids_dev turns (contig, code_1, ..., code_K) of both sides into
        dense group ids.  ``probe_codes`` / ``build_codes``: one contiguous int32 CUDA tensor per on_col (codes of a dictionary
        shared by both sides, in [0, cards[j]); negative = null).  -> (probe', build', n_groups, group_keys) where the sides
        carry the group ids as ``contig`` (-1: a null component or a key the build side lacks), so every other method of this
        class, called with ``n_contigs=max(n_groups, 1)``, runs within groups; group_keys is an (n_groups, 1 + K) int32 tensor
        of (contig, code_1, ..., code_K) per group id, in ascending key order."""
        torch = self.torch
        cards = [int(c) for c in cards]
        if len(probe_codes) != len(cards) or len(build_codes) != len(cards):
            raise ValueError("one code column per on_col on each side")
        for side, codes in ((probe, probe_codes), (build, build_codes)):
            for t in codes:
                if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or int(t.shape[0]) != side.n:
                    raise ValueError("code columns must be contiguous int32 CUDA tensors of the side's length")
        domain = int(n_contigs)
        for c in cards:
            domain *= c
        if domain > (1 << 31):
            raise ValueError(f"on_cols key space too large: {n_contigs} contigs x {cards} distinct values = {domain} keys, the limit is 2^31")
        dev = build.start.device
        cap = max(1, min(build.n, domain))
        keys = torch.empty((cap, 1 + len(cards)), dtype=torch.int32, device=dev)
        pg = torch.empty(probe.n, dtype=torch.int32, device=probe.start.device)
        bg = torch.empty(build.n, dtype=torch.int32, device=dev)
        g = self.engine.group_ids_dev(probe.contig.data_ptr(), [t.data_ptr() for t in probe_codes], probe.n, build.contig.data_ptr(),
                                      [t.data_ptr() for t in build_codes], build.n, cards, int(n_contigs), pg.data_ptr(), bg.data_ptr(),
                                      keys.data_ptr(), cap)
        return (DeviceSide(pg, probe.start, probe.end, probe.row_id), DeviceSide(bg, build.start, build.end, build.row_id), g, keys[:g])

    def build_index(self, build: DeviceSide, strict: bool, n_contigs: int, with_end_order: bool = False):
        return self.engine.index_build_dev(build.as_c(), make_opts(strict, n_contigs), with_end_order)

    def overlap(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, index=None, out=None,
                fused: bool = True, partition_mode: int = 0):
        """Index build (radix sort) + count + scan + fill.  -> (probe_idx, build_idx) int32 tensors.
        ``out``: optional pair of preallocated int32 CUDA tensors; views of their first n_pairs
        elements are returned when they are large enough (no allocation on the call path).  With
        ``out`` and ``fused`` the single-pass ivj_overlap_fused_dev is tried first."""
        torch = self.torch
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, False) if own else index
        try:
            side = probe.as_c()
            if out is not None and fused:
                # single fused pass into the caller's buffers (the library picks the window-scan kernel for
                # sparse results and the flat candidate kernel when the buffers say >= 16 pairs per probe)
                cap = min(out[0].numel(), out[1].numel())
                total, fits = self.engine.overlap_fused_dev(ix, side, opts, out[0].data_ptr(), out[1].data_ptr(), cap)
                if fits:
                    return out[0][:total], out[1][:total]
            total = self.engine.overlap_count_dev(ix, side, opts)
            if out is not None and out[0].numel() >= total and out[1].numel() >= total:
                out_p, out_b = out[0][:total], out[1][:total]
            else:
                out_p = torch.empty(total, dtype=torch.int32, device=probe.start.device)
                out_b = torch.empty(total, dtype=torch.int32, device=probe.start.device)
            self.engine.overlap_fill_dev(ix, side, opts, out_p.data_ptr(), out_b.data_ptr(), total)
        finally:
            if own:
                ix.close()
        return out_p, out_b

    def overlap_rows(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, out: dict, index=None,
                     partition_mode: int = 0):
        """Join + row materialisation in one pass (ivj_overlap_fused_rows_dev) into the preallocated int32
        CUDA tensors of ``out`` (keys from _engine.ROW_COLUMNS; a missing key = column not wanted).
        -> (dict of views of the first n_rows elements, n_rows, fits); fits=False: grow ``out`` to n_rows."""
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, False) if own else index
        try:
            cap = min(int(t.numel()) for t in out.values())
            ptrs = {f"{k}_ptr": t.data_ptr() for k, t in out.items()}
            total, fits = self.engine.overlap_fused_rows_dev(ix, probe.as_c(), opts, cap, **ptrs)
        finally:
            if own:
                ix.close()
        return ({k: t[:total] for k, t in out.items()} if fits else {}), total, fits

    def materialize(self, probe: DeviceSide, build: DeviceSide, probe_idx, build_idx, out=None):
        """Row materialisation (ivj_materialize_dev): for every pair the key columns of both sides.
        -> dict contig / start_1 / end_1 / start_2 / end_2 of int32 CUDA tensors (``out``: optional dict
        of preallocated tensors of at least n_pairs elements)."""
        torch = self.torch
        n = int(probe_idx.shape[0])
        names = ("contig", "start_1", "end_1", "start_2", "end_2")
        cols = {k: (out[k][:n] if out is not None else torch.empty(n, dtype=torch.int32, device=probe.start.device)) for k in names}
        self.engine.materialize_dev(probe.as_c(), build.as_c(), n, probe_idx.data_ptr(), build_idx.data_ptr(),
                                    *(cols[k].data_ptr() for k in names))
        return cols

    def take(self, column, idx, with_validity: bool = False):
        """Arrow take of one 4- or 8-byte CUDA column by int32 row indices (negative -> 0 / null).
        -> values, or (values, validity bitmap as int64 words) with ``with_validity``."""
        torch = self.torch
        if column.element_size() not in (4, 8) or not column.is_contiguous():
            raise ValueError("column must be a contiguous tensor of 4- or 8-byte elements")
        n = int(idx.shape[0])
        dst = torch.empty(n, dtype=column.dtype, device=column.device)
        val = torch.zeros((n + 63) // 64, dtype=torch.int64, device=column.device) if with_validity else None
        self.engine.take_dev(column.data_ptr(), column.element_size(), idx.data_ptr(), n, dst.data_ptr(),
                             val.data_ptr() if val is not None else 0)
        return (dst, val) if with_validity else dst

    def count_overlaps(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, index=None,
                       partition_mode: int = 0):
        torch = self.torch
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, True) if own else index
        try:
            out = torch.empty(probe.n, dtype=torch.int64, device=probe.start.device)
            self.engine.count_overlaps_dev(ix, probe.as_c(), opts, out.data_ptr())
        finally:
            if own:
                ix.close()
        return out

    # ---- overlap thresholds (include/ivjoin.h: ivj_thresholds) ---------------------------------------
    def _thresholds(self, probe: DeviceSide, build: DeviceSide, min_overlap: int, probe_min, build_min):
        """probe_min / build_min: contiguous CUDA tensors of one 4-byte unsigned base count per row (torch.uint32, or torch.int32
        holding the same bits: -1 = never), or None."""
        torch = self.torch
        for t, side, what in ((probe_min, probe, "probe_min"), (build_min, build, "build_min")):
            if t is None:
                continue
            if t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (side.n,):
                raise ValueError(f"{what} must be a contiguous 4-byte integer CUDA tensor with one element per row")
        if not min_overlap and probe_min is None and build_min is None:
            raise ValueError("no threshold is set: use overlap / count_overlaps")
        return make_thresholds(min_overlap, probe_min.data_ptr() if probe_min is not None and probe.n else 0,
                               build_min.data_ptr() if build_min is not None and build.n else 0)

    def overlap_thresh(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, min_overlap: int = 0, probe_min=None,
                       build_min=None, index=None, out=None, partition_mode: int = 0):
        """Thresholded join (ivj_overlap_thresh_dev): the pairs with ov >= max(1, min_overlap, probe_min[probe row],
        build_min[build row]) -> (probe_idx, build_idx) int32 tensors.  ``out``: optional pair of preallocated int32 CUDA tensors,
        used when they hold the result (views of their first n_pairs elements come back)."""
        torch = self.torch
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        thr = self._thresholds(probe, build, min_overlap, probe_min, build_min)
        if probe.n == 0 or build.n == 0:
            e = torch.empty(0, dtype=torch.int32, device=probe.start.device)
            return e, e.clone()
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, False) if own else index
        try:
            side = probe.as_c()
            if out is not None:
                total, fits = self.engine.overlap_thresh_dev(ix, side, opts, thr, out[0].data_ptr(), out[1].data_ptr(),
                                                             min(out[0].numel(), out[1].numel()))
                if fits:
                    return out[0][:total], out[1][:total]
            else:
                total, _ = self.engine.overlap_thresh_dev(ix, side, opts, thr, 0, 0, 0)
            out_p = torch.empty(total, dtype=torch.int32, device=probe.start.device)
            out_b = torch.empty(total, dtype=torch.int32, device=probe.start.device)
            if total:
                self.engine.overlap_thresh_dev(ix, side, opts, thr, out_p.data_ptr(), out_b.data_ptr(), total)
        finally:
            if own:
                ix.close()
        return out_p, out_b

    def count_overlaps_thresh(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, min_overlap: int = 0,
                              probe_min=None, build_min=None, index=None, partition_mode: int = 0):
        """Thresholded count (ivj_count_overlaps_thresh_dev) -> int64 tensor, probe order kept."""
        torch = self.torch
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        thr = self._thresholds(probe, build, min_overlap, probe_min, build_min)
        out = torch.zeros(probe.n, dtype=torch.int64, device=probe.start.device)
        if probe.n == 0 or build.n == 0:
            return out
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, False) if own else index
        try:
            self.engine.count_overlaps_thresh_dev(ix, probe.as_c(), opts, thr, out.data_ptr())
        finally:
            if own:
                ix.close()
        return out

    # ---- distance window (include/ivjoin.h: ivj_window) ----------------------------------------------
    def _window(self, probe: DeviceSide, left: int, right: int, probe_left, probe_right, min_distance: int):
        """probe_left / probe_right: contiguous CUDA tensors of one 4-byte unsigned extent per probe row (torch.uint32, or torch.int32
        holding the same bits), or None for the scalar."""
        torch = self.torch
        for t, what in ((probe_left, "probe_left"), (probe_right, "probe_right")):
            if t is None:
                continue
            if t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (probe.n,):
                raise ValueError(f"{what} must be a contiguous 4-byte integer CUDA tensor with one element per probe row")
        return make_window(left, right, probe_left.data_ptr() if probe_left is not None and probe.n else 0,
                           probe_right.data_ptr() if probe_right is not None and probe.n else 0, min_distance)

    def overlap_window(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, left: int = 0, right: int = 0,
                       min_distance: int = 0, probe_left=None, probe_right=None, distance: bool = True, index=None, out=None,
                       partition_mode: int = 0):
        """Distance-window join (ivj_overlap_window_dev): every build row within ``left`` / ``right`` bases of each probe row and at
        least ``min_distance`` away -> (probe_idx, build_idx, dist): int32, int32 and -- with ``distance`` -- the signed int64
        distance (else None).  ``out``: optional preallocated CUDA tensors (int32, int32[, int64]), used when they hold the result
        (views of their first n_pairs elements come back)."""
        torch = self.torch
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        win = self._window(probe, left, right, probe_left, probe_right, min_distance)
        dev = probe.start.device
        if probe.n == 0 or build.n == 0:
            e = torch.empty(0, dtype=torch.int32, device=dev)
            return e, e.clone(), (torch.empty(0, dtype=torch.int64, device=dev) if distance else None)
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, False) if own else index
        try:
            side = probe.as_c()
            if out is not None:
                if distance and len(out) < 3:
                    raise ValueError("out must hold an int64 tensor for the distances")
                cols = out[:3] if distance else out[:2]
                total, fits = self.engine.overlap_window_dev(ix, side, opts, win, cols[0].data_ptr(), cols[1].data_ptr(),
                                                             cols[2].data_ptr() if distance else 0, min(t.numel() for t in cols))
                if fits:
                    return cols[0][:total], cols[1][:total], (cols[2][:total] if distance else None)
            else:
                total, _ = self.engine.overlap_window_dev(ix, side, opts, win, 0, 0, 0, 0)
            out_p = torch.empty(total, dtype=torch.int32, device=dev)
            out_b = torch.empty(total, dtype=torch.int32, device=dev)
            out_d = torch.empty(total, dtype=torch.int64, device=dev) if distance else None
            if total:
                self.engine.overlap_window_dev(ix, side, opts, win, out_p.data_ptr(), out_b.data_ptr(), out_d.data_ptr() if distance else 0, total)
        finally:
            if own:
                ix.close()
        return out_p, out_b, out_d

    def count_window(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, left: int = 0, right: int = 0,
                     min_distance: int = 0, probe_left=None, probe_right=None, index=None, out=None, partition_mode: int = 0):
        """Distance-window count (ivj_count_window_dev) -> int64 tensor, probe order kept (``out``: optional int64 CUDA tensor of
        probe.n elements)."""
        torch = self.torch
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        win = self._window(probe, left, right, probe_left, probe_right, min_distance)
        if out is None:
            out = torch.zeros(probe.n, dtype=torch.int64, device=probe.start.device)
        elif out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (probe.n,):
            raise ValueError("out must be a contiguous int64 CUDA tensor with one element per probe row")
        if probe.n == 0 or build.n == 0:
            return out.zero_()
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, False) if own else index
        try:
            self.engine.count_window_dev(ix, probe.as_c(), opts, win, out.data_ptr())
        finally:
            if own:
                ix.close()
        return out

    # ---- permutation_test (include/ivjoin.h: ivj_permute_overlaps_dev) ---------------------------------
    def permute_overlaps(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, contig_len, offsets, index=None,
                         partition_mode: int = 0):
        """Overlap statistics of ``probe`` under circular shifts: ``contig_len`` int32 CUDA tensor [n_contigs] (>= 1), ``offsets``
        int32 CUDA tensor [n_perm, n_contigs] with 0 <= offsets[p, c] < contig_len[c] (NOT validated here: values outside give
        unspecified statistics, never a read outside the tables).  -> (n_pairs, n_rows) int64 tensors of length n_perm."""
        torch = self.torch
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        for t, what in ((contig_len, "contig_len"), (offsets, "offsets")):
            if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous int32 CUDA tensor")
        if offsets.dim() != 2 or offsets.shape[1] != n_contigs or tuple(contig_len.shape) != (n_contigs,):
            raise ValueError(f"offsets must be [n_perm, {n_contigs}] and contig_len [{n_contigs}]")
        n_perm = int(offsets.shape[0])
        pairs = torch.zeros(n_perm, dtype=torch.int64, device=probe.start.device)
        rows = torch.zeros(n_perm, dtype=torch.int64, device=probe.start.device)
        if n_perm and (probe.n == 0 or build.n == 0 or n_contigs == 0):
            return pairs, rows
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, True) if own else index
        try:
            self.engine.permute_overlaps_dev(ix, probe.as_c(), opts, contig_len.data_ptr(), offsets.data_ptr(), n_perm, pairs.data_ptr(),
                                             rows.data_ptr())
        finally:
            if own:
                ix.close()
        return pairs, rows

    # ---- map_overlaps (include/ivjoin.h: ivj_overlap_agg_dev) ------------------------------------------
    def overlap_agg(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, agg, min_overlap: int = 0, probe_min=None,
                    build_min=None, index=None, partition_mode: int = 0):
        """Build-side value columns reduced over each probe row's matches (ivj_overlap_agg_dev), all in HBM.  ``agg``: a list of
        (values, valid, ops) per value column as in ``merge`` -- the values indexed by the build side's rows (by its ``row_id``
        where it carries one; rows beyond the column's length contribute nothing).  The predicate is the plain one, or the
        thresholded one when min_overlap / probe_min / build_min are given (as in ``count_overlaps_thresh``).  -> one dict per
        column, name -> tensor of probe.n elements in probe order: sum int64 (wrapped) / float64, min / max the column's type,
        mean float64, count int64.  sum and count are 0 where nothing valid matches; min / max / mean are unspecified there."""
        return self._overlap_agg(False, probe, build, strict, n_contigs, agg, min_overlap, probe_min, build_min, index, partition_mode)

    def overlap_wagg(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, agg, min_overlap: int = 0, probe_min=None,
                     build_min=None, index=None, partition_mode: int = 0):
        """The build side as a signal track (ivj_overlap_wagg_dev), all in HBM: arguments and results as ``overlap_agg``, but a build
        row contributes iff it shares ov >= max(1, minima) positions with the probe row and then weighs ov -- ``count`` holds the
        bases (sum of ov), ``sum`` the sum of value * ov (int64 wrapped / float64), ``mean`` = sum / bases, ``min`` / ``max`` the
        extremes of the contributing values, unweighted.  Rows of either side that cover no position share nothing."""
        return self._overlap_agg(True, probe, build, strict, n_contigs, agg, min_overlap, probe_min, build_min, index, partition_mode)

    def _agg_columns(self, agg):
        """-> ([(values, valid, dtype, ops mask)], n_values) of a list of (values, valid, ops) on CUDA tensors."""
        torch = self.torch
        cols = []
        for values, valid, ops in list(agg):
            if values.dtype not in (torch.int64, torch.float64) or not values.is_cuda or not values.is_contiguous() or values.dim() != 1:
                raise ValueError("value columns must be contiguous 1-D int64 or float64 CUDA tensors")
            if valid is not None and (valid.dtype not in (torch.bool, torch.uint8) or not valid.is_cuda or not valid.is_contiguous()
                                      or valid.shape != values.shape):
                raise ValueError("validity columns must be contiguous bool / uint8 CUDA tensors of the value column's length")
            cols.append((values, valid, AGG_I64 if values.dtype == torch.int64 else AGG_F64, agg_ops_mask(ops)))
        lengths = {int(v.shape[0]) for v, _, _, _ in cols}
        if len(lengths) > 1:
            raise ValueError(f"the value columns of one call must have one length, got {sorted(lengths)}")
        return cols, (lengths.pop() if lengths else 0)

    def _agg_results(self, cols, shape, dev):
        torch = self.torch
        kinds = {"sum": None, "min": None, "max": None, "mean": torch.float64, "count": torch.int64}
        return [{name: torch.zeros(shape, dtype=kinds[name] or values.dtype, device=dev) for name, bit in AGG_OPS.items() if ops & bit}
                for values, _, _, ops in cols]

    def _overlap_agg(self, weighted, probe, build, strict, n_contigs, agg, min_overlap, probe_min, build_min, index, partition_mode):
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        plain = not min_overlap and probe_min is None and build_min is None
        thr = None if plain else self._thresholds(probe, build, min_overlap, probe_min, build_min)
        cols, n_values = self._agg_columns(agg)
        results = self._agg_results(cols, probe.n, probe.start.device)
        if build.n == 0:
            plain, thr = True, None                            # every count is 0 under either predicate
        own = index is None
        # (the weighted walk is the thresholded one: it reads no end order)
        ix = self.engine.index_build_dev(build.as_c(), opts, plain and not weighted) if own else index
        try:
            (self.engine.overlap_wagg_dev if weighted else self.engine.overlap_agg_dev)(
                ix, probe.as_c(), opts, thr, n_values,
                [(v.data_ptr() if n_values else 0, (m.data_ptr() if m is not None and n_values else 0), dt, ops) for v, m, dt, ops in cols],
                [{name: (t.data_ptr() if probe.n else 0) for name, t in r.items()} for r in results])
        finally:
            if own:
                ix.close()
        return results

    # ---- map_quantiles (include/ivjoin.h: ivj_overlap_quantiles_dev) -----------------------------------
    def overlap_quantiles(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, values, valid, q, upper,
                          min_overlap: int = 0, probe_min=None, build_min=None, index=None, partition_mode: int = 0):
        """Exact order statistics of ONE build-side value column over each probe row's matches (ivj_overlap_quantiles_dev), all in
        HBM.  ``values`` / ``valid`` as one column of ``overlap_agg``; ``q`` / ``upper``: host sequences of 1 .. 16 floats in
        [0, 1] and one flag each.  With the m valid matched values of a row sorted (int64 signed; doubles as a numeric sort, NaN
        last): cell (row, j) = v[floor(q_j (m - 1))], or v[ceil(q_j (m - 1))] where upper_j is set.  The predicate is the plain one,
        or the thresholded one when min_overlap / probe_min / build_min are given.  -> (out (probe.n, len(q)) in the values'
        dtype, count int64 (probe.n,) = m), probe order; rows with m == 0 hold zeros."""
        torch = self.torch
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        plain = not min_overlap and probe_min is None and build_min is None
        thr = None if plain else self._thresholds(probe, build, min_overlap, probe_min, build_min)
        (values, valid, dtype, _), = self._agg_columns([(values, valid, "count")])[0]
        n_values = int(values.shape[0])
        n_q = len(q)
        dev = probe.start.device
        out = torch.zeros((probe.n, n_q), dtype=values.dtype, device=dev)
        count = torch.zeros(probe.n, dtype=torch.int64, device=dev)
        if build.n == 0:
            plain, thr = True, None                            # every count is 0 under either predicate
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, plain) if own else index
        try:
            self.engine.overlap_quantiles_dev(ix, probe.as_c(), opts, thr, n_values,
                                              (values.data_ptr() if n_values else 0, valid.data_ptr() if valid is not None and n_values else 0, dtype),
                                              q, upper, out.data_ptr() if out.numel() else 0, count.data_ptr() if probe.n else 0)
        finally:
            if own:
                ix.close()
        return out, count

    def signal_profile(self, windows: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, n_bins: int, agg, reverse=None,
                       index=None):
        """Every window row cut into ``n_bins`` bins as by ``depth_profile``, every bin a probe of ``overlap_wagg`` without
        thresholds (ivj_signal_profile_dev) -> one dict per column of ``agg``, name -> tensor (windows.n, n_bins) in HBM.
        ``reverse``: None or a bool / uint8 CUDA tensor of windows.n flags, a flagged row comes back right to left."""
        torch = self.torch
        n_bins = int(n_bins)
        opts = make_opts(strict, n_contigs)
        dev = windows.start.device
        rev = None
        if reverse is not None:
            rev = reverse.to(torch.uint8) if reverse.dtype == torch.bool else reverse
            if rev.dtype != torch.uint8 or tuple(rev.shape) != (windows.n,) or not rev.is_contiguous() or rev.device != dev:
                raise ValueError("reverse must be a contiguous bool / uint8 tensor of windows.n elements on the windows' device")
        cols, n_values = self._agg_columns(agg)
        results = self._agg_results(cols, (windows.n, max(n_bins, 0)), dev)
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, False) if own else index
        try:
            # (a tensor without elements has no address: the entry still checks n_bins, and refuses a NULL output only with rows)
            self.engine.signal_profile_dev(
                ix, windows.as_c(), rev.data_ptr() if rev is not None and windows.n else 0, n_bins, opts, n_values,
                [(v.data_ptr() if n_values else 0, (m.data_ptr() if m is not None and n_values else 0), dt, ops) for v, m, dt, ops in cols],
                [{name: (t.data_ptr() if t.numel() else 0) for name, t in r.items()} for r in results])
        finally:
            if own:
                ix.close()
        return results

    # ---- join kinds: semi / anti (include/ivjoin.h: ivj_overlap_select_dev) -------------------------------
    def overlap_select(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, mode, min_overlap: int = 0, probe_min=None,
                       build_min=None, index=None, out=None, partition_mode: int = 0):
        """Semi ("semi") / anti ("anti") join on tensors in HBM: the probe rows (``probe.row_id`` where given, else positions) with
        at least one / no build row under the predicate -- plain, or thresholded when min_overlap / probe_min / build_min are given
        (as in ``count_overlaps_thresh``) -> int32 tensor, ascending position order.  ``out``: optional preallocated int32 CUDA
        tensor, used when it holds the result (the filled slice comes back)."""
        torch = self.torch
        mode = select_mode(mode)
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        plain = not min_overlap and probe_min is None and build_min is None
        thr = None if plain else self._thresholds(probe, build, min_overlap, probe_min, build_min)
        if build.n == 0:
            plain, thr = True, None                            # every count is 0 under either predicate
        if probe.n == 0:
            return torch.empty(0, dtype=torch.int32, device=probe.start.device)
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, plain) if own else index
        try:
            side = probe.as_c()
            if out is not None:
                total, fits = self.engine.overlap_select_dev(ix, side, opts, thr, mode, out.data_ptr(), 0, out.numel())
                if fits:
                    return out[:total]
            else:
                total, _ = self.engine.overlap_select_dev(ix, side, opts, thr, mode, 0, 0, 0)
            rows = torch.empty(total, dtype=torch.int32, device=probe.start.device)
            if total:
                self.engine.overlap_select_dev(ix, side, opts, thr, mode, rows.data_ptr(), 0, total)
        finally:
            if own:
                ix.close()
        return rows

    # ---- sort-scan family ---------------------------------------------
    def coverage(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, index=None, out=None):
        """Covered positions of every probe row by the union of the build side -> int64 tensor."""
        torch = self.torch
        opts = make_opts(strict, n_contigs)
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, False) if own else index
        try:
            cov = out if out is not None else torch.empty(probe.n, dtype=torch.int64, device=probe.start.device)
            self.engine.coverage_dev(ix, probe.as_c(), opts, cov.data_ptr())
        finally:
            if own:
                ix.close()
        return cov

    def overlap_bases(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, index=None, out=None,
                      partition_mode: int = 0):
        """Positions every probe row shares with each build row of its contig, summed over the build rows (the integral of the
        build side's depth over the probe row) -> int64 tensor."""
        torch = self.torch
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, False) if own else index
        try:
            bases = out if out is not None else torch.empty(probe.n, dtype=torch.int64, device=probe.start.device)
            self.engine.overlap_bases_dev(ix, probe.as_c(), opts, bases.data_ptr())
        finally:
            if own:
                ix.close()
        return bases

    def depth_profile(self, windows: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, n_bins: int, reverse=None,
                      index=None, out=None):
        """Every window row cut into ``n_bins`` bins (edges S + floor(j L / n_bins) over the row's L positions), per bin the
        positions shared with each build row of the window's contig, summed -> int64 tensor (windows.n, n_bins) in HBM; a row
        sums to its ``overlap_bases``.  ``reverse``: None or a bool / uint8 CUDA tensor of windows.n flags, a flagged row comes
        back right to left.  ``index`` / ``out`` as in ``overlap_bases`` (``out``: contiguous int64 of that shape)."""
        torch = self.torch
        n_bins = int(n_bins)
        opts = make_opts(strict, n_contigs)
        dev = windows.start.device
        rev = None
        if reverse is not None:
            rev = reverse.to(torch.uint8) if reverse.dtype == torch.bool else reverse
            if rev.dtype != torch.uint8 or tuple(rev.shape) != (windows.n,) or not rev.is_contiguous() or rev.device != dev:
                raise ValueError("reverse must be a contiguous bool / uint8 tensor of windows.n elements on the windows' device")
        if out is not None and (out.dtype != torch.int64 or tuple(out.shape) != (windows.n, n_bins) or not out.is_contiguous()):
            raise ValueError("out must be a contiguous int64 tensor of shape (windows.n, n_bins)")
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, False) if own else index
        try:
            bases = out if out is not None else torch.empty((windows.n, max(n_bins, 0)), dtype=torch.int64, device=dev)
            # (a tensor without elements has no address: the entry still checks n_bins, and refuses a NULL output only with rows)
            self.engine.depth_profile_dev(ix, windows.as_c(), rev.data_ptr() if rev is not None and windows.n else 0, n_bins, opts,
                                          bases.data_ptr() if bases.numel() else 0)
        finally:
            if own:
                ix.close()
        return bases

    def depth_summary(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, thresholds=(1,), index=None,
                      out_max=None, out_bases=None, partition_mode: int = 0):
        """Per probe row the maximum depth of the build side under it and, per threshold T, its positions covered at least T deep
        -> (max_depth int32[n], bases_ge int64[K, n]) tensors in HBM, row k of bases_ge = thresholds[k].  ``index``: a prebuilt
        index of the build side (any form); ``out_max`` / ``out_bases``: caller buffers of those shapes (contiguous)."""
        torch = self.torch
        thresholds = [int(t) for t in thresholds]
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, True, sweep_only=True) if own else index
        try:
            dev = probe.start.device
            md = out_max if out_max is not None else torch.empty(probe.n, dtype=torch.int32, device=dev)
            bg = out_bases if out_bases is not None else torch.empty((len(thresholds), probe.n), dtype=torch.int64, device=dev)
            if md.dtype != torch.int32 or tuple(md.shape) != (probe.n,) or not md.is_contiguous():
                raise ValueError("out_max must be a contiguous int32 tensor of probe.n elements")
            if bg.dtype != torch.int64 or tuple(bg.shape) != (len(thresholds), probe.n) or not bg.is_contiguous():
                raise ValueError("out_bases must be a contiguous int64 tensor of shape (len(thresholds), probe.n)")
            if probe.n > 0:      # a tensor without elements has no address, and the entry refuses NULL outputs whatever the row count
                self.engine.depth_summary_dev(ix, probe.as_c(), opts, thresholds, md.data_ptr(), bg.data_ptr() if thresholds else 0)
        finally:
            if own:
                ix.close()
        return md, bg

    def depth_histogram(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, max_depth: int, index=None, out=None,
                        partition_mode: int = 0):
        """Per probe row the number of its positions at each depth 0 .. max_depth of the build side (the last bin: max_depth or
        more) -> int64 tensor (probe.n, max_depth + 1) in HBM; a row sums to its positions.  ``index``: a prebuilt index of the
        build side (any form); ``out``: a contiguous int64 tensor of that shape."""
        torch = self.torch
        max_depth = int(max_depth)
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        bins = max_depth + 1 if max_depth >= 0 else 0
        if out is not None and (out.dtype != torch.int64 or tuple(out.shape) != (probe.n, bins) or not out.is_contiguous()):
            raise ValueError("out must be a contiguous int64 tensor of shape (probe.n, max_depth + 1)")
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, True, sweep_only=True) if own else index
        try:
            hist = out if out is not None else torch.empty((probe.n, bins), dtype=torch.int64, device=probe.start.device)
            # (a tensor without elements has no address, and the entry refuses a NULL output whatever the row count)
            spare = hist if hist.numel() else torch.empty(1, dtype=torch.int64, device=probe.start.device)
            self.engine.depth_hist_dev(ix, probe.as_c(), opts, max_depth, spare.data_ptr())
        finally:
            if own:
                ix.close()
        return hist

    def depth_quantiles(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, ranks, index=None, out=None,
                        partition_mode: int = 0):
        """Per probe row and per rank the order statistic of the build side's depth over the row's positions: ``ranks`` is a
        contiguous int64 tensor (probe.n, K) in HBM, 0-based, K in 1 .. 16 -> int32 tensor (probe.n, K) in HBM; -1 for a rank
        outside the row's positions and for a row without a position.  ``index``: a prebuilt index of the build side (any form);
        ``out``: a contiguous int32 tensor of that shape."""
        torch = self.torch
        opts = make_opts(strict, n_contigs, partition_mode=partition_mode)
        if ranks.dtype != torch.int64 or ranks.dim() != 2 or ranks.shape[0] != probe.n or not ranks.is_contiguous():
            raise ValueError("ranks must be a contiguous int64 tensor of shape (probe.n, K)")
        k = int(ranks.shape[1])
        if out is not None and (out.dtype != torch.int32 or tuple(out.shape) != (probe.n, k) or not out.is_contiguous()):
            raise ValueError("out must be a contiguous int32 tensor of shape (probe.n, K)")
        own = index is None
        ix = self.engine.index_build_dev(build.as_c(), opts, True, sweep_only=True) if own else index
        try:
            dev = probe.start.device
            res = out if out is not None else torch.empty((probe.n, k), dtype=torch.int32, device=dev)
            # (a tensor without elements has no address, and the entry refuses a NULL pointer whatever the row count)
            spare_r = ranks if ranks.numel() else torch.zeros(1, dtype=torch.int64, device=dev)
            spare_o = res if res.numel() else torch.empty(1, dtype=torch.int32, device=dev)
            self.engine.depth_quantiles_dev(ix, probe.as_c(), opts, k, spare_r.data_ptr(), spare_o.data_ptr())
        finally:
            if own:
                ix.close()
        return res

    def depth_histogram_contigs(self, frame: DeviceSide, strict: bool, n_contigs: int, max_depth: int, index=None, out=None):
        """Per contig the number of positions at each depth 1 .. max_depth of the frame (the last bin: max_depth or more; bin 0 is
        0, the engine does not know a contig's length) -> int64 tensor (n_contigs, max_depth + 1) in HBM.  ``index`` / ``out`` as
        in ``depth_histogram``."""
        torch = self.torch
        max_depth = int(max_depth)
        opts = make_opts(strict, n_contigs)
        bins = max_depth + 1 if max_depth >= 0 else 0
        if out is not None and (out.dtype != torch.int64 or tuple(out.shape) != (int(n_contigs), bins) or not out.is_contiguous()):
            raise ValueError("out must be a contiguous int64 tensor of shape (n_contigs, max_depth + 1)")
        own = index is None
        ix = self.engine.index_build_dev(frame.as_c(), opts, True, sweep_only=True) if own else index
        try:
            dev = frame.start.device
            hist = out if out is not None else torch.empty((int(n_contigs), bins), dtype=torch.int64, device=dev)
            spare = hist if hist.numel() else torch.empty(1, dtype=torch.int64, device=dev)
            self.engine.depth_hist_contigs_dev(ix, opts, max_depth, spare.data_ptr())
        finally:
            if own:
                ix.close()
        return hist

    def merge(self, frame: DeviceSide, strict: bool, n_contigs: int, min_dist: int = 0, out=None, agg=None):
        """Merged intervals of one frame -> (contig, start, end int32, n_intervals int64) tensors.
        ``out``: optional preallocated 4-tuple (views of the first n_merged elements are returned).
        ``agg``: a list of (values, valid, ops) per value column -- values a contiguous int64 or float64 CUDA tensor indexed by
        the frame's rows (by ``row_id`` where the frame carries one), valid a contiguous bool / uint8 CUDA tensor of the same
        length or None, ops a name or list of names of "sum", "min", "max", "mean", "count" (or a mask of _engine.AGG_*).  The
        result is then the 4-tuple plus one list with a dict per column, name -> tensor of n_merged elements: sum int64
        (wrapped) / float64, min / max the column's type, mean float64, count int64; min / max / mean are unspecified where
        count is 0."""
        torch = self.torch
        opts = make_opts(strict, n_contigs)
        dev = frame.start.device
        cols, n_values = [], 0
        if agg is not None:
            agg = list(agg)
            for values, valid, ops in agg:
                if values.dtype not in (torch.int64, torch.float64) or not values.is_cuda or not values.is_contiguous() or values.dim() != 1:
                    raise ValueError("value columns must be contiguous 1-D int64 or float64 CUDA tensors")
                if valid is not None and (valid.dtype not in (torch.bool, torch.uint8) or not valid.is_cuda or not valid.is_contiguous()
                                          or valid.shape != values.shape):
                    raise ValueError("validity columns must be contiguous bool / uint8 CUDA tensors of the value column's length")
                cols.append((values, valid, AGG_I64 if values.dtype == torch.int64 else AGG_F64, agg_ops_mask(ops)))
            lengths = {int(v.shape[0]) for v, _, _, _ in cols}
            if len(lengths) > 1:
                raise ValueError(f"the value columns of one call must have one length, got {sorted(lengths)}")
            n_values = lengths.pop() if lengths else 0
        ix = self.engine.index_build_dev(frame.as_c(), opts, False, sweep_only=True)
        try:
            if out is None:
                out = tuple(torch.empty(frame.n, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int32, torch.int64))
            cap = min(int(t.numel()) for t in out)
            if agg is None:
                n, fits = self.engine.merge_dev(ix, opts, min_dist, cap, *(t.data_ptr() for t in out))
            else:
                kinds = {"sum": None, "min": None, "max": None, "mean": torch.float64, "count": torch.int64}
                results = [{name: torch.empty(cap, dtype=kinds[name] or values.dtype, device=dev) for name, bit in AGG_OPS.items() if ops & bit}
                           for values, _, _, ops in cols]
                n, fits = self.engine.merge_agg_dev(
                    ix, opts, min_dist, cap, *(t.data_ptr() for t in out), n_values,
                    [(v.data_ptr() if n_values else 0, (m.data_ptr() if m is not None and n_values else 0), dt, ops) for v, m, dt, ops in cols],
                    [{name: (t.data_ptr() if cap else 0) for name, t in r.items()} for r in results])
            if not fits:
                raise ValueError(f"merge output buffers hold fewer than {n} intervals")
        finally:
            ix.close()
        table = tuple(t[:n] for t in out)
        if agg is None:
            return table
        return (*table, [{name: t[:n] for name, t in r.items()} for r in results])

    def depth(self, frame: DeviceSide, strict: bool, n_contigs: int, out=None):
        """Blocks of constant coverage >= 1 of one frame -> (contig, start, end, depth) int32 tensors, (contig, start) order.
        ``out``: optional preallocated 4-tuple (views of the first n_blocks elements are returned); at most 2 * frame.n
        blocks exist."""
        torch = self.torch
        opts = make_opts(strict, n_contigs)
        ix = self.engine.index_build_dev(frame.as_c(), opts, True, sweep_only=True)
        try:
            if out is None:
                dev = frame.start.device
                out = tuple(torch.empty(2 * frame.n, dtype=torch.int32, device=dev) for _ in range(4))
            n, fits = self.engine.depth_dev(ix, opts, min(int(t.numel()) for t in out), *(t.data_ptr() for t in out))
            if not fits:
                raise ValueError(f"depth output buffers hold fewer than {n} blocks")
        finally:
            ix.close()
        return tuple(t[:n] for t in out)

    def _set_index(self, side: DeviceSide, opts):
        """sweep-only index with the end order of one side of a set operation; an empty side is the NULL index"""
        if side.n == 0:
            return DeviceIndex(self.engine, None, 0)
        return self.engine.index_build_dev(side.as_c(), opts, True, sweep_only=True)

    def setop(self, a: DeviceSide, b: DeviceSide, op, strict: bool, n_contigs: int, out=None):
        """Maximal runs of op(U(a), U(b)) -> (contig, start, end) int32 tensors, (contig, start) order.  ``op``: "intersection",
        "union", "difference" or "symmetric_difference".  ``out``: optional preallocated 3-tuple (views of the first
        n_regions elements are returned); at most a.n + b.n regions exist."""
        torch = self.torch
        opts = make_opts(strict, n_contigs)
        ix_a = self._set_index(a, opts)
        try:
            ix_b = self._set_index(b, opts)
            try:
                if out is None:
                    dev = a.start.device
                    out = tuple(torch.empty(a.n + b.n, dtype=torch.int32, device=dev) for _ in range(3))
                n, fits = self.engine.setop_dev(ix_a, ix_b, opts, op, min(int(t.numel()) for t in out), *(t.data_ptr() for t in out))
                if not fits:
                    raise ValueError(f"setop output buffers hold fewer than {n} regions")
            finally:
                ix_b.close()
        finally:
            ix_a.close()
        return tuple(t[:n] for t in out)

    def set_stats(self, a: DeviceSide, b: DeviceSide, strict: bool, n_contigs: int):
        """-> (only_a, only_b, both, n_intersections) as Python ints: the positions only U(a), only U(b), both cover, and the
        regions of the intersection, from one walk (what pb.jaccard needs)."""
        opts = make_opts(strict, n_contigs)
        ix_a = self._set_index(a, opts)
        try:
            ix_b = self._set_index(b, opts)
            try:
                return self.engine.set_stats_dev(ix_a, ix_b, opts)
            finally:
                ix_b.close()
        finally:
            ix_a.close()

    def multi_inter(self, frames, min_frames: int, strict: bool, n_contigs: int, consensus: bool = False, indexes=None, out=None):
        """N frames (a list of DeviceSide) as position sets.  ``consensus=False``: the maximal runs of positions covered by one set
        of at least ``min_frames`` frames -> (contig, start, end int32, mask int64) tensors, bit f of mask = frame f (the 64 bits
        of the engine's uint64 word: frame 63 is the sign bit; ``mask.cpu().numpy().view(numpy.uint64)`` reads them unsigned).
        ``consensus=True``: the maximal runs covered by at least ``min_frames`` frames -> (contig, start, end).  (contig, start)
        order.  ``indexes``: prebuilt indexes of the frames (None entries = empty frames); ``out``: optional preallocated tuple of
        those tensors (views of the first n elements are returned); at most twice the summed rows come back."""
        torch = self.torch
        frames = list(frames)
        mode = MULTI_CONSENSUS if consensus else MULTI_SEGMENTS
        min_frames = check_multi(len(frames), min_frames, mode)
        opts = make_opts(strict, n_contigs)
        own = indexes is None
        ixs = []
        try:
            if own:
                for side in frames:
                    ixs.append(self._set_index(side, opts) if side.n else None)
            else:
                ixs = list(indexes)
            if out is None:
                dev, cap = frames[0].start.device, 2 * sum(side.n for side in frames)
                out = tuple(torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
                if not consensus:
                    out += (torch.empty(cap, dtype=torch.int64, device=dev),)
            if len(out) != (3 if consensus else 4):
                raise ValueError("out must hold (contig, start, end) tensors, and the 8-byte mask tensor unless consensus")
            ptrs = [t.data_ptr() for t in out[:3]] + [out[3].data_ptr() if not consensus else 0]
            n, fits = self.engine.multi_inter_dev(ixs, opts, min_frames, mode, min(int(t.numel()) for t in out), *ptrs)
            if not fits:
                raise ValueError(f"multi_inter output buffers hold fewer than {n} regions")
        finally:
            if own:
                for ix in ixs:
                    if ix is not None:
                        ix.close()
        return tuple(t[:n] for t in out)

    def multi_pairwise(self, frames, strict: bool, n_contigs: int, indexes=None, out=None):
        """N frames (a list of DeviceSide) pair by pair -> (bases, runs), two (F, F) int64 CUDA tensors, symmetric: bases[i, j] =
        the positions frames i and j both cover (the diagonal: what frame i covers), runs[i, j] = the regions of their
        intersection (set_stats' n_intersections).  One walk over all frames; only the two matrices are written.  ``indexes``:
        prebuilt indexes of the frames (None entries = empty frames); ``out``: optional preallocated pair of contiguous int64
        tensors of F * F elements each (returned viewed as (F, F))."""
        torch = self.torch
        frames = list(frames)
        n_frames = len(frames)
        check_multi(n_frames, 1)
        opts = make_opts(strict, n_contigs)
        own = indexes is None
        ixs = []
        try:
            if own:
                for side in frames:
                    ixs.append(self._set_index(side, opts) if side.n else None)
            else:
                ixs = list(indexes)
                if len(ixs) != n_frames:
                    raise ValueError(f"indexes must hold one entry per frame: {n_frames} frames, {len(ixs)} indexes")
            if out is None:
                dev = frames[0].start.device
                out = tuple(torch.empty((n_frames, n_frames), dtype=torch.int64, device=dev) for _ in range(2))
            if len(out) != 2 or any(t.dtype != torch.int64 or t.numel() != n_frames * n_frames or not t.is_contiguous() for t in out):
                raise ValueError(f"out must hold two contiguous int64 tensors of {n_frames * n_frames} elements (bases, runs)")
            self.engine.multi_pairwise_dev(ixs, opts, out[0].data_ptr(), out[1].data_ptr())
        finally:
            if own:
                for ix in ixs:
                    if ix is not None:
                        ix.close()
        return tuple(t.view(n_frames, n_frames) for t in out)

    def subtract(self, left: DeviceSide, right: DeviceSide, strict: bool, n_contigs: int, index=None, out=None):
        """left minus the union of right -> (left row, start, end) int32 tensors of the remaining pieces."""
        torch = self.torch
        opts = make_opts(strict, n_contigs)
        own = index is None
        ix = self.engine.index_build_dev(right.as_c(), opts, False) if own else index
        try:
            if out is not None:
                n, fits = self.engine.subtract_dev(ix, left.as_c(), opts, min(int(t.numel()) for t in out), *(t.data_ptr() for t in out))
                if fits:
                    return tuple(t[:n] for t in out)
            else:
                n, _ = self.engine.subtract_dev(ix, left.as_c(), opts, 0, 0, 0, 0)
            out = tuple(torch.empty(n, dtype=torch.int32, device=left.start.device) for _ in range(3))
            n, fits = self.engine.subtract_dev(ix, left.as_c(), opts, n, *(t.data_ptr() for t in out))
        finally:
            if own:
                ix.close()
        return out

    def nearest(self, probe: DeviceSide, build: DeviceSide, strict: bool, n_contigs: int, k: int = 1,
                include_overlaps: bool = True, index=None, partition_mode: int = 0, nearest_ignore: int = 0):
        """nearest_ignore: direction mask (1: leave out the rows before the probe, 2: the rows after it), one per call."""
        torch = self.torch
        opts = make_opts(strict, n_contigs, k, include_overlaps, partition_mode=partition_mode, nearest_ignore=nearest_ignore)
        own = index is None
        general = not (k == 1 and include_overlaps)
        ix = self.engine.index_build_dev(build.as_c(), opts, general) if own else index
        try:
            dev = probe.start.device
            idx = torch.empty((probe.n, k), dtype=torch.int32, device=dev)
            dist = torch.empty((probe.n, k), dtype=torch.int64, device=dev)
            nf = torch.empty(probe.n, dtype=torch.int32, device=dev)
            self.engine.nearest_dev(ix, probe.as_c(), opts, idx.data_ptr(), dist.data_ptr(), nf.data_ptr())
        finally:
            if own:
                ix.close()
        return idx, dist, nf
