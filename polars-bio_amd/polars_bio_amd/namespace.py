"""The ``.pb`` namespace on frames: ``df.pb.overlap(other, ...)`` = ``pb.overlap(df, other, ...)``.

The reference registers it on polars LazyFrames (/root/reference/polars_bio/polars_ext.py:9-97: pure aliasing of the
range operations).  Here one accessor class is generated from the table below and registered on every frame library that
is importable: polars LazyFrame / DataFrame (``pl.api.register_*_namespace``) and pandas DataFrame
(``pd.api.extensions.register_dataframe_accessor``); the default output kind follows the frame the call was made on.
Every keyword is passed through as given, the keyword-only ones included (``df.pb.overlap(other, min_frac1=0.5)``).
"""
from __future__ import annotations

from . import range_op

# method -> (function, takes a second frame); "frames": takes a list of further frames, the call is made on [this frame, *others]
_ALIASES = {
    "overlap": (range_op.overlap, True), "nearest": (range_op.nearest, True), "count_overlaps": (range_op.count_overlaps, True),
    "window": (range_op.window, True), "count_window": (range_op.count_window, True),
    "coverage": (range_op.coverage, True), "mean_depth": (range_op.mean_depth, True), "depth_summary": (range_op.depth_summary, True),
    "depth_profile": (range_op.depth_profile, True), "depth_histogram": (range_op.depth_histogram, True),
    "depth_quantiles": (range_op.depth_quantiles, True), "median_depth": (range_op.median_depth, True),
    "subtract": (range_op.subtract, True), "map_overlaps": (range_op.map_overlaps, True),
    "map_quantiles": (range_op.map_quantiles, True), "map_median": (range_op.map_median, True),
    "signal_summary": (range_op.signal_summary, True), "signal_profile": (range_op.signal_profile, True),
    "permutation_test": (range_op.permutation_test, True),
    "merge": (range_op.merge, False), "depth": (range_op.depth, False), "genome_depth_histogram": (range_op.genome_depth_histogram, False), "cluster": (range_op.cluster, False), "complement": (range_op.complement, False),
    "set_intersect": (range_op.set_intersect, True), "set_union": (range_op.set_union, True), "set_difference": (range_op.set_difference, True),
    "set_symmetric_difference": (range_op.set_symmetric_difference, True), "jaccard": (range_op.jaccard, True),
    "multi_intersect": (range_op.multi_intersect, "frames"), "consensus": (range_op.consensus, "frames"),
    "pairwise_jaccard": (range_op.pairwise_jaccard, "frames"),
}


def _make_accessor(default_output: str):
    class RangeNamespace:
        __doc__ = "Range operations of polars_bio_amd as methods of the frame (aliases of pb.<operation>)."

        def __init__(self, frame):
            self._frame = frame

    def bind(name, fn, binary):
        if binary == "frames":
            def method(self, other_dfs, *args, **kwargs):
                kwargs.setdefault("output_type", default_output)
                if isinstance(other_dfs, (str, bytes)) or not isinstance(other_dfs, (list, tuple)):
                    raise ValueError("the other frames must be given as a list")
                return fn([self._frame, *other_dfs], *args, **kwargs)
        elif binary:
            def method(self, other_df, **kwargs):
                kwargs.setdefault("output_type", default_output)
                return fn(self._frame, other_df, **kwargs)
        else:
            def method(self, **kwargs):
                kwargs.setdefault("output_type", default_output)
                return fn(self._frame, **kwargs)
        method.__name__ = name
        what = "as frame 0 of [this frame, *other_dfs]" if binary == "frames" else "as the first argument"
        method.__doc__ = f"Alias of pb.{name} with this frame {what}.\n\n{fn.__doc__ or ''}"
        return method

    for name, (fn, binary) in _ALIASES.items():
        setattr(RangeNamespace, name, bind(name, fn, binary))
    return RangeNamespace


registered = []
try:
    import polars as _pl
    _pl.api.register_lazyframe_namespace("pb")(_make_accessor("polars.LazyFrame"))
    _pl.api.register_dataframe_namespace("pb")(_make_accessor("polars.DataFrame"))
    registered += ["polars.LazyFrame", "polars.DataFrame"]
except ImportError:
    pass
try:
    import pandas as _pd
    _pd.api.extensions.register_dataframe_accessor("pb")(_make_accessor("pandas.DataFrame"))
    registered.append("pandas.DataFrame")
except ImportError:
    pass
