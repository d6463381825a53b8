"""Join kinds (how = "left" / "semi" / "anti") without a GPU: the header declares the entries and constants, the ctypes binding
knows them under the same values, the front door validates ``how`` before any engine is touched, and the yardstick
(tests/_join_kinds_util.py) agrees with the committed golden tables."""
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _engine, range_op
import _join_kinds_util as J
from _util import GOLDEN, random_side

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ivj_overlap_select", "ivj_rowsel_free", "ivj_overlap_select_dev", "ivj_overlap_outer")
COLS = ("contig", "pos_start", "pos_end")


def _header():
    return open(os.path.join(ROOT, "include", "ivjoin.h")).read()


def test_header_declares_the_entries_and_constants():
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", code), name
    assert re.search(r"#define\s+IVJ_SELECT_SEMI\s+0\b", code) and re.search(r"#define\s+IVJ_SELECT_ANTI\s+1\b", code)
    assert re.search(r"typedef\s+struct\s*\{[^}]*int32_t\s*\*\s*rows\s*;[^}]*int64_t\s+n\s*;[^}]*\}\s*ivj_rowsel\s*;", code)
    assert re.search(r"#define\s+IVJ_ABI_VERSION\s+6\b", code), "new entries and a new struct do not change the ABI version"
    for word in ("semi", "anti", "left"):                  # the semantics are written down where the other sections are
        assert re.search(rf"\b{word}\b", hdr)


def test_binding_knows_the_entries_and_the_constants():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ENTRIES:
        assert name in _engine.ABI_SYMBOLS
    assert _engine.SELECT_SEMI == int(re.search(r"#define\s+IVJ_SELECT_SEMI\s+(\d+)", hdr).group(1))
    assert _engine.SELECT_ANTI == int(re.search(r"#define\s+IVJ_SELECT_ANTI\s+(\d+)", hdr).group(1))
    assert _engine.select_mode("semi") == _engine.SELECT_SEMI and _engine.select_mode("anti") == _engine.SELECT_ANTI
    assert _engine.select_mode(1) == _engine.SELECT_ANTI
    for bad in ("left", "inner", 2, -1, True):
        with pytest.raises(ValueError):
            _engine.select_mode(bad)
    assert [f[0] for f in _engine._RowSel._fields_] == ["rows", "n"]
    L = _engine.load_library()
    for name in ENTRIES:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for method in ("overlap_select", "overlap_outer", "overlap_select_dev"):
        assert callable(getattr(_engine.Engine, method))


def test_selection_tile_is_named_in_the_kernel_header():
    tile = J.kernel_tile()
    assert tile >= 256 and tile % 64 == 0


def _df(zero_based=True):
    df = pd.DataFrame({"chrom": ["chr1", "chr1"], "start": [1, 10], "end": [8, 20]})
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


@pytest.fixture
def no_engine(monkeypatch):
    def refuse():
        raise AssertionError("the engine was touched before the arguments were validated")
    monkeypatch.setattr(range_op, "default_engine", refuse)


def test_how_is_keyword_only_and_defaults_to_inner():
    p = inspect.signature(pb.overlap).parameters["how"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "inner"
    assert "how" not in inspect.signature(pb.overlap_batches).parameters


@pytest.mark.parametrize("how", ["outer", "right", "INNER", "", None, 1])
def test_unknown_how_is_a_value_error(no_engine, how):
    with pytest.raises(ValueError, match="how"):
        pb.overlap(_df(), _df(), output_type="pandas.DataFrame", how=how)


@pytest.mark.parametrize("kw", [dict(overlap_output="left"), dict(distinct_output=True), dict(overlap_output="left", distinct_output=True)])
@pytest.mark.parametrize("how", ["semi", "anti", "left"])
def test_non_inner_how_refuses_the_left_output_mode_and_distinct(no_engine, how, kw):
    with pytest.raises(ValueError, match="how"):
        pb.overlap(_df(), _df(), output_type="pandas.DataFrame", how=how, **kw)


def test_engine_without_join_kinds_is_a_clear_error(monkeypatch):
    class Plain:                                           # what a multi-device engine looks like to the front door
        pass
    monkeypatch.setattr(range_op, "default_engine", lambda: Plain())
    for how in ("semi", "anti", "left"):
        with pytest.raises(NotImplementedError, match="single-device engine"):
            pb.overlap(_df(), _df(), output_type="pandas.DataFrame", how=how)


def _golden_sides():
    reads, targets = pd.read_csv(f"{GOLDEN}/overlap/reads.csv"), pd.read_csv(f"{GOLDEN}/overlap/targets.csv")
    ids = {v: i for i, v in enumerate(sorted(set(reads[COLS[0]]) | set(targets[COLS[0]])))}
    side = lambda df: (df[COLS[0]].map(ids).to_numpy(np.int32), df[COLS[1]].to_numpy(np.int32), df[COLS[2]].to_numpy(np.int32))
    return reads, targets, side(reads), side(targets), len(ids)


def test_yardstick_on_the_golden_tables():
    """Semi of reads against targets = the distinct df1 rows of expected_overlap.csv; anti = the remaining rows (1-based frames)."""
    reads, targets, probe, build, nc = _golden_sides()
    exp = pd.read_csv(f"{GOLDEN}/expected_overlap.csv")
    want = exp[[c + "_1" for c in COLS]].drop_duplicates()
    want.columns = list(COLS)
    e = J.expected(probe, build, nc, False)
    semi, anti = reads.iloc[e["semi"]], reads.iloc[e["anti"]]
    key = lambda df: sorted(map(tuple, df[list(COLS)].itertuples(index=False)))
    assert key(semi) == key(want) and len(semi) == len(want) > 0
    assert sorted(np.concatenate([e["semi"], e["anti"]])) == list(range(len(reads)))
    assert not set(key(anti)) & set(key(want))
    assert len(e["inner"][0]) == len(exp) and len(e["left"][0]) == len(exp) + len(anti)
    assert (e["left"][1] == -1).sum() == len(anti)


@pytest.mark.parametrize("strict", [True, False])
def test_yardstick_ignores_contigs_outside_the_dictionary_and_agrees_between_predicates(strict):
    rng = np.random.default_rng(3)
    pc, ps, pe = random_side(rng, 600, 4, 3000, 100, zero_len_frac=0.0)
    bc, bs, be = random_side(rng, 500, 4, 3000, 150, zero_len_frac=0.0)
    pe, be = np.maximum(pe, ps + 1).astype(np.int32), np.maximum(be, bs + 1).astype(np.int32)     # every row covers a position
    pc[:20], bc[:20] = -1, -1
    pc[20:40], bc[20:40] = 7, 7                             # equal ids outside the dictionary never match
    plain = J.expected((pc, ps, pe), (bc, bs, be), 4, strict)
    thr = J.expected((pc, ps, pe), (bc, bs, be), 4, strict, min_overlap=1)
    assert not plain["cnt"][:40].any() and (plain["anti"][:40] == np.arange(40)).all()
    assert 0 < len(plain["semi"]) < 600
    for k in ("cnt", "semi", "anti"):
        assert (plain[k] == thr[k]).all(), k
    assert all((a == b).all() for a, b in zip(plain["left"], thr["left"]))
