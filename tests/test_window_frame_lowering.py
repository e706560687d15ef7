"""CPU tests: lowering of explicit ROWS frames to the device frame model
(dask_sql_amd/physical/window_frames.py) — bounds, the can-be-empty
predicate, the static output dtype rule and the tile/prefix/host
thresholds. No GPU needed."""
import ctypes as ct
from pathlib import Path

import pytest

from dask_sql_amd.physical import window_frames as wf
from dask_sql_amd.planner.parser import parse_sql

REPO = Path(__file__).resolve().parent.parent
SO = REPO / "dask_sql_amd" / "libdsxhip.so"

UP = ("unbounded_preceding", None)
UF = ("unbounded_following", None)
CUR = ("current", 0)


def P(k):
    return ("preceding", k)


def F(k):
    return ("following", k)


def _window_frame(sql_over):
    """Frame tuple exactly as the SQL parser produces it."""
    stmt = parse_sql(f"SELECT SUM(x) OVER ({sql_over}) AS s FROM t")
    ast = stmt.items[0][0]
    assert ast[0] == "window"
    return ast[5]


@pytest.mark.parametrize("over, want", [
    ("ORDER BY o ROWS BETWEEN 2 PRECEDING AND CURRENT ROW", (-2, 0)),
    ("ORDER BY o ROWS 2 PRECEDING", (-2, 0)),
    ("ORDER BY o ROWS CURRENT ROW", (0, 0)),
    ("ORDER BY o ROWS UNBOUNDED PRECEDING", (None, 0)),
    ("ORDER BY o ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING", (-1, 1)),
    ("ORDER BY o ROWS BETWEEN 2 PRECEDING AND 1 PRECEDING", (-2, -1)),
    ("ORDER BY o ROWS BETWEEN 1 FOLLOWING AND 2 FOLLOWING", (1, 2)),
    ("ORDER BY o ROWS BETWEEN 1 FOLLOWING AND 1 PRECEDING", (1, -1)),
    ("ORDER BY o ROWS BETWEEN CURRENT ROW AND 3 FOLLOWING", (0, 3)),
    ("ORDER BY o ROWS BETWEEN CURRENT ROW AND CURRENT ROW", (0, 0)),
    ("ORDER BY o ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW",
     (None, 0)),
    ("ORDER BY o ROWS BETWEEN UNBOUNDED PRECEDING AND 2 FOLLOWING",
     (None, 2)),
    ("ORDER BY o ROWS BETWEEN UNBOUNDED PRECEDING AND 2 PRECEDING",
     (None, -2)),
    ("ORDER BY o ROWS BETWEEN 3 PRECEDING AND UNBOUNDED FOLLOWING",
     (-3, None)),
    ("ORDER BY o ROWS BETWEEN 3 FOLLOWING AND UNBOUNDED FOLLOWING",
     (3, None)),
    ("ORDER BY o ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING",
     (0, None)),
    ("ORDER BY o ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING",
     (None, None)),
])
def test_parser_frames_lower_to_offsets(over, want):
    frame = _window_frame(over)
    assert frame[0] == "rows"
    assert wf.frame_offsets(frame) == want
    low = wf.lower_rows_frame("sum", frame)
    assert (low.lo_off, low.hi_off) == want
    assert low.strategy in ("tile", "prefix")


def test_frames_outside_the_device_model_stay_on_host():
    # RANGE with offsets is rejected by the planner; the lowering still
    # refuses it, and the two bound placements the host path cannot express
    assert wf.frame_offsets(("range", P(2), CUR)) is None
    assert wf.lower_rows_frame("sum", ("range", P(2), CUR)).strategy == "host"
    assert wf.lower_rows_frame("sum", ("rows", UF, UF)).strategy == "host"
    assert wf.lower_rows_frame("sum", ("rows", UP, UP)).strategy == "host"
    for f in ("lag", "row_number", "rank", "stddev"):
        assert wf.lower_rows_frame(f, ("rows", P(2), CUR)).strategy == "host"


@pytest.mark.parametrize("lo, hi, empty", [
    (-2, 0, False), (-1, 1, False), (0, 0, False), (0, 3, False),
    (None, 0, False), (None, 2, False), (-3, None, False),
    (0, None, False), (None, None, False),
    (-2, -1, True), (1, 2, True), (1, -1, True), (None, -2, True),
    (3, None, True), (0, -1, True), (1, 0, True), (-300, -290, True),
])
def test_can_be_empty(lo, hi, empty):
    assert wf.frame_can_be_empty(lo, hi) is empty


def _brute_has_empty(lo, hi, plen):
    """Does some row of a plen-row partition get an empty frame?"""
    for i in range(plen):
        s = 0 if lo is None else max(0, i + lo)
        e = plen - 1 if hi is None else min(plen - 1, i + hi)
        if s > e:
            return True
    return False


def test_can_be_empty_matches_brute_force():
    offs = [None, -3, -1, 0, 1, 3]
    for lo in offs:
        for hi in offs:
            want = wf.frame_can_be_empty(lo, hi)
            for plen in (1, 2, 5):
                # the predicate is static: true means EVERY non-empty
                # partition has an empty-frame row, false means none has
                assert _brute_has_empty(lo, hi, plen) is want, (lo, hi, plen)


def test_dtype_rule():
    agg = ("sum", "count", "avg", "min", "max")
    # a frame that can be empty: every aggregate is f64 with validity
    for lo, hi in ((-2, -1), (1, 2), (1, -1)):
        for f in agg:
            for big in (True, False):
                for nullable in (True, False):
                    assert wf.frame_out_dtype(f, lo, hi, big, nullable) == \
                        ("f64", True)
    for lo, hi in ((-2, 0), (None, 0), (-3, None), (None, None)):
        for nullable in (True, False):
            for big in (True, False):
                assert wf.frame_out_dtype("count", lo, hi, big, nullable) == \
                    ("i64", False)
                assert wf.frame_out_dtype("avg", lo, hi, big, nullable) == \
                    ("f64", True)
        for f in ("sum", "min", "max"):
            assert wf.frame_out_dtype(f, lo, hi, True, False) == \
                ("i64", False)
            assert wf.frame_out_dtype(f, lo, hi, True, True) == ("f64", True)
            assert wf.frame_out_dtype(f, lo, hi, False, False) == \
                ("f64", True)
    for f in ("first_value", "last_value"):
        assert wf.frame_out_dtype(f, -2, 0, True, False) == ("value", True)
        assert wf.frame_out_dtype(f, 1, 2, False, True) == ("value", True)
    with pytest.raises(ValueError):
        wf.frame_out_dtype("lag", -2, 0, True, False)


def test_strategy_thresholds():
    d, t = wf.WIN_ROWS_DIRECT_MAXW, wf.WIN_ROWS_TILE_MAXW
    assert 1 <= d <= t
    for f in ("sum", "count", "avg"):
        assert wf.frame_strategy(f, -(d - 1), 0) == "tile"      # W = d
        assert wf.frame_strategy(f, -d, 0) == "prefix"          # W = d + 1
        assert wf.frame_strategy(f, -(d // 2), d - 1 - d // 2) == "tile"
        assert wf.frame_strategy(f, -10 * t, 10 * t) == "prefix"
        assert wf.frame_strategy(f, 1, -1) == "tile"            # W < 1
        assert wf.frame_strategy(f, -300, -290) == "tile"
    for f in ("min", "max"):
        assert wf.frame_strategy(f, -(t - 1), 0) == "tile"      # W = t
        assert wf.frame_strategy(f, -t, 0) == "host"            # W = t + 1
        assert wf.frame_strategy(f, -d, 0) == "tile"
        assert wf.frame_strategy(f, 1, -1) == "tile"
    for f in ("sum", "count", "avg", "min", "max"):
        for lo, hi in ((None, 0), (None, 2), (-3, None), (None, None),
                       (None, -2), (3, None)):
            assert wf.frame_strategy(f, lo, hi) == "prefix"
    for f in ("first_value", "last_value"):
        for lo, hi in ((-2, 0), (None, None), (-10 * t, 10 * t), (1, -1)):
            assert wf.frame_strategy(f, lo, hi) == "prefix"


def test_huge_offsets_stay_in_int64():
    low = wf.lower_rows_frame("sum", ("rows", P(10 ** 30), F(10 ** 30)))
    assert low.strategy == "prefix"
    assert -(1 << 62) < low.lo_off < 0 < low.hi_off < (1 << 62)


def test_thresholds_match_the_library():
    """The strategy constants are the ones the kernels were built with."""
    lib = ct.CDLL(str(SO))
    d, t = ct.c_int(), ct.c_int()
    assert lib.dsx_window_rows_limits(ct.byref(d), ct.byref(t)) == 0
    assert (d.value, t.value) == (wf.WIN_ROWS_DIRECT_MAXW,
                                  wf.WIN_ROWS_TILE_MAXW)
