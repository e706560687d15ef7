"""CPU tests: RANGE window frames with value offsets — what the parser and
the builder accept and refuse, the offset units, the output dtype rule, and
the numpy host model (dask_sql_amd/physical/window_range.py) against the
in-process sqlite3. No GPU needed."""
import numpy as np
import pandas as pd
import pytest

from dask_sql_amd.physical import window_range as wrg
from dask_sql_amd.planner import range_frame as rf
from dask_sql_amd.planner.builder import Builder, Catalog
from dask_sql_amd.planner.parser import parse_sql
from tests import range_oracle as ro
from tests.range_oracle import CUR, OFF, UNB

DAY_NS = 86_400_000_000_000


# ---- parser and builder -------------------------------------------------------
def _catalog():
    cat = Catalog()
    cat.add("t", [("p", "BIGINT"), ("t", "BIGINT"), ("i", "INTEGER"),
                  ("x", "BIGINT"), ("f", "DOUBLE"), ("g", "FLOAT"),
                  ("d", "DATE"), ("ts", "TIMESTAMP"), ("s", "VARCHAR")])
    return cat


def _spec(over, func="SUM(x)"):
    plan = Builder(_catalog()).build(
        f"SELECT {func} OVER ({over}) AS w FROM t")
    found = []

    def walk(p):
        if p.get_current_node_type() == "Window":
            found.extend(p.window().getWindowSpecs())
        for c in p.get_inputs():
            walk(c)

    walk(plan)
    assert len(found) == 1
    return found[0]


ACCEPTED = [
    ("PARTITION BY p ORDER BY t RANGE BETWEEN 7 PRECEDING AND CURRENT ROW",
     ("range", ("preceding", 7), ("current", 0))),
    ("ORDER BY t RANGE 7 PRECEDING",
     ("range", ("preceding", 7), ("current", 0))),
    ("ORDER BY t RANGE BETWEEN 3 PRECEDING AND 2 FOLLOWING",
     ("range", ("preceding", 3), ("following", 2))),
    ("ORDER BY t RANGE BETWEEN 2 FOLLOWING AND 9 FOLLOWING",
     ("range", ("following", 2), ("following", 9))),
    ("ORDER BY t RANGE BETWEEN 2 PRECEDING AND 5 PRECEDING",
     ("range", ("preceding", 2), ("preceding", 5))),
    ("ORDER BY t RANGE BETWEEN UNBOUNDED PRECEDING AND 2 FOLLOWING",
     ("range", ("unbounded_preceding", None), ("following", 2))),
    ("ORDER BY t RANGE BETWEEN 0 PRECEDING AND UNBOUNDED FOLLOWING",
     ("range", ("preceding", 0), ("unbounded_following", None))),
    ("ORDER BY t RANGE BETWEEN CURRENT ROW AND CURRENT ROW",
     ("range", ("current", 0), ("current", 0))),
    ("ORDER BY t RANGE BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING",
     ("range", ("unbounded_preceding", None), ("unbounded_following", None))),
    # a decimal literal is floored on an integer key
    ("ORDER BY t RANGE BETWEEN 2.75 PRECEDING AND CURRENT ROW",
     ("range", ("preceding", 2), ("current", 0))),
    ("ORDER BY i DESC RANGE BETWEEN 1 PRECEDING AND 1 FOLLOWING",
     ("range", ("preceding", 1), ("following", 1))),
    ("ORDER BY t DESC NULLS FIRST RANGE BETWEEN 3 PRECEDING AND CURRENT ROW",
     ("range", ("preceding", 3), ("current", 0))),
    ("ORDER BY f RANGE BETWEEN 1.5 PRECEDING AND 2 FOLLOWING",
     ("range", ("preceding", 1.5), ("following", 2.0))),
    ("ORDER BY g NULLS FIRST RANGE BETWEEN 0.25 PRECEDING AND CURRENT ROW",
     ("range", ("preceding", 0.25), ("current", 0))),
    ("ORDER BY d RANGE BETWEEN INTERVAL '30' DAY PRECEDING AND CURRENT ROW",
     ("range", ("preceding", 30), ("current", 0))),
    ("ORDER BY d RANGE BETWEEN INTERVAL '2' WEEK PRECEDING AND 3 FOLLOWING",
     ("range", ("preceding", 14), ("following", 3))),
    ("ORDER BY d RANGE BETWEEN INTERVAL '7 days' PRECEDING AND CURRENT ROW",
     ("range", ("preceding", 7), ("current", 0))),
    ("ORDER BY ts RANGE BETWEEN INTERVAL '90' MINUTE PRECEDING AND "
     "INTERVAL '1' DAY FOLLOWING",
     ("range", ("preceding", 90 * 60 * 10**9), ("following", DAY_NS))),
    ("ORDER BY ts RANGE BETWEEN INTERVAL '1' WEEK PRECEDING AND "
     "INTERVAL '5' MILLISECOND FOLLOWING",
     ("range", ("preceding", 7 * DAY_NS), ("following", 5_000_000))),
    # peer-only frames take any number of order keys
    ("ORDER BY t, i DESC RANGE BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING",
     ("range", ("current", 0), ("unbounded_following", None))),
    ("ORDER BY s, t RANGE BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED "
     "FOLLOWING",
     ("range", ("unbounded_preceding", None), ("unbounded_following", None))),
]


@pytest.mark.parametrize("over, want", ACCEPTED)
def test_accepted_spellings_plan(over, want):
    spec = _spec(over)
    assert spec.frame == want
    for got_b, want_b in zip(spec.frame[1:], want[1:]):
        # 2 == 2.0: an integer key's offset must really be an int
        assert type(got_b[1]) is type(want_b[1])
    lo, hi = wrg.frame_bounds(spec.frame)
    assert lo.kind in (wrg.UNBOUNDED, wrg.CURRENT, wrg.OFFSET)
    if spec.frame[1][0] == "preceding":
        assert lo == wrg.RangeBound(wrg.OFFSET, -want[1][1])
    if spec.frame[2][0] == "following":
        assert hi == wrg.RangeBound(wrg.OFFSET, want[2][1])


@pytest.mark.parametrize("func", ["SUM(x)", "COUNT(x)", "COUNT(*)", "AVG(x)",
                                  "MIN(x)", "MAX(x)", "FIRST_VALUE(x)",
                                  "LAST_VALUE(x)"])
def test_every_function_plans(func):
    spec = _spec("ORDER BY t RANGE BETWEEN 7 PRECEDING AND 1 FOLLOWING", func)
    assert spec.frame[0] == "range"


def test_order_flags_reach_the_spec():
    spec = _spec("ORDER BY t DESC NULLS FIRST RANGE 3 PRECEDING")
    assert spec.order_idx[0][1] is True
    assert spec.order_nf == [True]


def test_default_frame_spelling_still_folds():
    spec = _spec("ORDER BY t RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT "
                 "ROW")
    assert spec.frame is None
    spec = _spec("ORDER BY t RANGE UNBOUNDED PRECEDING")
    assert spec.frame is None


REFUSED = [
    # a low bound of a later kind than the high bound
    ("ORDER BY t RANGE BETWEEN 2 FOLLOWING AND CURRENT ROW", ValueError),
    ("ORDER BY t RANGE BETWEEN CURRENT ROW AND 2 PRECEDING", ValueError),
    ("ORDER BY t RANGE BETWEEN 2 FOLLOWING AND 1 PRECEDING", ValueError),
    ("ORDER BY t RANGE BETWEEN UNBOUNDED FOLLOWING AND UNBOUNDED FOLLOWING",
     ValueError),
    ("ORDER BY t RANGE BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED PRECEDING",
     ValueError),
    ("ORDER BY t RANGE BETWEEN -1 PRECEDING AND CURRENT ROW", ValueError),
    ("ORDER BY f RANGE BETWEEN CURRENT ROW AND -0.5 FOLLOWING", ValueError),
    ("ORDER BY d RANGE BETWEEN INTERVAL '-3' DAY PRECEDING AND CURRENT ROW",
     ValueError),
    # an offset needs exactly one order key
    ("ORDER BY t, i RANGE BETWEEN 1 PRECEDING AND CURRENT ROW", ValueError),
    ("PARTITION BY p RANGE BETWEEN 1 PRECEDING AND CURRENT ROW", ValueError),
    # units
    ("ORDER BY d RANGE BETWEEN INTERVAL '1' MONTH PRECEDING AND CURRENT ROW",
     NotImplementedError),
    ("ORDER BY ts RANGE BETWEEN INTERVAL '1' YEAR PRECEDING AND CURRENT ROW",
     NotImplementedError),
    ("ORDER BY d RANGE BETWEEN INTERVAL '2' HOUR PRECEDING AND CURRENT ROW",
     NotImplementedError),
    ("ORDER BY ts RANGE BETWEEN 5 PRECEDING AND CURRENT ROW",
     NotImplementedError),
]


@pytest.mark.parametrize("over, exc", REFUSED)
def test_refusals(over, exc):
    with pytest.raises(exc):
        _spec(over)


@pytest.mark.parametrize("over, unit", [
    ("ORDER BY d RANGE INTERVAL '1' MONTH PRECEDING", "MONTH"),
    ("ORDER BY ts RANGE INTERVAL '1' YEAR PRECEDING", "YEAR"),
    ("ORDER BY d RANGE INTERVAL '2' HOUR PRECEDING", "HOUR"),
])
def test_unit_refusals_name_the_unit(over, unit):
    with pytest.raises(NotImplementedError, match=unit):
        _spec(over)


@pytest.mark.parametrize("func", ["RANK()", "ROW_NUMBER()", "LAG(x)"])
def test_other_functions_keep_the_existing_error(func):
    with pytest.raises(NotImplementedError, match="RANGE frames"):
        _spec("ORDER BY t RANGE BETWEEN 1 PRECEDING AND CURRENT ROW", func)


def test_rows_frames_keep_integers_only():
    with pytest.raises(ValueError):
        parse_sql("SELECT SUM(x) OVER (ORDER BY t ROWS BETWEEN 1.5 PRECEDING "
                  "AND CURRENT ROW) FROM t")
    with pytest.raises(ValueError):
        parse_sql("SELECT SUM(x) OVER (ORDER BY t ROWS BETWEEN INTERVAL '1' "
                  "DAY PRECEDING AND CURRENT ROW) FROM t")


# ---- the dtype rule and small helpers -----------------------------------------
def _b(x):
    if x is None:
        return wrg.RangeBound(wrg.UNBOUNDED, 0)
    if x == "cur":
        return wrg.RangeBound(wrg.CURRENT, 0)
    return wrg.RangeBound(wrg.OFFSET, x)


@pytest.mark.parametrize("lo, hi, empty", [
    (-7, "cur", False), (-7, 2, False), ("cur", 2, False), (None, 2, False),
    (-7, None, False), (0, 0, False), ("cur", "cur", False),
    (None, None, False), (2, 9, True), (-7, -3, True), (-2, -5, True),
    (None, -1, True), (1, None, True), (0.5, 2.0, True), (-0.5, 0.0, False),
])
def test_can_be_empty(lo, hi, empty):
    assert wrg.range_can_be_empty(_b(lo), _b(hi)) is empty


def test_dtype_rule():
    lo, hi = _b(-7), _b("cur")
    gap_lo, gap_hi = _b(2), _b(9)
    assert wrg.range_out_dtype("count", lo, hi, True, True) == ("i64", False)
    # COUNT over an empty frame is 0, so it needs no validity either
    assert wrg.range_out_dtype("count", gap_lo, gap_hi, True, True) == \
        ("i64", False)
    for f in ("sum", "min", "max"):
        assert wrg.range_out_dtype(f, lo, hi, True, False) == ("i64", False)
        assert wrg.range_out_dtype(f, lo, hi, True, True) == ("f64", True)
        assert wrg.range_out_dtype(f, lo, hi, False, False) == ("f64", True)
        assert wrg.range_out_dtype(f, gap_lo, gap_hi, True, False) == \
            ("f64", True)
    assert wrg.range_out_dtype("avg", lo, hi, True, False) == ("f64", True)
    for f in ("first_value", "last_value"):
        assert wrg.range_out_dtype(f, lo, hi, True, False) == ("value", True)
    with pytest.raises(ValueError):
        wrg.range_out_dtype("rank", lo, hi, True, False)


def test_sat_add():
    k = np.array([wrg.INT64_MAX, wrg.INT64_MAX - 5, 0, wrg.INT64_MIN + 5,
                  wrg.INT64_MIN], dtype=np.int64)
    assert wrg.sat_add(k, 10).tolist() == [
        wrg.INT64_MAX, wrg.INT64_MAX, 10, wrg.INT64_MIN + 15,
        wrg.INT64_MIN + 10]
    assert wrg.sat_add(k, -10).tolist() == [
        wrg.INT64_MAX - 10, wrg.INT64_MAX - 15, -10, wrg.INT64_MIN,
        wrg.INT64_MIN]
    assert wrg.sat_add(k, wrg.INT64_MAX).tolist() == [
        wrg.INT64_MAX, wrg.INT64_MAX, wrg.INT64_MAX, 4, -1]


def test_sat_overflow():
    k = np.array([wrg.INT64_MAX, wrg.INT64_MAX - 5, 0, wrg.INT64_MIN + 5,
                  wrg.INT64_MIN], dtype=np.int64)
    assert wrg.sat_overflow(k, 5).tolist() == [1, 0, 0, 0, 0]
    assert wrg.sat_overflow(k, 6).tolist() == [1, 1, 0, 0, 0]
    assert wrg.sat_overflow(k, -5).tolist() == [0, 0, 0, 0, -1]
    assert wrg.sat_overflow(k, -6).tolist() == [0, 0, 0, -1, -1]
    assert wrg.sat_overflow(k, 0).tolist() == [0] * 5


def test_table_bytes():
    # 5 000 rows: 79 blocks, 7 levels
    assert wrg.rmq_table_bytes(5000) == 8 * 79 * 7
    assert wrg.rmq_table_bytes(1) == 8
    assert wrg.rmq_table_bytes(64 * 64) == 8 * 64 * 7
    assert wrg.rmq_table_bytes(64 * 63) == 8 * 63 * 6


# ---- host model against sqlite --------------------------------------------------
N = 400


def _peer_value(p, o, mod):
    """A value that is a function of (partition, key), NULL for some pairs:
    FIRST/LAST do not depend on the order among peers."""
    h = (np.where(np.isnan(p), 97.0, p) * 31
         + np.where(np.isnan(o), 53.0, o * 4) * 7).astype(np.int64)
    w = pd.array(h % 1000 - 500, dtype="Int64")
    w[h % mod == 0] = pd.NA
    return w


@pytest.fixture(scope="module")
def int_table():
    rng = np.random.default_rng(20241021)
    p = rng.integers(0, 5, N).astype(np.float64)
    o = rng.integers(0, 40, N).astype(np.float64)      # duplicate keys
    o[rng.random(N) < 0.10] = np.nan
    v = pd.array(rng.integers(-1000, 1000, N), dtype="Int64")
    v[rng.random(N) < 0.15] = pd.NA
    df = pd.DataFrame({"rid": np.arange(N, dtype=np.int64),
                       "p": pd.array(p.astype(np.int64), dtype="Int64"),
                       "o": pd.array(np.where(np.isnan(o), 0, o)
                                     .astype(np.int64), dtype="Int64"),
                       "v": v, "w": _peer_value(p, o, 7)})
    df.loc[np.isnan(o), "o"] = pd.NA
    return df, ro.SqliteTable("t", df)


def _np_col(s, dtype):
    valid = s.notna().to_numpy()
    arr = s.fillna(0).to_numpy(dtype=dtype)
    return arr, valid


def _bound(b):
    if b[0] == "unb":
        return wrg.RangeBound(wrg.UNBOUNDED, 0)
    if b[0] == "cur":
        return wrg.RangeBound(wrg.CURRENT, 0)
    return wrg.RangeBound(wrg.OFFSET, b[1])


_HOST_FUNC = {"sum": ("sum", "v"), "count": ("count", "v"),
              "countstar": ("count", None), "avg": ("avg", "v"),
              "min": ("min", "v"), "max": ("max", "v"),
              "first": ("first_value", "w"), "last": ("last_value", "w")}
FUNCS = ("sum", "count", "countstar", "avg", "min", "max", "first", "last")


def _host(df, f, lo, hi, desc, nulls_first, key_dtype=np.int64, key=None):
    func, col = _HOST_FUNC[f]
    pid = wrg.dense_ids([_np_col(df["p"], np.int64)])
    k, kv = key if key is not None else _np_col(df["o"], key_dtype)
    value = valid = None
    if col is not None:
        value, valid = _np_col(df[col], np.int64)
    kind = "value" if func in wrg.RANGE_POSITIONAL else "f64"
    out, ok = wrg.range_frames_host(func, pid, [(k, kv, desc, nulls_first)],
                                    value, valid, _bound(lo), _bound(hi),
                                    kind)
    return np.where(ok.astype(bool), out.astype(np.float64), np.nan)


SIDE = [UNB, CUR, OFF(-7), OFF(-3), OFF(0), OFF(2), OFF(9)]
FRAMES = [(lo, hi) for lo in SIDE for hi in SIDE if ro.legal(lo, hi)]


def test_frame_cross_is_the_legal_subset():
    # 49 pairs minus CURRENT..PRECEDING (2) and FOLLOWING..CURRENT/PRECEDING
    # (2 x 3)
    assert len(FRAMES) == 49 - 2 - 6


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
def test_host_model_matches_sqlite(int_table, desc, nulls_first):
    df, lite = int_table
    for lo, hi in FRAMES:
        want = lite.run(FUNCS, ro.over_sql(lo, hi, desc, nulls_first))
        for f in FUNCS:
            got = _host(df, f, lo, hi, desc, nulls_first)
            ro.assert_same(got, want[f],
                           f"{f} {ro.frame_sql(lo, hi)} desc={desc} "
                           f"nulls_first={nulls_first}")


def test_avg_is_sum_over_count(int_table):
    df, lite = int_table
    lo, hi = OFF(-7), OFF(2)
    want = lite.run(("avg",), ro.over_sql(lo, hi))["avg"]
    got = _host(df, "avg", lo, hi, False, False)
    assert (np.isnan(got) == np.isnan(want)).all()
    ok = ~np.isnan(want)
    # both divide an exact integer sum by the count
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-15)


def test_int64_output_kind(int_table):
    df, _lite = int_table
    pid = wrg.dense_ids([_np_col(df["p"], np.int64)])
    k, kv = _np_col(df["o"], np.int64)
    value = df["rid"].to_numpy()
    out, ok = wrg.range_frames_host(
        "sum", pid, [(k, kv, False, False)], value, None,
        wrg.RangeBound(wrg.OFFSET, -7), wrg.RangeBound(wrg.CURRENT, 0), "i64")
    assert ok is None and out.dtype == np.int64
    ref, rok = wrg.range_frames_host(
        "sum", pid, [(k, kv, False, False)], value, None,
        wrg.RangeBound(wrg.OFFSET, -7), wrg.RangeBound(wrg.CURRENT, 0), "f64")
    assert rok.all() and (out == ref).all()
    cnt, cok = wrg.range_frames_host(
        "count", pid, [(k, kv, False, False)], None, None,
        wrg.RangeBound(wrg.OFFSET, 2), wrg.RangeBound(wrg.OFFSET, 9), "i64")
    assert cok is None and cnt.dtype == np.int64 and (cnt == 0).any()


def test_float_keys(int_table):
    """REAL keys in quarter steps with a 1.5 offset (exact in binary), -0.0
    next to +0.0, and NaN keys, which count as NULL."""
    df, _ = int_table
    rng = np.random.default_rng(7)
    o = rng.integers(-20, 20, N) / 4.0
    o[o == 0.0] = np.where(rng.random((o == 0.0).sum()) < 0.5, -0.0, 0.0)
    o[rng.random(N) < 0.1] = np.nan
    fdf = df.copy()
    fdf["o"] = o
    fdf["w"] = _peer_value(df["p"].to_numpy(dtype=np.float64), o, 5)
    lite = ro.SqliteTable("tf", fdf)
    key = (o, None)
    for lo, hi in [(OFF(-1.5), CUR), (OFF(-1.5), OFF(1.5)), (CUR, OFF(1.5)),
                   (OFF(0.25), OFF(1.5)), (UNB, OFF(-1.5)),
                   (OFF(-1.5), UNB)]:
        for desc in (False, True):
            for nf in (False, True):
                want = lite.run(FUNCS, ro.over_sql(lo, hi, desc, nf))
                for f in FUNCS:
                    got = _host(fdf, f, lo, hi, desc, nf, key=key)
                    ro.assert_same(got, want[f],
                                   f"float {f} {ro.frame_sql(lo, hi)} "
                                   f"desc={desc} nf={nf}")


def test_date_and_timestamp_keys(int_table):
    """DATE keys are int32 days, TIMESTAMP keys int64 nanoseconds: sqlite
    gets the integers, the model the resolved offsets."""
    df, _ = int_table
    rng = np.random.default_rng(11)
    days = (19_000 + rng.integers(0, 60, N)).astype(np.int32)
    ns = (1_700_000_000 * 10**9
          + rng.integers(0, 500, N) * 60 * 10**9).astype(np.int64)
    valid = rng.random(N) >= 0.1
    for arr, off in ((days, rf.resolve_offset(("interval", 1, "WEEK"),
                                               "DATE")),
                     (ns, rf.resolve_offset(("interval", 90, "MINUTE"),
                                             "TIMESTAMP"))):
        kdf = df.copy()
        kdf["o"] = pd.array(arr.astype(np.int64), dtype="Int64")
        kdf.loc[~valid, "o"] = pd.NA
        kdf["w"] = _peer_value(df["p"].to_numpy(dtype=np.float64),
                               np.where(valid, arr % 1000, np.nan), 5)
        lite = ro.SqliteTable("tk", kdf)
        for lo, hi in [(OFF(-off), CUR), (OFF(-off), OFF(off))]:
            for desc in (False, True):
                want = lite.run(FUNCS, ro.over_sql(lo, hi, desc, False))
                for f in FUNCS:
                    got = _host(kdf, f, lo, hi, desc, False,
                                key=(arr, valid))
                    ro.assert_same(got, want[f], f"{arr.dtype} {f}")
    assert rf.resolve_offset(("interval", 1, "WEEK"), "DATE") == 7
    assert rf.resolve_offset(("interval", 90, "MINUTE"), "TIMESTAMP") == \
        90 * 60 * 10**9


def test_two_keys_peer_frames(int_table):
    df, _ = int_table
    rng = np.random.default_rng(3)
    o2 = pd.array(rng.integers(0, 3, N), dtype="Int64")
    o2[rng.random(N) < 0.1] = pd.NA
    kdf = df.copy()
    kdf["o2"] = o2
    lite = ro.SqliteTable("t2", kdf)
    pid = wrg.dense_ids([_np_col(kdf["p"], np.int64)])
    order = [_np_col(kdf["o"], np.int64) + (False, False),
             _np_col(kdf["o2"], np.int64) + (True, False)]
    value, valid = _np_col(kdf["v"], np.int64)
    for lo, hi in [(CUR, UNB), (UNB, CUR), (CUR, CUR), (UNB, UNB)]:
        over = ("PARTITION BY p ORDER BY o NULLS LAST, o2 DESC NULLS LAST "
                + ro.frame_sql(lo, hi))
        want = lite.run(("sum", "count", "min", "max"), over)
        for f in ("sum", "count", "min", "max"):
            out, ok = wrg.range_frames_host(f, pid, order, value, valid,
                                            _bound(lo), _bound(hi), "f64")
            ro.assert_same(np.where(ok.astype(bool), out, np.nan), want[f],
                           f"two keys {f} {ro.frame_sql(lo, hi)}")
    with pytest.raises(ValueError):
        wrg.range_frames_host("sum", pid, order, value, valid,
                              _bound(OFF(-1)), _bound(CUR), "f64")


def test_empty_and_single_row():
    z = np.zeros(0, dtype=np.int64)
    out, ok = wrg.range_frames_host(
        "sum", z, [(z, None, False, False)], z, None,
        wrg.RangeBound(wrg.OFFSET, -1), wrg.RangeBound(wrg.CURRENT, 0), "f64")
    assert len(out) == 0 and len(ok) == 0
    one = np.array([5], dtype=np.int64)
    out, ok = wrg.range_frames_host(
        "max", np.zeros(1, dtype=np.int64), [(one, None, True, False)], one,
        None, wrg.RangeBound(wrg.OFFSET, -1), wrg.RangeBound(wrg.OFFSET, 1),
        "f64")
    assert out.tolist() == [5.0] and ok.tolist() == [1]


def _brute(df, lo, hi, desc):
    """The inclusion rule lo <= d * (key[j] - k) <= hi in exact Python
    integers (no NULL keys here) → sum, count, countstar, min, max."""
    d = -1 if desc else 1
    o = [int(x) for x in df["o"]]
    pp = df["p"].to_numpy(dtype=np.int64)
    v = df["v"]
    out = {f: np.full(len(df), np.nan) for f in
           ("sum", "count", "countstar", "min", "max")}
    for i in range(len(df)):
        rows = [j for j in range(len(df)) if pp[j] == pp[i]
                and (lo[0] == "unb" or d * (o[j] - o[i]) >= lo[1])
                and (hi[0] == "unb" or d * (o[j] - o[i]) <= hi[1])]
        vals = [int(v[j]) for j in rows if not pd.isna(v[j])]
        out["countstar"][i] = len(rows)
        out["count"][i] = len(vals)
        if vals:
            out["sum"][i] = sum(vals)
            out["min"][i] = min(vals)
            out["max"][i] = max(vals)
    return out


@pytest.mark.parametrize("near_max", [True, False])
def test_offsets_past_the_int64_limits(near_max):
    """Keys at and next to an int64 limit. A target beyond the limit admits
    every key on one side (100 PRECEDING .. 100 FOLLOWING) and none on the
    other: `5 FOLLOWING AND 100 FOLLOWING` of INT64_MAX - 2 must not frame
    the rows whose key IS INT64_MAX, which a saturated target alone would
    tie with. The reference is the issue's inclusion rule evaluated in exact
    Python integers. sqlite is compared near INT64_MAX only: it promotes an
    overflowing target to REAL, where INT64_MAX + 3 becomes 2^63 and still
    excludes every key, but INT64_MIN - 3 rounds to -2^63 == INT64_MIN and
    ties with the keys at the limit, an artefact of the rounding."""
    n = 240
    rng = np.random.default_rng(13 + near_max)
    edge = wrg.INT64_MAX if near_max else wrg.INT64_MIN
    sign = -1 if near_max else 1
    o = (edge + sign * rng.integers(0, 9, n).astype(object)).astype(np.int64)
    assert (o == edge).sum() > 5
    p = rng.integers(0, 2, n).astype(np.float64)
    v = pd.array(rng.integers(-1000, 1000, n), dtype="Int64")
    v[rng.random(n) < 0.15] = pd.NA
    df = pd.DataFrame({"rid": np.arange(n, dtype=np.int64),
                       "p": pd.array(p.astype(np.int64), dtype="Int64"),
                       "o": o, "v": v,
                       "w": _peer_value(p, (o - edge).astype(np.float64), 5)})
    lite = ro.SqliteTable("tl", df)
    frames = [(OFF(5), OFF(100)), (OFF(-100), OFF(-5)), (OFF(-100), OFF(100)),
              (OFF(3), ro.UNB), (ro.UNB, OFF(-3)), (OFF(2), OFF(4))]
    for lo, hi in frames:
        for desc in (False, True):
            what = f"{ro.frame_sql(lo, hi)} desc={desc}"
            want = _brute(df, lo, hi, desc)
            for f in want:
                got = _host(df, f, lo, hi, desc, False, key=(o, None))
                if f.startswith("count"):
                    got = np.nan_to_num(got)
                ro.assert_same(got, want[f], f"limit {f} {what}")
            if near_max:
                lite_want = lite.run(FUNCS, ro.over_sql(lo, hi, desc))
                for f in FUNCS:
                    got = _host(df, f, lo, hi, desc, False, key=(o, None))
                    ro.assert_same(got, lite_want[f],
                                   f"limit {f} {what} vs sqlite")
