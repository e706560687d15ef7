"""GPU tests: RANGE window frames with value offsets on the device
(dsx_window_range — k_win_range_key / k_win_range_bounds for the per-row
frame bounds, the k_win_segscan_* scans, the k_win_rmq_* sparse table for
MIN/MAX bounded on both sides, k_win_range_apply for the result).

Every case checks through the kernel profile that the new kernels really
launched (k_win_range_bounds and k_win_range_apply always, k_win_rmq_*
exactly when a MIN/MAX is bounded on both sides), and compares the result
bit for bit, NULL positions and dtypes included, with (a) the same query
under DSX_DISABLE_DEVWINDOW=1, which runs the numpy host model, and (b) the
in-process sqlite3. Values are small integers, so sums are exact in any
order. FIRST_VALUE/LAST_VALUE read a column that is a function of
(partition, key): the order among peers, which SQL leaves open, cannot show.
"""
import numpy as np
import pandas as pd
import pytest

from dask_sql_amd.physical import window_range as wrg
from tests import range_oracle as ro
from tests.range_oracle import CUR, OFF, UNB

pytestmark = pytest.mark.gpu

RANGE_KERNELS = ("k_win_range_key", "k_win_range_bounds",
                 "k_win_range_apply", "k_win_rmq_blocks", "k_win_rmq_level")
FUNCS = ("sum", "count", "countstar", "avg", "min", "max", "first", "last")


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    return Context()


def _run(ctx, sql):
    r = ctx._get_runtime()
    r.prof_enable(True)
    r.prof_reset()
    try:
        out = ctx.sql(sql).compute()
        prof = r.prof_get()
    finally:
        r.prof_enable(False)
    return out.sort_values("rid").reset_index(drop=True), prof


def _launches(prof, name):
    return prof.get(name, {}).get("launches", 0)


def _host(ctx, monkeypatch, sql):
    """Same query through the numpy host model; no range kernel may run."""
    monkeypatch.setenv("DSX_DISABLE_DEVWINDOW", "1")
    try:
        out, prof = _run(ctx, sql)
    finally:
        monkeypatch.delenv("DSX_DISABLE_DEVWINDOW")
    for k in RANGE_KERNELS:
        assert _launches(prof, k) == 0, (k, prof)
    return out


def _levels(n):
    return ((n + 63) // 64).bit_length()


def _check(ctx, monkeypatch, table, lite, funcs, over, lite_over=None,
           rmq=0, n=None, what="", sqlite=True):
    """Run `funcs` over one OVER clause on the device, on the host model and
    in sqlite. `rmq` = how many of the columns need the sparse table."""
    sql = ro.query(table, funcs, over)
    got, prof = _run(ctx, sql)
    assert _launches(prof, "k_win_range_bounds") == len(funcs), prof
    assert _launches(prof, "k_win_range_apply") == len(funcs), prof
    assert _launches(prof, "k_win_rmq_blocks") == rmq, prof
    assert _launches(prof, "k_win_rmq_level") == \
        rmq * (_levels(n if n is not None else lite.n) - 1), prof
    ref = _host(ctx, monkeypatch, sql)
    want = _sqlite(lite, funcs, lite_over or over) if sqlite else None
    for f in funcs:
        assert got[f].dtype == ref[f].dtype, (f, got[f].dtype, ref[f].dtype)
        ro.assert_same(ro.f64(got[f]), ro.f64(ref[f]),
                       f"{what} {f} OVER ({over}) vs host model")
        if sqlite:
            ro.assert_same(ro.f64(got[f]), want[f],
                           f"{what} {f} OVER ({over}) vs sqlite")
    return got, prof


_SQLITE_CACHE = {}


def _sqlite(lite, funcs, over):
    """sqlite answers are computed once per (table, clause) and shared by
    the cases that differ only in the engine's front half."""
    key = (lite.name, funcs, over)
    if key not in _SQLITE_CACHE:
        _SQLITE_CACHE[key] = lite.run(funcs, over)
    return _SQLITE_CACHE[key]


def _peer_value(p, o, mod):
    h = (np.where(np.isnan(p), 97.0, p) * 31
         + np.where(np.isnan(o), 53.0, o) * 7).astype(np.int64)
    w = pd.array(h % 1000 - 500, dtype="Int64")
    w[h % mod == 0] = pd.NA
    return w


def _nullable(arr, null):
    a = pd.array(np.where(null, 0, arr).astype(np.int64), dtype="Int64")
    a[null] = pd.NA
    return a


# ---- 1. the general table -------------------------------------------------------
# 5 000 rows = 20 scan tiles and 79 sparse-table blocks with 7 levels. One
# partition of 3 000 rows (about 10 rows per key: a 50-wide frame holds some
# 500 rows and takes the table, a 5-wide one the direct loop), partitions of
# 1 to 40 rows behind it, and 60 rows with a NULL partition key.
N1 = 5000


@pytest.fixture(scope="module")
def general(ctx):
    rng = np.random.default_rng(20241021)
    sizes = [3000]
    while sum(sizes) < N1 - 60:
        sizes.append(int(min(rng.integers(1, 41), N1 - 60 - sum(sizes))))
    sizes[-3:-1] = [1] * (sizes[-3] + sizes[-2])        # one-row partitions
    p = np.repeat(np.arange(len(sizes), dtype=np.float64) * 3 - 7, sizes)
    p = np.concatenate([p, np.full(N1 - len(p), np.nan)])
    assert len(p) == N1 and sizes.count(1) >= 2
    o = rng.integers(0, 300, N1).astype(np.float64)
    o[rng.random(N1) < 0.08] = np.nan
    v = pd.array(rng.integers(-1000, 1000, N1), dtype="Int64")
    v[rng.random(N1) < 0.15] = pd.NA
    df = pd.DataFrame({"p": _nullable(p, np.isnan(p)),
                       "o": _nullable(o, np.isnan(o)), "v": v,
                       "w": _peer_value(p, o, 7)})
    df = df.iloc[rng.permutation(N1)].reset_index(drop=True)
    df.insert(0, "rid", np.arange(N1, dtype=np.int64))
    assert (N1 + 255) // 256 == 20 and (N1 + 63) // 64 == 79
    assert _levels(N1) == 7 and wrg.rmq_table_bytes(N1) == 8 * 79 * 7
    ctx.create_table("wg_general", df)
    return df, ro.SqliteTable("wg_general", df)


M = 10**6
GENERAL_FRAMES = [
    (OFF(-5), CUR), (OFF(-M), CUR),                     # a P .. CUR
    (OFF(-1), OFF(1)), (OFF(-50), OFF(5)), (OFF(0), OFF(0)),
    (CUR, OFF(5)),                                      # CUR .. b F
    (UNB, OFF(1)), (UNB, OFF(50)),                      # UNB .. b F
    (OFF(-5), UNB), (OFF(-50), UNB),                    # a P .. UNB
    (OFF(1), OFF(5)),                                   # a F .. b F
    (OFF(-50), OFF(-5)),                                # a P .. b P
    (OFF(-2), OFF(-5)),                                 # inverted
    (CUR, CUR), (UNB, UNB),
]


@pytest.mark.parametrize("words", [False, True], ids=["bucket", "words"])
@pytest.mark.parametrize("desc, nulls_first", [(False, False), (True, False),
                                               (False, True), (True, True)])
@pytest.mark.parametrize("lo, hi", GENERAL_FRAMES,
                         ids=[ro.frame_sql(*f)[14:].replace(" ", "_")
                              for f in GENERAL_FRAMES])
def test_general_table(ctx, monkeypatch, general, lo, hi, desc, nulls_first,
                       words):
    df, lite = general
    if words:
        monkeypatch.setenv("DSX_WIN_WORDS", "1")
    bounded = lo != UNB and hi != UNB
    # the engine's default NULL placement is LAST in both directions; sqlite
    # gets it spelled out
    over = ro.over_sql(lo, hi, desc, nulls_first, spell_nulls=False)
    lite_over = ro.over_sql(lo, hi, desc, nulls_first)
    got, prof = _check(ctx, monkeypatch, "wg_general", lite, FUNCS, over,
                       lite_over, rmq=2 if bounded else 0)
    offset = lo[0] == "off" or hi[0] == "off"
    assert _launches(prof, "k_win_range_key") == (len(FUNCS) if offset else 0)
    # an explicit NULLS FIRST is sorted by the word front half either way
    if words or nulls_first:
        assert _launches(prof, "k_win_mark_word") > 0
    else:
        assert _launches(prof, "k_win_mark_word") == 0
    # COUNT is int64 and never NULL: an empty frame counts 0
    assert got["count"].dtype == np.int64
    assert got["countstar"].dtype == np.int64
    if wrg.range_can_be_empty(*(wrg.RangeBound(wrg.OFFSET, b[1])
                                if b[0] == "off" else
                                wrg.RangeBound(wrg.UNBOUNDED) for b in
                                (lo, hi))):
        assert (got["countstar"] == 0).any()


def test_dtype_rule(ctx, general):
    over = "PARTITION BY p ORDER BY o RANGE BETWEEN 5 PRECEDING AND "
    sql = ("SELECT rid, "
           f"SUM(rid) OVER ({over} CURRENT ROW) AS s_int, "
           f"MIN(rid) OVER ({over} 1 FOLLOWING) AS m_int, "
           f"SUM(rid) OVER ({over} 2 PRECEDING) AS s_gap, "
           f"SUM(v) OVER ({over} CURRENT ROW) AS s_null, "
           f"AVG(rid) OVER ({over} CURRENT ROW) AS a_int, "
           f"COUNT(v) OVER ({over} 2 PRECEDING) AS c_gap, "
           f"FIRST_VALUE(rid) OVER ({over} CURRENT ROW) AS f_int "
           "FROM wg_general")
    got, prof = _run(ctx, sql)
    assert _launches(prof, "k_win_range_bounds") == 7
    assert _launches(prof, "k_win_range_apply") == 7
    assert _launches(prof, "k_win_rmq_blocks") == 1
    assert got["s_int"].dtype == np.int64
    assert got["m_int"].dtype == np.int64
    assert got["c_gap"].dtype == np.int64
    assert got["s_gap"].dtype == np.float64 and got["s_gap"].isna().any()
    assert got["s_null"].dtype == np.float64
    assert got["a_int"].dtype == np.float64
    assert got["f_int"].notna().all()


# ---- 2. sparse-table edges ------------------------------------------------------
# One partition, 5 000 unique keys equal to the row's sorted position: an
# offset is a row distance, so the frame of `w PRECEDING` holds w + 1 rows
# (64 and 128 are the block size and the direct-loop limit) and the ROWS
# frame of the same numbers is the same frame.
@pytest.fixture(scope="module")
def dense(ctx):
    rng = np.random.default_rng(5)
    o = rng.permutation(N1).astype(np.float64)
    v = pd.array(rng.integers(-10**6, 10**6, N1), dtype="Int64")
    v[rng.random(N1) < 0.15] = pd.NA
    v[(o >= 1000) & (o < 1300)] = pd.NA          # frames without any value
    df = pd.DataFrame({"rid": np.arange(N1, dtype=np.int64),
                       "o": o.astype(np.int64), "v": v,
                       "w": _peer_value(np.zeros(N1), o, 7)})
    ctx.create_table("wg_dense", df)
    return df, ro.SqliteTable("wg_dense", df)


@pytest.mark.parametrize("w", [62, 63, 64, 127, 128, 129, 4000])
def test_rmq_edges(ctx, monkeypatch, dense, w):
    df, lite = dense
    funcs = ("min", "max")
    for lo, hi in ((OFF(-w), CUR), (OFF(-w), OFF(w))):
        over = ro.over_sql(lo, hi, partition=False, spell_nulls=False)
        got, prof = _check(ctx, monkeypatch, "wg_dense", lite, funcs, over,
                           ro.over_sql(lo, hi, partition=False), rmq=2)
        if w <= 511:
            # within ROWS' MIN/MAX tile limit (2 w + 1 <= 1023 rows)
            rows_sql = ro.query("wg_dense", funcs, "ORDER BY o ROWS" +
                                ro.frame_sql(lo, hi)[5:])
            rows, rprof = _run(ctx, rows_sql)
            assert _launches(rprof, "k_win_rows_tile") == 2
            for f in funcs:
                ro.assert_same(ro.f64(got[f]), ro.f64(rows[f]),
                               f"{f} w={w} RANGE vs ROWS on the device")


# ---- 3. float, date and timestamp keys --------------------------------------------
N3 = 1500


def _typed_table(ctx, name, key_engine, key_sqlite, null, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 4, N3).astype(np.float64)
    v = pd.array(rng.integers(-1000, 1000, N3), dtype="Int64")
    v[rng.random(N3) < 0.15] = pd.NA
    w = _peer_value(p, np.where(null, np.nan, pd.factorize(key_sqlite)[0]), 5)
    base = {"rid": np.arange(N3, dtype=np.int64), "p": p.astype(np.int64)}
    ctx.create_table(name, pd.DataFrame({**base, "o": key_engine, "v": v,
                                         "w": w}))
    return ro.SqliteTable(name, pd.DataFrame({**base, "o": key_sqlite,
                                              "v": v, "w": w}))


@pytest.fixture(scope="module")
def float_table(ctx):
    rng = np.random.default_rng(31)
    o = rng.integers(-40, 40, N3) / 4.0              # quarter steps: exact
    zero = o == 0.0
    o[zero] = np.where(rng.random(zero.sum()) < 0.5, -0.0, 0.0)
    null = rng.random(N3) < 0.08
    o[null] = np.nan                                 # NaN keys count as NULL
    assert np.signbit(o[zero & ~null]).any() and \
        not np.signbit(o[zero & ~null]).all()
    # sqlite has no -0.0 / NaN distinction to offer: 0.0 and NULL
    lite_o = pd.Series(np.where(null, np.nan, o + 0.0)).astype(object) \
        .where(~null, None)
    return _typed_table(ctx, "wg_float", o, lite_o, null, 32)


@pytest.mark.parametrize("desc, nulls_first", [(False, False), (True, True)])
@pytest.mark.parametrize("lo, hi", [(OFF(-0.5), CUR), (OFF(-2.25), OFF(0.5)),
                                    (OFF(0.5), OFF(2.25)), (UNB, OFF(-0.5))])
def test_float_keys(ctx, monkeypatch, float_table, lo, hi, desc, nulls_first):
    bounded = lo != UNB and hi != UNB
    _check(ctx, monkeypatch, "wg_float", float_table, FUNCS,
           ro.over_sql(lo, hi, desc, nulls_first, spell_nulls=False),
           ro.over_sql(lo, hi, desc, nulls_first),
           rmq=2 if bounded else 0, what="float keys")


@pytest.fixture(scope="module")
def date_table(ctx):
    rng = np.random.default_rng(41)
    days = 19_000 + rng.integers(0, 90, N3)
    null = rng.random(N3) < 0.08
    eng = pd.Series(days.astype("datetime64[D]").astype("datetime64[ns]"))
    eng[null] = pd.NaT
    lite = pd.Series(days.astype(object)).where(~null, None)
    return _typed_table(ctx, "wg_date", eng, lite, null, 42)


@pytest.fixture(scope="module")
def ts_table(ctx):
    rng = np.random.default_rng(51)
    ns = 1_700_000_000 * 10**9 + rng.integers(0, 900, N3) * 60 * 10**9 \
        + rng.integers(0, 2, N3) * 10**9
    null = rng.random(N3) < 0.08
    eng = pd.Series(ns.astype("datetime64[ns]"))
    eng[null] = pd.NaT
    lite = pd.Series(ns.astype(object)).where(~null, None)
    return _typed_table(ctx, "wg_ts", eng, lite, null, 52)


@pytest.mark.parametrize("desc", [False, True])
def test_date_keys(ctx, monkeypatch, date_table, desc):
    for lo_e, hi_e, lo, hi in (
            ("INTERVAL '7' DAY PRECEDING", "CURRENT ROW", OFF(-7), CUR),
            ("INTERVAL '7' DAY PRECEDING", "INTERVAL '1' WEEK FOLLOWING",
             OFF(-7), OFF(7))):
        order = "ORDER BY o" + (" DESC" if desc else "")
        _check(ctx, monkeypatch, "wg_date", date_table, FUNCS,
               f"PARTITION BY p {order} RANGE BETWEEN {lo_e} AND {hi_e}",
               ro.over_sql(lo, hi, desc), rmq=2, what="date keys")


@pytest.mark.parametrize("desc", [False, True])
def test_timestamp_keys(ctx, monkeypatch, ts_table, desc):
    off = 90 * 60 * 10**9
    for lo_e, hi_e, lo, hi in (
            ("INTERVAL '90' MINUTE PRECEDING", "CURRENT ROW", OFF(-off), CUR),
            ("INTERVAL '90' MINUTE PRECEDING", "INTERVAL '90' MINUTE "
             "FOLLOWING", OFF(-off), OFF(off))):
        order = "ORDER BY o" + (" DESC" if desc else "")
        _check(ctx, monkeypatch, "wg_ts", ts_table, FUNCS,
               f"PARTITION BY p {order} RANGE BETWEEN {lo_e} AND {hi_e}",
               ro.over_sql(lo, hi, desc), rmq=2, what="timestamp keys")


# ---- 4. two order keys, peer-only frame ---------------------------------------------
def test_two_order_keys(ctx, monkeypatch, general):
    df, _ = general
    rng = np.random.default_rng(61)
    o2 = pd.array(rng.integers(0, 3, N1), dtype="Int64")
    o2[rng.random(N1) < 0.1] = pd.NA
    df2 = df.assign(o2=o2)
    ctx.create_table("wg_two", df2)
    lite = ro.SqliteTable("wg_two", df2)
    funcs = ("sum", "count", "countstar", "min", "max")
    frame = "RANGE BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING"
    got, prof = _check(
        ctx, monkeypatch, "wg_two", lite, funcs,
        f"PARTITION BY p ORDER BY o, o2 DESC {frame}",
        f"PARTITION BY p ORDER BY o NULLS LAST, o2 DESC NULLS LAST {frame}",
        rmq=0, what="two keys")
    assert _launches(prof, "k_win_range_key") == 0
    with pytest.raises(ValueError):
        ctx.sql("SELECT SUM(v) OVER (ORDER BY o, o2 RANGE 1 PRECEDING) AS s "
                "FROM wg_two")


# ---- 5. keys at the int64 limits ------------------------------------------------------
@pytest.mark.parametrize("near_max", [True, False], ids=["max", "min"])
@pytest.mark.parametrize("desc", [False, True])
def test_saturating_keys(ctx, monkeypatch, near_max, desc):
    """Keys within 10 of INT64_MAX (or INT64_MIN) next to keys some 2^40
    away: key + 100 (or key - 100) leaves int64 and must saturate, not
    wrap. The span stays under 2^62, so the key packs."""
    n = 600
    rng = np.random.default_rng(71 + near_max)
    edge = np.iinfo(np.int64).max if near_max else np.iinfo(np.int64).min
    sign = -1 if near_max else 1
    o = np.where(rng.random(n) < 0.5,
                 edge + sign * rng.integers(0, 11, n),
                 edge + sign * ((1 << 40) + rng.integers(0, 300, n)))
    o = o.astype(np.int64)
    assert (np.abs(o.astype(object) - int(edge)) <= 10).sum() > 100
    v = pd.array(rng.integers(-1000, 1000, n), dtype="Int64")
    v[rng.random(n) < 0.15] = pd.NA
    p = rng.integers(0, 3, n).astype(np.float64)
    df = pd.DataFrame({"rid": np.arange(n, dtype=np.int64),
                       "p": p.astype(np.int64), "o": o, "v": v,
                       "w": _peer_value(p, pd.factorize(o)[0]
                                        .astype(np.float64), 5)})
    name = "wg_sat_max" if near_max else "wg_sat_min"
    ctx.create_table(name, df)
    lite = ro.SqliteTable(name, df)
    for lo, hi in ((OFF(-100), OFF(100)), (OFF(-100), CUR), (CUR, OFF(100))):
        _check(ctx, monkeypatch, name, lite, FUNCS,
               ro.over_sql(lo, hi, desc, spell_nulls=False),
               ro.over_sql(lo, hi, desc), rmq=2, n=n, what="saturation")
    # a target past the limit on the side no key can reach admits no row,
    # also not the keys AT the limit, which tie with the saturated target.
    # The host model is checked against the exact inclusion rule on the CPU
    # (test_window_range_lowering.py); sqlite is asked near INT64_MAX only:
    # near INT64_MIN its REAL target rounds onto the limit itself
    for lo, hi in ((OFF(5), OFF(100)), (OFF(-100), OFF(-5))):
        got, _ = _check(ctx, monkeypatch, name, lite, FUNCS,
                        ro.over_sql(lo, hi, desc, spell_nulls=False),
                        ro.over_sql(lo, hi, desc), rmq=2, n=n,
                        what="saturation, no row", sqlite=near_max)
        assert (got["countstar"] == 0).any()


# ---- NULLS FIRST with the word front half off -----------------------------------------
def test_nulls_first_without_words_is_still_a_range_frame(ctx, monkeypatch,
                                                          general):
    """DSX_DISABLE_WINWORDS=1 takes the only device sort that honours an
    explicit NULLS FIRST away. The frame must then run on the host model of
    RANGE frames, not on the ROWS rolling path, which would read the offset
    as a row count: no range kernel launches, and the answer is the one the
    device gives without the knob, and sqlite's."""
    df, lite = general
    for lo, hi, desc in ((OFF(-5), CUR, False), (OFF(-50), OFF(5), True)):
        over = ro.over_sql(lo, hi, desc, True, spell_nulls=False)
        sql = ro.query("wg_general", FUNCS, over)
        dev, dprof = _run(ctx, sql)
        assert _launches(dprof, "k_win_range_bounds") == len(FUNCS)
        monkeypatch.setenv("DSX_DISABLE_WINWORDS", "1")
        try:
            got, prof = _run(ctx, sql)
        finally:
            monkeypatch.delenv("DSX_DISABLE_WINWORDS")
        for k in RANGE_KERNELS + ("k_win_rows_tile", "k_win_rows_prefix"):
            assert _launches(prof, k) == 0, (k, prof)
        want = _sqlite(lite, FUNCS, ro.over_sql(lo, hi, desc, True))
        for f in FUNCS:
            assert got[f].dtype == dev[f].dtype
            ro.assert_same(ro.f64(got[f]), ro.f64(dev[f]),
                           f"{f} words off vs device")
            ro.assert_same(ro.f64(got[f]), want[f], f"{f} words off vs sqlite")


# ---- a computed key that holds a valid NaN ----------------------------------------------
def test_computed_nan_key(ctx, monkeypatch):
    """NaN in a table column becomes NULL at upload, so the staged key's own
    NaN test only sees a computed key: o + (g - g) is NaN, with the validity
    bit set, wherever g is infinite. Those rows must form the NULL block.
    sqlite turns the same expression into NULL."""
    n = 1200
    rng = np.random.default_rng(81)
    p = rng.integers(0, 3, n).astype(np.float64)
    o = rng.integers(-40, 40, n) / 4.0
    g = np.where(rng.random(n) < 0.1, np.inf, 1.0)
    v = pd.array(rng.integers(-1000, 1000, n), dtype="Int64")
    v[rng.random(n) < 0.15] = pd.NA
    df = pd.DataFrame({"rid": np.arange(n, dtype=np.int64),
                       "p": p.astype(np.int64), "o": o, "g": g, "v": v,
                       "w": _peer_value(p, np.where(np.isinf(g), np.nan,
                                                    o * 4), 5)})
    ctx.create_table("wg_nan", df)
    lite = ro.SqliteTable("wg_nan", df)
    for desc, nulls_first in ((False, False), (True, True)):
        for lo, hi in ((OFF(-0.5), CUR), (OFF(-2.25), OFF(0.5))):
            _check(ctx, monkeypatch, "wg_nan", lite, FUNCS,
                   ro.over_sql(lo, hi, desc, nulls_first, order="o + (g - g)",
                               spell_nulls=False),
                   ro.over_sql(lo, hi, desc, nulls_first,
                               order="o + (g - g)"),
                   rmq=2, n=n, what="computed NaN key")


# ---- 6. the table-size knob --------------------------------------------------------------
def test_rmq_cap_falls_back_to_the_host_model(ctx, monkeypatch, general):
    df, lite = general
    assert wrg.rmq_table_bytes(N1) > 1024
    funcs = ("sum", "min", "max")
    lo, hi = OFF(-50), OFF(5)
    over = ro.over_sql(lo, hi, spell_nulls=False)
    sql = ro.query("wg_general", funcs, over)
    free, fprof = _run(ctx, sql)
    assert _launches(fprof, "k_win_rmq_blocks") == 2
    monkeypatch.setenv("DSX_WIN_RANGE_RMQ_MAX_BYTES", "1024")
    capped, prof = _run(ctx, sql)
    monkeypatch.delenv("DSX_WIN_RANGE_RMQ_MAX_BYTES")
    # SUM stays on the device; MIN and MAX are declined before any launch
    assert _launches(prof, "k_win_range_bounds") == 1
    assert _launches(prof, "k_win_range_apply") == 1
    assert _launches(prof, "k_win_rmq_blocks") == 0
    assert _launches(prof, "k_win_rmq_level") == 0
    want = _sqlite(lite, funcs, ro.over_sql(lo, hi))
    for f in funcs:
        assert capped[f].dtype == free[f].dtype
        ro.assert_same(ro.f64(capped[f]), ro.f64(free[f]), f"capped {f}")
        ro.assert_same(ro.f64(capped[f]), want[f], f"capped {f} vs sqlite")


# ---- 7. an empty table and a one-row table -------------------------------------------------
def test_one_row_table(ctx, monkeypatch):
    df = pd.DataFrame({"rid": np.zeros(1, dtype=np.int64),
                       "p": np.array([3], dtype=np.int64),
                       "o": np.array([10], dtype=np.int64),
                       "v": np.array([-4], dtype=np.int64),
                       "w": np.array([9], dtype=np.int64)})
    ctx.create_table("wg_one", df)
    lite = ro.SqliteTable("wg_one", df)
    for lo, hi, rmq in ((OFF(-1), OFF(1), 2), (OFF(1), OFF(2), 2),
                        (CUR, UNB, 0)):
        got, _ = _check(ctx, monkeypatch, "wg_one", lite, FUNCS,
                        ro.over_sql(lo, hi, spell_nulls=False),
                        ro.over_sql(lo, hi), rmq=rmq, n=1)
    assert got["sum"].tolist() == [-4]


def test_empty_table(ctx, monkeypatch):
    """No row, so no kernel has anything to launch for: the plugin answers
    from the host model, as the ROWS path does. Both routes and sqlite
    agree on zero rows and on the column dtypes."""
    df = pd.DataFrame({"rid": np.zeros(0, dtype=np.int64),
                       "p": np.zeros(0, dtype=np.int64),
                       "o": np.zeros(0, dtype=np.int64),
                       "v": np.zeros(0, dtype=np.int64),
                       "w": np.zeros(0, dtype=np.int64)})
    ctx.create_table("wg_empty", df)
    lite = ro.SqliteTable("wg_empty", df)
    over = ro.over_sql(OFF(-1), OFF(1), spell_nulls=False)
    sql = ro.query("wg_empty", FUNCS, over)
    got, prof = _run(ctx, sql)
    for k in RANGE_KERNELS:
        assert _launches(prof, k) == 0
    ref = _host(ctx, monkeypatch, sql)
    want = lite.run(FUNCS, ro.over_sql(OFF(-1), OFF(1)))
    for f in FUNCS:
        assert len(got[f]) == 0 and len(ref[f]) == 0 and len(want[f]) == 0
        assert got[f].dtype == ref[f].dtype
