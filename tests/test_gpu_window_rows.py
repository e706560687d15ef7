"""GPU tests: explicit ROWS window frames on the device (dsx_window_rows —
k_win_rows_tile for narrow bounded frames, the k_win_segscan_* scans +
k_win_rows_prefix for unbounded sides / wide sums / FIRST / LAST).

Every case checks that the new kernel really launched, and compares the
result with (a) the host rolling path (DSX_DISABLE_DEVWINDOW=1, the
behaviour before the device path existed) and (b) an independent numpy
restatement of the frame model: int64 prefix sums for SUM/COUNT, explicit
slices for MIN/MAX/FIRST/LAST. Values are integers, so sums are exact in
any order and results must match bit for bit, NULL positions included."""
import numpy as np
import pandas as pd
import pytest

from dask_sql_amd.physical import window_frames as wf

pytestmark = pytest.mark.gpu

NEW_KERNELS = ("k_win_stage", "k_win_rows_tile", "k_win_rows_prefix",
               "k_win_segscan_tile", "k_win_segscan_carry",
               "k_win_segscan_apply")
FUNCS = ("sum", "count", "countstar", "avg", "min", "max", "first", "last")


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    return Context()


# ---- frame spelling ---------------------------------------------------------
def _bound(off, side):
    if off is None:
        return "UNBOUNDED " + ("PRECEDING" if side == "lo" else "FOLLOWING")
    if off == 0:
        return "CURRENT ROW"
    return f"{-off} PRECEDING" if off < 0 else f"{off} FOLLOWING"


def _frame_sql(lo, hi):
    return f"ROWS BETWEEN {_bound(lo, 'lo')} AND {_bound(hi, 'hi')}"


_EXPR = {"sum": "SUM(v)", "count": "COUNT(v)", "countstar": "COUNT(*)",
         "avg": "AVG(v)", "min": "MIN(v)", "max": "MAX(v)",
         "first": "FIRST_VALUE(v)", "last": "LAST_VALUE(v)"}


def _sql(table, funcs, lo, hi, partition=True):
    over = ("PARTITION BY p " if partition else "") + "ORDER BY o " + \
        _frame_sql(lo, hi)
    cols = ", ".join(f"{_EXPR[f]} OVER ({over}) AS {f}" for f in funcs)
    return f"SELECT rid, {cols} FROM {table}"


# ---- running a query with the kernel profile --------------------------------
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
    """Same query on the host rolling path; no new kernel may launch."""
    monkeypatch.setenv("DSX_DISABLE_DEVWINDOW", "1")
    try:
        out, prof = _run(ctx, sql)
    finally:
        monkeypatch.delenv("DSX_DISABLE_DEVWINDOW")
    for k in NEW_KERNELS:
        assert _launches(prof, k) == 0, (k, prof)
    return out


def _f64(series):
    return series.to_numpy(dtype=np.float64, na_value=np.nan)


def _assert_same(got, want, what):
    got, want = _f64(got), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(np.isnan(got) != np.isnan(want))
    assert bad.size == 0, f"{what}: NULL positions differ at rows {bad[:8]}"
    ok = ~np.isnan(want)
    bad = np.flatnonzero(ok)[got[ok] != want[ok]]
    assert bad.size == 0, (f"{what}: values differ at rows {bad[:8]}: "
                           f"{got[bad[:8]]} vs {want[bad[:8]]}")


# ---- numpy restatement of the frame model ------------------------------------
def _model(df, lo, hi, partition=True, slices=True):
    """Expected columns (float64, NaN = NULL) in rid order."""
    n = len(df)
    p = df["p"].to_numpy() if partition else np.zeros(n, dtype=np.int64)
    order = np.lexsort((df["o"].to_numpy(), p))     # sorted pos → row
    ps = p[order]
    valid = df["v"].notna().to_numpy()[order]
    vals = df["v"].fillna(0).to_numpy(dtype=np.int64)[order]
    csum = np.concatenate([[0], np.cumsum(np.where(valid, vals, 0))])
    ccnt = np.concatenate([[0], np.cumsum(valid.astype(np.int64))])
    head = np.flatnonzero(np.r_[True, ps[1:] != ps[:-1]])
    p0 = np.repeat(head, np.diff(np.r_[head, n]))
    p1 = np.repeat(np.r_[head[1:], n], np.diff(np.r_[head, n]))
    i = np.arange(n, dtype=np.int64)
    s = p0 if lo is None else np.maximum(p0, i + lo)
    e = p1 - 1 if hi is None else np.minimum(p1 - 1, i + hi)
    empty = s > e
    sc = np.where(empty, 0, s)
    ec = np.where(empty, 0, e)
    tot = (csum[ec + 1] - csum[sc]).astype(np.float64)
    cnt = ccnt[ec + 1] - ccnt[sc]
    nothing = empty | (cnt == 0)
    exp = {
        "sum": np.where(nothing, np.nan, tot),
        "count": np.where(empty, np.nan, cnt.astype(np.float64)),
        "countstar": np.where(empty, np.nan, (ec - sc + 1).astype(np.float64)),
        "avg": np.where(nothing, np.nan, tot / np.where(cnt == 0, 1, cnt)),
        "first": np.where(empty | ~valid[sc], np.nan,
                          vals[sc].astype(np.float64)),
        "last": np.where(empty | ~valid[ec], np.nan,
                         vals[ec].astype(np.float64)),
    }
    mn = np.full(n, np.nan)
    mx = np.full(n, np.nan)
    if slices:
        for k in np.flatnonzero(~nothing):
            w = vals[s[k]:e[k] + 1][valid[s[k]:e[k] + 1]]
            mn[k] = w.min()
            mx[k] = w.max()
    else:
        # one partition, one side unbounded: running extrema (the slices
        # above would be O(n^2) at the many-tile size)
        assert head.size == 1 and (lo is None) != (hi is None)
        lo_v = np.where(valid, vals, np.iinfo(np.int64).max)
        hi_v = np.where(valid, vals, np.iinfo(np.int64).min)
        if lo is None:
            rmn = np.minimum.accumulate(lo_v)[ec]
            rmx = np.maximum.accumulate(hi_v)[ec]
        else:
            rmn = np.minimum.accumulate(lo_v[::-1])[::-1][sc]
            rmx = np.maximum.accumulate(hi_v[::-1])[::-1][sc]
        mn = np.where(nothing, np.nan, rmn.astype(np.float64))
        mx = np.where(nothing, np.nan, rmx.astype(np.float64))
    exp["min"], exp["max"] = mn, mx
    out = {}
    for name, col in exp.items():      # sorted space → rid order
        a = np.empty(n, dtype=np.float64)
        a[df["rid"].to_numpy()[order]] = col
        out[name] = a
    return out


# ---- the tile-edge table -----------------------------------------------------
# sorted layout: partitions of 255, 1, 257, 2, 600, 256, 40 and 90 rows —
# heads at 0, 255, 256 (exactly a tile edge), 513, 515, 1115, 1371, 1411, so
# the 257/600/256-row partitions straddle 256-row tile boundaries and n =
# 1501 leaves a 221-row last tile. The 40-row partition is all NULL.
PLENS = (255, 1, 257, 2, 600, 256, 40, 90)


@pytest.fixture(scope="module")
def edge_table(ctx):
    rng = np.random.default_rng(20240607)
    p = np.repeat(np.arange(len(PLENS), dtype=np.int64) * 7 - 3, PLENS)
    o = np.concatenate([rng.permutation(ln) * 3 - 50 for ln in PLENS]) \
        .astype(np.int64)
    n = len(p)
    v = pd.array(rng.integers(-1000, 1000, n), dtype="Int64")
    v[rng.random(n) < 0.25] = pd.NA
    v[p == p[sum(PLENS[:6])]] = pd.NA          # the 40-row partition
    shuffle = rng.permutation(n)
    df = pd.DataFrame({"p": p, "o": o, "v": v}).iloc[shuffle] \
        .reset_index(drop=True)
    df["rid"] = np.arange(n, dtype=np.int64)
    assert n == 1501 and n % 256 != 0
    ctx.create_table("wr_edge", df)
    return df


TILE_FRAMES = [(-2, 0), (-1, 1), (-2, -1), (1, 2), (-300, -290), (1, -1)]
PREFIX_FRAMES = [(None, 0), (None, 2), (-3, None), (None, None)]


def _check_all(ctx, monkeypatch, table, df, funcs, lo, hi, kernels,
               partition=True, host=True, slices=True):
    sql = _sql(table, funcs, lo, hi, partition)
    got, prof = _run(ctx, sql)
    for k in kernels:
        assert _launches(prof, k) > 0, (k, prof)
    exp = _model(df, lo, hi, partition, slices)
    for f in funcs:
        _assert_same(got[f], exp[f], f"{f} {_frame_sql(lo, hi)} vs numpy")
    if host:
        ref = _host(ctx, monkeypatch, sql)
        for f in funcs:
            _assert_same(got[f], _f64(ref[f]),
                         f"{f} {_frame_sql(lo, hi)} vs host path")
    return got, prof


@pytest.mark.parametrize("lo, hi", TILE_FRAMES)
def test_tile_frames(ctx, monkeypatch, edge_table, lo, hi):
    for f in ("sum", "count", "avg", "min", "max"):
        assert wf.frame_strategy(f, lo, hi) == "tile"
    got, prof = _check_all(ctx, monkeypatch, "wr_edge", edge_table, FUNCS,
                           lo, hi, ("k_win_rows_tile", "k_win_rows_prefix"))
    # six aggregates on the tile pass, FIRST/LAST on the positional copy,
    # and no scan for a narrow bounded frame
    assert _launches(prof, "k_win_rows_tile") == 6
    assert _launches(prof, "k_win_rows_prefix") == 2
    assert _launches(prof, "k_win_segscan_tile") == 0


@pytest.mark.parametrize("lo, hi", PREFIX_FRAMES)
def test_prefix_frames(ctx, monkeypatch, edge_table, lo, hi):
    got, prof = _check_all(ctx, monkeypatch, "wr_edge", edge_table, FUNCS,
                           lo, hi, ("k_win_rows_prefix", "k_win_segscan_tile",
                                    "k_win_segscan_carry",
                                    "k_win_segscan_apply"))
    assert _launches(prof, "k_win_rows_tile") == 0
    assert _launches(prof, "k_win_rows_prefix") == 8
    assert _launches(prof, "k_win_segscan_carry") == 6


def test_wide_bounded_sum_takes_the_prefix_path(ctx, monkeypatch, edge_table):
    d = wf.WIN_ROWS_DIRECT_MAXW
    lo, hi = -(d // 2), d - d // 2          # W = d + 1
    assert hi - lo + 1 == d + 1
    funcs = ("sum", "count", "countstar", "avg")
    for f in ("sum", "count", "avg"):
        assert wf.frame_strategy(f, lo, hi) == "prefix"
    got, prof = _check_all(ctx, monkeypatch, "wr_edge", edge_table, funcs,
                           lo, hi, ("k_win_rows_prefix",
                                    "k_win_segscan_carry"))
    assert _launches(prof, "k_win_rows_tile") == 0
    # one row narrower stays on the tile pass
    got, prof = _check_all(ctx, monkeypatch, "wr_edge", edge_table, funcs,
                           lo + 1, hi, ("k_win_rows_tile",), host=False)
    assert _launches(prof, "k_win_rows_prefix") == 0


def test_wide_bounded_min_stays_on_host(ctx, monkeypatch, edge_table):
    t = wf.WIN_ROWS_TILE_MAXW
    lo, hi = -t, 0                          # W = t + 1
    assert wf.frame_strategy("min", lo, hi) == "host"
    sql = _sql("wr_edge", ("min",), lo, hi)
    got, prof = _run(ctx, sql)
    for k in NEW_KERNELS:
        assert _launches(prof, k) == 0, (k, prof)
    _assert_same(got["min"], _model(edge_table, lo, hi)["min"],
                 "wide MIN vs numpy")
    _assert_same(got["min"], _f64(_host(ctx, monkeypatch, sql)["min"]),
                 "wide MIN vs host path")


def test_widest_tile_min_max(ctx, monkeypatch, edge_table):
    """W = WIN_ROWS_TILE_MAXW fills the whole LDS tile + halo."""
    t = wf.WIN_ROWS_TILE_MAXW
    lo, hi = -(t // 2), t - 1 - t // 2
    assert hi - lo + 1 == t
    got, prof = _check_all(ctx, monkeypatch, "wr_edge", edge_table,
                           ("min", "max"), lo, hi, ("k_win_rows_tile",))
    assert _launches(prof, "k_win_rows_prefix") == 0


def test_dtype_rule(ctx, edge_table):
    sql = ("SELECT rid, p, o, "
           "COUNT(v) OVER (PARTITION BY p ORDER BY o ROWS BETWEEN 2 "
           "PRECEDING AND CURRENT ROW) AS c_full, "
           "COUNT(v) OVER (PARTITION BY p ORDER BY o ROWS BETWEEN 2 "
           "PRECEDING AND 1 PRECEDING) AS c_gap, "
           "SUM(rid) OVER (PARTITION BY p ORDER BY o ROWS BETWEEN 2 "
           "PRECEDING AND CURRENT ROW) AS s_int, "
           "SUM(v) OVER (PARTITION BY p ORDER BY o ROWS BETWEEN 2 "
           "PRECEDING AND CURRENT ROW) AS s_null "
           "FROM wr_edge")
    got, prof = _run(ctx, sql)
    assert _launches(prof, "k_win_rows_tile") == 4
    assert got["c_full"].dtype == np.int64
    assert got["s_int"].dtype == np.int64
    assert got["c_gap"].dtype == np.float64
    assert got["s_null"].dtype == np.float64
    first = got["o"] == got.groupby("p")["o"].transform("min")
    assert first.sum() == len(PLENS)
    assert got.loc[first, "c_gap"].isna().all()
    assert got.loc[~first, "c_gap"].notna().all()
    # the all-NULL partition: COUNT is 0 (not NULL), SUM is NULL
    allnull = got["p"] == 6 * 7 - 3
    assert (got.loc[allnull, "c_full"] == 0).all()
    assert got.loc[allnull, "s_null"].isna().all()


# ---- carry across many tiles -------------------------------------------------
def test_one_partition_many_tiles(ctx):
    """ORDER BY only: one 70,001-row partition = 274 tiles, so the carry
    scan itself loops (more than 256 tiles) and every tile but the first
    takes its whole value from the carry. numpy restatement only — the host
    path is too slow at this size to belong in a seconds-long test."""
    n = 70_001
    rng = np.random.default_rng(77)
    v = pd.array(rng.integers(-1000, 1000, n), dtype="Int64")
    v[rng.random(n) < 0.2] = pd.NA
    df = pd.DataFrame({"p": np.zeros(n, dtype=np.int64),
                       "o": rng.permutation(n).astype(np.int64), "v": v,
                       "rid": np.arange(n, dtype=np.int64)})
    ctx.create_table("wr_one", df)
    assert (n + 255) // 256 > 256
    for lo, hi in ((None, 0), (-100, None)):
        _check_all(ctx, None, "wr_one", df, ("sum", "min"), lo, hi,
                   ("k_win_rows_prefix", "k_win_segscan_carry"),
                   partition=False, host=False, slices=False)


# ---- duplicate order keys ----------------------------------------------------
def test_ties_match_the_host_path(ctx, monkeypatch):
    """Duplicate order keys: which peer comes first is decided by the sort,
    and both sorts are stable by row id — compare with the host path."""
    n = 300
    rng = np.random.default_rng(5)
    df = pd.DataFrame({"p": rng.integers(0, 4, n).astype(np.int64),
                       "o": rng.integers(0, 12, n).astype(np.int64),
                       "v": rng.integers(-50, 50, n).astype(np.int64),
                       "rid": np.arange(n, dtype=np.int64)})
    ctx.create_table("wr_ties", df)
    for lo, hi, kernel in ((-2, 1, "k_win_rows_tile"),
                           (None, 1, "k_win_rows_prefix")):
        sql = _sql("wr_ties", ("sum", "min", "first", "last"), lo, hi)
        got, prof = _run(ctx, sql)
        assert _launches(prof, kernel) > 0, prof
        ref = _host(ctx, monkeypatch, sql)
        for f in ("sum", "min", "first", "last"):
            _assert_same(got[f], _f64(ref[f]), f"ties {f}")


# ---- float values through the prefix difference ------------------------------
def test_float_wide_sum(ctx, monkeypatch):
    """rng.random values, partitions of at most 500 rows: the prefix
    magnitude stays under 500, so the cancellation error of cum[e] -
    cum[s-1] is ~500 * 2^-52 ≈ 1e-13 absolute, and it only arises where
    s > p0, i.e. on frames of at least 65 values (sum ≈ 30) — orders of
    magnitude inside rtol=1e-9."""
    n = 2000
    rng = np.random.default_rng(9)
    df = pd.DataFrame({"p": np.repeat(np.arange(5, dtype=np.int64),
                                      (500, 500, 500, 499, 1)),
                       "o": rng.permutation(n).astype(np.int64),
                       "v": rng.random(n),
                       "rid": np.arange(n, dtype=np.int64)})
    ctx.create_table("wr_float", df)
    d = wf.WIN_ROWS_DIRECT_MAXW
    lo, hi = -d, d                          # W = 2 d + 1
    assert wf.frame_strategy("sum", lo, hi) == "prefix"
    sql = _sql("wr_float", ("sum", "avg"), lo, hi)
    got, prof = _run(ctx, sql)
    assert _launches(prof, "k_win_rows_prefix") == 2
    assert _launches(prof, "k_win_rows_tile") == 0
    ref = _host(ctx, monkeypatch, sql)
    # independent reference: per-row numpy slice sums in float64
    order = np.lexsort((df["o"].to_numpy(), df["p"].to_numpy()))
    ps, vs = df["p"].to_numpy()[order], df["v"].to_numpy()[order]
    exp = np.empty(n)
    for i in range(n):
        s, e = max(0, i + lo), min(n - 1, i + hi)
        w = vs[s:e + 1][ps[s:e + 1] == ps[i]]
        exp[df["rid"].to_numpy()[order[i]]] = w.sum()
    assert got["sum"].notna().all()
    np.testing.assert_allclose(_f64(got["sum"]), exp, rtol=1e-9)
    np.testing.assert_allclose(_f64(got["sum"]), _f64(ref["sum"]), rtol=1e-9)
    np.testing.assert_allclose(_f64(got["avg"]), _f64(ref["avg"]), rtol=1e-9)
