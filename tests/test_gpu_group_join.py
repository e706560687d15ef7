"""Group-join: an inner PK-FK join grouped by the PK, accumulated per build
row (dsx_filter_probe_groupby, -m gpu).

Entry level: Runtime.filter_probe_groupby over a 1 000-row build side is
compared with pandas (filter, merge, group by build row) — values, dtypes,
column order and the ascending build row order of the output. SQL level:
every query is compared, up to row order, with the same query under
DSX_DISABLE_GROUPJOIN=1 (column order, dtypes, values, floats at rtol 1e-9)
and with pandas or oracle.tpch.oracle_q3, and the launches say which path
ran."""
import numpy as np
import pandas as pd
import pytest

from tests.conftest import assert_frame_close

pytestmark = pytest.mark.gpu

N_BUILD = 1000
NONE, EXACT, HASHED = 0, 1, 2
OP_COL, OP_LIT_I64, OP_LT_I64, OP_I64_TO_F64 = 1, 3, 30, 50
KNOBS = ("DSX_DISABLE_JOINFILTER", "DSX_JOIN_FILTER_MAX_BYTES",
         "DSX_JOIN_FILTER_MIN_BITS", "DSX_DISABLE_JIT_FPROBE",
         "DSX_DISABLE_GROUPJOIN", "DSX_GROUPJOIN_MIN_ROWS",
         "DSX_DISABLE_FILTERPROBE")
FORMS = pytest.mark.parametrize("interp", [False, True],
                                ids=["generated", "interpreter"])
SIZES = pytest.mark.parametrize("n", [4097, 65_573])


@pytest.fixture(scope="module")
def runtime():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    return Context()._get_runtime()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------------------
# entry level
# ---------------------------------------------------------------------------
# probe columns, in the order of the entry's column list
PCOLS = ["f", "k", "k2", "x", "i", "xn", "nv"]
F, K, K2, X, I, XN, NV = range(7)


def _probe(n, rng, key_lo=0, key_hi=1500, null_keys=True, null_f=True):
    k = pd.array(rng.integers(key_lo, key_hi, n), dtype="Int64")
    if null_keys:
        k[rng.random(n) < 0.05] = pd.NA
    f = pd.array(rng.integers(0, 100, n), dtype="Int64")
    if null_f:
        f[rng.random(n) < 0.1] = pd.NA
    xn = pd.array(rng.random(n) * 100 - 50, dtype="Float64")
    xn[rng.random(n) < 0.5] = pd.NA
    nv = pd.array(rng.integers(-1000, 1000, n), dtype="Int64")
    nv[rng.random(n) < 0.5] = pd.NA
    return pd.DataFrame({
        "f": f, "k": k,
        "k2": rng.integers(0, 10, n).astype(np.int32),
        "x": rng.random(n) * 100 - 50,
        "i": rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64),
        "xn": xn, "nv": nv,
    })


def _build(rng, n=N_BUILD):
    bn = pd.array(rng.integers(0, 50, n), dtype="Int64")
    bn[rng.random(n) < 0.3] = pd.NA
    return pd.DataFrame({
        "bk": rng.permutation(n).astype(np.int64),  # unique keys
        "b32": rng.integers(0, 100, n).astype(np.int32),
        "bn": bn,
    })


def _upload(r, s):
    if pd.api.types.is_extension_array_dtype(s.dtype):
        valid = (~s.isna()).to_numpy()
        np_dtype = np.float64 if s.dtype == "Float64" else np.int64
        return r.upload_column(s.fillna(0).to_numpy(dtype=np_dtype),
                               valid.astype(np.uint8))
    return r.upload_column(np.ascontiguousarray(s.to_numpy()))


def _download(cols, names):
    out = {}
    for name, col in zip(names, cols):
        arr, valid = col.to_numpy()
        if valid is not None:
            arr = arr.astype(np.float64)
            arr[~valid] = np.nan
        out[name] = arr
    return pd.DataFrame(out)


def _agg_set(xc, ic, tag):
    """(agg specs, calls, names, pandas column, pandas reducer) over a float
    column xc and an integer column ic."""
    from dask_sql_amd import runtime as rt
    fx, ix = [(OP_COL, xc, 0)], [(OP_COL, ic, 0)]
    rows = [
        (rt.AGG_SUM_F64, fx, "sum_f", xc, lambda g: g.sum(min_count=1)),
        (rt.AGG_SUM_I64, ix, "sum_i", ic, lambda g: g.sum(min_count=1)),
        (rt.AGG_MIN_F64, fx, "min_f", xc, lambda g: g.min()),
        (rt.AGG_MAX_F64, fx, "max_f", xc, lambda g: g.max()),
        (rt.AGG_MIN_I64, ix, "min_i", ic, lambda g: g.min()),
        (rt.AGG_MAX_I64, ix, "max_i", ic, lambda g: g.max()),
        (rt.AGG_SUM_F64, fx, "avg", xc, lambda g: g.mean()),
        (rt.AGG_COUNT, ix, "count", ic, lambda g: g.count()),
    ]
    return [(op, prog, fin, f"{fin}_{tag}", PCOLS[c], red)
            for op, prog, fin, c, red in rows]


def _aggs_all():
    from dask_sql_amd import runtime as rt
    star = [(rt.AGG_COUNT, [(OP_LIT_I64, 0, 1)], "count", "count_star", None,
             None)]
    return {
        "never_null": _agg_set(X, I, "nn") + star,
        "nullable": _agg_set(XN, NV, "nu") + star,
        # Q3's shape: one never-NULL f64 SUM, no count anywhere. The sum
        # itself tells which build rows matched (the −0.0 start).
        "sum_only": _agg_set(X, I, "nn")[:1],
        # no row count and no never-NULL f64 SUM: the live byte in word 0
        # tells which build rows matched
        "sum_i_only": _agg_set(X, I, "nn")[1:2],
        "min_f_only": _agg_set(X, I, "nn")[2:3],
        "max_i_only": _agg_set(X, I, "nn")[5:6],
        # a live group whose every input is NULL stays, with a NULL sum
        "sum_f_nullable_only": _agg_set(XN, NV, "nu")[:1],
        "sum_i_nullable_only": _agg_set(XN, NV, "nu")[1:2],
    }


LIVE_BYTE = ["sum_i_only", "min_f_only", "max_i_only", "sum_f_nullable_only",
             "sum_i_nullable_only"]


def _expected(p, b, thresh, p_on, b_on, knames, aggs):
    m = (p["f"] < thresh).fillna(False).to_numpy(dtype=bool)
    for c in p_on:
        m &= p[c].notna().to_numpy()
    pf = p[m].copy()
    for c in p_on:
        pf[c] = pf[c].astype(np.int64)
    bb = b.reset_index().rename(columns={"index": "bid"})
    j = pf.merge(bb, left_on=p_on, right_on=b_on, how="inner")
    g = j.groupby("bid", sort=True)
    bids = np.array(sorted(g.groups), dtype=np.int64)
    out = {}
    for kn in knames:
        s = b[kn].iloc[bids]
        out[kn] = s.astype("float64").to_numpy() \
            if pd.api.types.is_extension_array_dtype(s.dtype) \
            else s.to_numpy().astype(np.int64)
    for _, _, _, name, col, red in aggs:
        if col is None:
            out[name] = g.size().to_numpy().astype(np.int64)
        else:
            v = red(g[col])
            out[name] = v.astype("float64").to_numpy() \
                if pd.api.types.is_extension_array_dtype(v.dtype) \
                else v.to_numpy()
    return pd.DataFrame(out, index=None), len(j)


def _run(r, monkeypatch, p, b, aggs, *, interp=False, thresh=50,
         p_on=("k",), b_on=("bk",), ranges=((0, 1500),), knames=("bk",),
         env=None, want_mode=None):
    """filter_probe_groupby over p and b → (frame or None, table mode)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if interp:
        monkeypatch.setenv("DSX_DISABLE_JIT_FPROBE", "1")
    pc = [_upload(r, p[c]) for c in PCOLS]
    bc = {c: _upload(r, b[c]) for c in b.columns}
    bkeys = [bc[c] for c in b_on]
    bspecs = [(j, mn, rng, False) for j, (mn, rng) in enumerate(ranges)]
    bcodes, space = r.keypack(bkeys, bspecs, len(b))
    table = r.hash_build(bcodes, None, code_max=space - 1, key_filter=True)
    pspecs = [(PCOLS.index(c), mn, rng, False)
              for c, (mn, rng) in zip(p_on, ranges)]
    prog = r.make_prog([(OP_COL, F, 0), (OP_LIT_I64, 0, thresh),
                        (OP_LT_I64, 0, 0)])
    specs = [(op, r.make_prog(pr + ([(OP_I64_TO_F64, 0, 0)]
                                   if fin == "avg" and pr[0][1] in (I, NV)
                                   else [])))
             for op, pr, fin, _, _, _ in aggs]
    calls = [(fin, a) for a, (_, _, fin, _, _, _) in enumerate(aggs)]
    jit0 = r.fprobe_agg_jit_launches()
    try:
        mode, _ = r.hash_table_filter(table)
        res = r.filter_probe_groupby(table, prog, pc, pspecs, len(p), specs,
                                     calls, [bc[c] for c in knames])
    finally:
        r.hash_table_free(table)
    if want_mode is not None:
        assert mode == want_mode
    if res is None:
        return None, mode
    kcols, acols, G = res
    # the live-byte layout has no generated form: no row count kept (COUNT
    # or AVG over a never-NULL input) and no never-NULL f64 SUM either
    from dask_sql_amd import runtime as rt_

    def never_null(a):
        return not any(pc[ins[1]].validity for ins in a[1]
                       if ins[0] == OP_COL)

    row_count = any(a[2] in ("count", "avg") and never_null(a) for a in aggs)
    live_sum = any(a[0] == rt_.AGG_SUM_F64 and never_null(a) for a in aggs)
    live_byte = not row_count and not live_sum
    assert r.fprobe_agg_jit_launches() - jit0 == (
        0 if interp or live_byte else 1)
    # cell types: keys widen to i64; COUNT alone carries no validity
    from dask_sql_amd import runtime as rt
    for col, kn in zip(kcols, knames):
        assert col.dtype == rt.I64 and col.len == G
        assert bool(col.validity) == bool(bc[kn].validity)
    for col, (_, _, fin, _, _, _) in zip(acols, aggs):
        assert col.dtype == (rt.F64 if fin in ("sum_f", "min_f", "max_f",
                                                "avg") else rt.I64)
        assert bool(col.validity) == (fin != "count") and col.len == G
    names = list(knames) + [a[3] for a in aggs]
    got = _download(kcols + acols, names)
    assert len(got) == G
    return got, mode


def _check(r, monkeypatch, p, b, aggs, **kw):
    got, _ = _run(r, monkeypatch, p, b, aggs, **kw)
    assert got is not None
    exp, n_join = _expected(
        p, b, kw.get("thresh", 50), list(kw.get("p_on", ("k",))),
        list(kw.get("b_on", ("bk",))), list(kw.get("knames", ("bk",))), aggs)
    assert list(got.columns) == list(exp.columns)
    # rows come out in ascending build row order: compare as they are
    assert_frame_close(got, exp, rel=1e-9)
    return exp, n_join


@SIZES
@FORMS
@pytest.mark.parametrize("which", ["never_null", "nullable", "sum_only"]
                         + LIVE_BYTE)
def test_entry_aggregates(runtime, monkeypatch, n, interp, which):
    rng = np.random.default_rng(300 + n)
    p, b = _probe(n, rng), _build(rng)
    assert p["k"].isna().any()  # NULL probe keys never match
    exp, n_join = _check(runtime, monkeypatch, p, b, _aggs_all()[which],
                         interp=interp, knames=("bk", "b32", "bn"),
                         want_mode=EXACT)
    assert 0 < n_join < n
    if n == 4097:  # build rows with no match are absent
        assert 0 < len(exp) < N_BUILD
    else:
        assert len(exp) == N_BUILD
    if which == "nullable":  # groups whose every input is NULL: NULL cells
        assert exp["sum_f_nu"].isna().any() or n > 4097
        assert (exp["count_nu"] <= exp["count_star"]).all()
    if which.endswith("nullable_only") and n == 4097:
        assert exp.iloc[:, -1].isna().any()  # live, yet nothing to sum


@FORMS
@pytest.mark.parametrize("which", ["sum_only", "sum_i_only",
                                   "sum_f_nullable_only"])
def test_entry_zero_addends(runtime, monkeypatch, interp, which):
    """Groups whose only addends are +0.0 or −0.0 are live groups: the
    liveness sum takes x as x + 0.0, so it leaves its −0.0 start with the
    first row whatever that row holds, and comes out as the +0.0 that a sum
    started at +0.0 gives."""
    rng = np.random.default_rng(317)
    p = _probe(4097, rng, key_lo=3)  # keys 0, 1, 2: the four rows below only
    b = _build(rng)
    for row, (key, x) in enumerate([(0, -0.0), (1, 0.0), (2, -0.0),
                                    (2, -0.0)]):
        p.loc[row, ["k", "f"]] = [key, 0]
        p.loc[row, "x"] = x
        p.loc[row, "i"] = 0
        p.loc[row, "xn"] = x
    assert np.signbit(p["x"].to_numpy()[[0, 2, 3]]).all()
    got, _ = _run(runtime, monkeypatch, p, b, _aggs_all()[which],
                  interp=interp)
    exp, _ = _check(runtime, monkeypatch, p, b, _aggs_all()[which],
                    interp=interp)
    zero = got[got["bk"].isin([0, 1, 2])]
    assert len(zero) == 3 and len(exp[exp["bk"].isin([0, 1, 2])]) == 3
    val = zero.iloc[:, -1].to_numpy(dtype=np.float64)
    assert (val == 0).all() and not np.signbit(val).any()


@FORMS
def test_entry_no_match(runtime, monkeypatch, interp):
    rng = np.random.default_rng(311)
    p, b = _probe(4097, rng, key_lo=1000, key_hi=2500), _build(rng)
    exp, n_join = _check(runtime, monkeypatch, p, b,
                         _aggs_all()["never_null"], interp=interp,
                         ranges=((0, 2500),))
    assert n_join == 0 and len(exp) == 0


@FORMS
def test_entry_every_row_matches(runtime, monkeypatch, interp):
    rng = np.random.default_rng(312)
    p = _probe(65_573, rng, key_hi=N_BUILD, null_keys=False, null_f=False)
    b = _build(rng)
    exp, n_join = _check(runtime, monkeypatch, p, b,
                         _aggs_all()["never_null"], interp=interp, thresh=100)
    assert n_join == len(p) and exp["count_star"].sum() == len(p)


@SIZES
@FORMS
def test_entry_composite_key(runtime, monkeypatch, n, interp):
    rng = np.random.default_rng(313 + n)
    p = _probe(n, rng, key_hi=150)
    b = _build(rng)
    b["bk"] = np.arange(N_BUILD, dtype=np.int64) // 10  # unique as a pair
    b["bk2"] = (np.arange(N_BUILD) % 10).astype(np.int32)
    exp, _ = _check(runtime, monkeypatch, p, b, _aggs_all()["nullable"],
                    interp=interp, p_on=("k", "k2"), b_on=("bk", "bk2"),
                    ranges=((0, 150), (0, 10)), knames=("bk", "bk2", "bn"))
    assert 0 < len(exp) <= N_BUILD


@FORMS
def test_entry_wide_key_range(runtime, monkeypatch, interp):
    """Codes past 2^32: the unpacked table layout (build row ids in their own
    array), which carries no exact bitmap."""
    rng = np.random.default_rng(314)
    p, b = _probe(4097, rng), _build(rng)
    p["k"] = p["k"] * (1 << 23)
    b["bk"] = b["bk"] * (1 << 23)
    got, mode = _run(runtime, monkeypatch, p, b, _aggs_all()["never_null"],
                     interp=interp, ranges=((0, 1500 << 23),))
    assert mode != EXACT
    exp, _ = _check(runtime, monkeypatch, p, b, _aggs_all()["never_null"],
                    interp=interp, ranges=((0, 1500 << 23),))
    assert 0 < len(exp) < N_BUILD


@FORMS
def test_entry_duplicate_build_key_declines(runtime, monkeypatch, interp):
    rng = np.random.default_rng(315)
    p, b = _probe(4097, rng), _build(rng)
    b.loc[7, "bk"] = b.loc[8, "bk"]
    got, _ = _run(runtime, monkeypatch, p, b, _aggs_all()["never_null"],
                  interp=interp)
    assert got is None


@FORMS
@pytest.mark.parametrize("env, mode", [
    ({}, EXACT),
    ({"DSX_JOIN_FILTER_MAX_BYTES": "64", "DSX_JOIN_FILTER_MIN_BITS": "0"},
     HASHED),
    ({"DSX_DISABLE_JOINFILTER": "1"}, NONE),
], ids=["exact", "hashed", "none"])
def test_entry_join_filter_modes(runtime, monkeypatch, interp, env, mode):
    rng = np.random.default_rng(316)
    p, b = _probe(4097, rng), _build(rng)
    exp, _ = _check(runtime, monkeypatch, p, b, _aggs_all()["nullable"],
                    interp=interp, env=env, want_mode=mode,
                    knames=("bk", "bn"))
    assert 0 < len(exp) < N_BUILD


# ---------------------------------------------------------------------------
# SQL level
# ---------------------------------------------------------------------------
def _launches(prof, name):
    return prof.get(name, {}).get("launches", 0)


def _family(prof, prefix):
    return sum(v.get("launches", 0) for k, v in prof.items()
               if k.startswith(prefix))


def _norm(df):
    out = {}
    for c in df.columns:
        s = df[c]
        if pd.api.types.is_extension_array_dtype(s.dtype):
            out[c] = s.astype("float64")
        elif np.issubdtype(s.dtype, np.datetime64):
            out[c] = s.to_numpy().astype("datetime64[D]").astype(np.int64)
        else:
            out[c] = s
    return pd.DataFrame(out).reset_index(drop=True)


def _sql_both(monkeypatch, ctx, sql, min_rows="0"):
    """(group-join frame, its prof, DSX_DISABLE_GROUPJOIN=1 frame, its
    prof); the two frames must agree on columns, dtypes and values."""
    r = ctx._get_runtime()
    r.prof_enable(True)
    res = []
    for off in (False, True):
        monkeypatch.delenv("DSX_DISABLE_GROUPJOIN", raising=False)
        monkeypatch.delenv("DSX_GROUPJOIN_MIN_ROWS", raising=False)
        if off:
            monkeypatch.setenv("DSX_DISABLE_GROUPJOIN", "1")
        elif min_rows is not None:
            monkeypatch.setenv("DSX_GROUPJOIN_MIN_ROWS", min_rows)
        r.prof_reset()
        res += [ctx.sql(sql).compute(), r.prof_get()]
    monkeypatch.delenv("DSX_DISABLE_GROUPJOIN", raising=False)
    monkeypatch.delenv("DSX_GROUPJOIN_MIN_ROWS", raising=False)
    r.prof_enable(False)
    got, prof, off, prof_off = res
    assert _launches(prof_off, "k_fprobe_agg") == 0, "knob must disable"
    assert list(got.columns) == list(off.columns)
    assert [str(t) for t in got.dtypes] == [str(t) for t in off.dtypes]
    return got, prof, off, prof_off


@pytest.fixture(scope="module")
def q3_ctx(runtime):
    from dask_sql_amd.context import Context
    from datagen import gen_q3, register_q3_tables
    frames = gen_q3(sf_rows=(1_500, 15_000, 60_000))
    c = Context()
    register_q3_tables(c, *frames)
    return c, frames


def test_q3_mini_group_join(q3_ctx, monkeypatch):
    from datagen import Q3_SQL
    from oracle.tpch import oracle_q3
    c, (cust, orders, li) = q3_ctx
    # the whole group-by, before ORDER BY ... LIMIT cuts it to ten rows
    sql = Q3_SQL[:Q3_SQL.index("ORDER BY")]
    got, prof, off, prof_off = _sql_both(monkeypatch, c, sql)
    assert _launches(prof, "k_fprobe_mask") == 2  # orders and lineitem
    assert _launches(prof, "k_fprobe_emit") == 1  # orders only
    assert _launches(prof, "k_fprobe_agg") == 1
    assert _family(prof, "k_gbpart") == 0
    assert _family(prof, "k_groupby") == 0
    assert _launches(prof_off, "k_fprobe_emit") == 2
    assert len(got) > 100
    assert_frame_close(_norm(got), _norm(off), rel=1e-9,
                       sort_by=["l_orderkey"])
    # and the query as the benchmark runs it, against the oracle
    got, prof, off, _ = _sql_both(monkeypatch, c, Q3_SQL)
    assert _launches(prof, "k_fprobe_agg") == 1
    exp = oracle_q3(cust, orders, li)
    assert len(got) == len(exp) == len(off)
    assert (got["l_orderkey"].to_numpy().astype(np.int64)
            == exp["l_orderkey"].to_numpy()).all()
    assert np.allclose(got["revenue"], exp["revenue"], rtol=1e-9)
    days = got["o_orderdate"].to_numpy().astype("datetime64[D]").astype(
        np.int64)
    assert (days == exp["o_orderdate"].to_numpy()).all()
    assert_frame_close(_norm(got), _norm(off), rel=1e-9)


def test_q3_mini_default_threshold_keeps_the_join(q3_ctx, monkeypatch):
    """60 000 lineitem rows are under DSX_GROUPJOIN_MIN_ROWS' default."""
    from datagen import Q3_SQL
    c, _ = q3_ctx
    got, prof, off, _ = _sql_both(monkeypatch, c, Q3_SQL, min_rows=None)
    assert _launches(prof, "k_fprobe_agg") == 0
    assert _launches(prof, "k_fprobe_emit") == 2
    assert_frame_close(_norm(got), _norm(off), rel=1e-9)


@pytest.fixture(scope="module")
def pb_ctx(runtime):
    from dask_sql_amd.context import Context
    rng = np.random.default_rng(320)
    p = _probe(30_011, rng)
    b = _build(rng)
    bd = b.copy()
    bd.loc[7, "bk"] = bd.loc[8, "bk"]
    c = Context()
    c.create_table("p", p)
    c.create_table("b", b)
    c.create_table("bd", bd)
    return c, p, b, bd


def _pandas_group(p, b, aggs):
    m = (p["f"] < 50).fillna(False) & p["k"].notna()
    pf = p[m.to_numpy(dtype=bool)].copy()
    pf["k"] = pf["k"].astype(np.int64)
    j = pf.merge(b, left_on="k", right_on="bk")
    return j.groupby(["bk", "b32"], as_index=False).agg(**aggs)


def test_sql_avg_count_shape(pb_ctx, monkeypatch):
    c, p, b, _ = pb_ctx
    sql = ("SELECT b.bk, b.b32, AVG(p.x) AS ax, COUNT(*) AS c, "
           "COUNT(p.nv) AS cn, SUM(p.nv) AS sn, MIN(p.xn) AS mx "
           "FROM p JOIN b ON p.k = b.bk WHERE p.f < 50 GROUP BY b.bk, b.b32")
    got, prof, off, _ = _sql_both(monkeypatch, c, sql)
    assert _launches(prof, "k_fprobe_agg") == 1
    assert _launches(prof, "k_fprobe_emit") == 0
    exp = _pandas_group(p, b, dict(
        ax=("x", "mean"), c=("x", "size"), cn=("nv", "count"),
        sn=("nv", lambda s: s.sum(min_count=1)), mx=("xn", "min")))
    assert 0 < len(exp) <= N_BUILD
    assert_frame_close(_norm(got), _norm(off), rel=1e-9, sort_by=["bk"])
    assert_frame_close(_norm(got), _norm(exp), rel=1e-9, sort_by=["bk"])


def test_sql_duplicate_build_key_falls_back(pb_ctx, monkeypatch):
    c, p, _, bd = pb_ctx
    sql = ("SELECT p.k, SUM(p.x) AS sx, COUNT(*) AS c FROM p JOIN bd "
           "ON p.k = bd.bk WHERE p.f < 50 GROUP BY p.k")
    got, prof, off, prof_off = _sql_both(monkeypatch, c, sql)
    # the attempt ran, declined, and the join probed the two-pass way
    assert _launches(prof, "k_fprobe_agg") == 1
    assert _launches(prof, "k_hash_probe_count") == 1
    assert _launches(prof_off, "k_hash_probe_count") == 1
    m = (p["f"] < 50).fillna(False) & p["k"].notna()
    pf = p[m.to_numpy(dtype=bool)].copy()
    pf["k"] = pf["k"].astype(np.int64)
    j = pf.merge(bd, left_on="k", right_on="bk")
    exp = j.groupby("k", as_index=False).agg(sx=("x", "sum"),
                                             c=("x", "size"))
    assert_frame_close(_norm(got), _norm(off), rel=1e-9, sort_by=["k"])
    assert_frame_close(_norm(got), _norm(exp), rel=1e-9, sort_by=["k"])


@pytest.mark.parametrize("sql", [
    # grouped by a probe-side column that is no join key
    "SELECT p.k2, SUM(p.x) AS sx FROM p JOIN b ON p.k = b.bk "
    "WHERE p.f < 50 GROUP BY p.k2",
    # an aggregate over a build-side column
    "SELECT b.bk, SUM(b.b32) AS sb FROM p JOIN b ON p.k = b.bk "
    "WHERE p.f < 50 GROUP BY b.bk",
], ids=["probe_group_key", "build_aggregate"])
def test_sql_ineligible_shapes_keep_the_join(pb_ctx, monkeypatch, sql):
    c = pb_ctx[0]
    got, prof, off, _ = _sql_both(monkeypatch, c, sql)
    assert _launches(prof, "k_fprobe_agg") == 0
    assert _launches(prof, "k_fprobe_emit") == 1
    assert len(got) > 0
    assert_frame_close(_norm(got), _norm(off), rel=1e-9,
                       sort_by=[got.columns[0]])
