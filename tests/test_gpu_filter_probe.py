"""Fused scan filter + key pack + probe for PK-FK inner joins
(dsx_filter_probe_cols, -m gpu).

Every case is compared with two things after sorting: the oracle join
(oracle/frame.py) over pandas-filtered inputs, and the same work with the
fusion off — the same query under DSX_DISABLE_FILTERPROBE=1, or, where the
planner cannot reach the entry (an inner join probes with its LARGER side,
so a probe side of fewer rows than the 1 000-row build side never gets
there through SQL), the separate dsx_filter_cols → dsx_keypack →
dsx_hash_probe_cols calls on the same columns."""
import numpy as np
import pandas as pd
import pytest

from tests.conftest import assert_frame_close

pytestmark = pytest.mark.gpu

N_BUILD = 1000
# VM opcodes (include/dsxhip.h DsxOp)
OP_COL, OP_LIT_I64, OP_LT_I64, OP_IS_NOT_NULL = 1, 3, 30, 44


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _norm(df):
    """Comparable plain-numpy frame: strings as str, nullable → float/NaN."""
    out = {}
    for c in df.columns:
        s = df[c]
        if isinstance(s.dtype, pd.CategoricalDtype) or s.dtype == object:
            out[c] = s.astype(object).where(s.notna(), "<NULL>").astype(str)
        elif pd.api.types.is_extension_array_dtype(s.dtype):
            out[c] = s.astype("float64")
        else:
            out[c] = s
    return pd.DataFrame(out).reset_index(drop=True)


def _oracle(p, b, mask, p_on, b_on, sel):
    from oracle.frame import oracle_filter, oracle_join
    j = oracle_join(oracle_filter(p, mask), b,
                    [p.columns.get_loc(c) for c in p_on],
                    [b.columns.get_loc(c) for c in b_on])
    j.columns = list(p.columns) + list(b.columns)
    return j[sel]


def _launches(prof, name):
    return prof.get(name, {}).get("launches", 0)


def _sql_both(monkeypatch, tables, sql, **kw):
    """(fused frame, fused prof, unfused frame, unfused prof)."""
    from dask_sql_amd.context import Context
    c = Context()
    for name, df in tables.items():
        c.create_table(name, df, **kw.get(name, {}))
    r = c._get_runtime()
    r.prof_enable(True)
    res = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("DSX_DISABLE_FILTERPROBE", "1")
        else:
            monkeypatch.delenv("DSX_DISABLE_FILTERPROBE", raising=False)
        r.prof_reset()
        res += [c.sql(sql).compute(), r.prof_get()]
    monkeypatch.delenv("DSX_DISABLE_FILTERPROBE", raising=False)
    r.prof_enable(False)
    assert _launches(res[3], "k_fprobe_mask") == 0, "knob must disable"
    return tuple(res)


def _probe_frame(n, rng, key_hi=1500, null_keys=True):
    """Probe table: rid (row id), k (join key, nullable), f (nullable
    predicate column, uniform 0..99), payload of every jm_write dtype."""
    k = pd.array(rng.integers(0, key_hi, n), dtype="Int64")
    if null_keys and n:
        k[rng.random(n) < 0.05] = pd.NA
    f = pd.array(rng.integers(0, 100, n), dtype="Int64")
    if n:
        f[rng.random(n) < 0.1] = pd.NA
    nv = pd.array(rng.integers(0, 1000, n), dtype="Int64")
    if n:
        nv[rng.random(n) < 0.2] = pd.NA
    return pd.DataFrame({
        "rid": np.arange(n, dtype=np.int64),
        "k": k,
        "f": f,
        "x": rng.random(n),
        "d32": rng.integers(0, 10_000, n).astype(np.int32),
        "c8": rng.integers(-100, 100, n).astype(np.int8),
        "s": pd.Series(rng.choice(["aa", "bb", "cc"], n),
                       dtype=object).astype("category"),
        "nv": nv,
    })


def _build_frame(rng, n=N_BUILD):
    bn = pd.array(rng.integers(0, 50, n), dtype="Int64")
    bn[rng.random(n) < 0.3] = pd.NA
    return pd.DataFrame({
        "bk": rng.permutation(n).astype(np.int64),  # unique keys
        "bv": rng.integers(0, 1 << 40, n).astype(np.int64),
        "bf": rng.random(n),
        "b32": rng.integers(0, 100, n).astype(np.int32),
        "bs": pd.Series(rng.choice(["u", "v"], n),
                        dtype=object).astype("category"),
        "bn": bn,
    })


SEL = ["rid", "k", "x", "d32", "c8", "s", "nv", "bk", "bv", "bf", "b32",
       "bs", "bn"]
SQL = ("SELECT p.rid, p.k, p.x, p.d32, p.c8, p.s, p.nv, b.bk, b.bv, b.bf, "
       "b.b32, b.bs, b.bn FROM p JOIN b ON p.k = b.bk WHERE p.f < {t}")


def _mask(p, t):
    return (p["f"] < t).fillna(False).to_numpy(dtype=bool)


# ---------------------------------------------------------------------------
# SQL level: planner → deferred filter → fused probe
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,thresh", [
    (100_003, 50),     # ~half
    (100_003, -1),     # none
    (100_003, 1000),   # all (NULL predicate rows still drop)
    (1_500_007, 50),   # > 2048 blocks' worth of words + ragged tail
])
def test_sql_selectivity_and_sizes(gpu, monkeypatch, n, thresh):
    rng = np.random.default_rng(n + thresh)
    p, b = _probe_frame(n, rng), _build_frame(rng)
    got, prof, off, _ = _sql_both(monkeypatch, {"p": p, "b": b},
                                  SQL.format(t=thresh))
    assert _launches(prof, "k_fprobe_mask") == 1
    assert _launches(prof, "k_hash_probe_count") == 0
    exp = _oracle(p, b, _mask(p, thresh), ["k"], ["bk"], SEL)
    if thresh == 1000:
        assert len(exp) > 0.5 * n
    if thresh == -1:
        assert len(exp) == 0 and _launches(prof, "k_fprobe_emit") == 0
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid"])


def test_sql_every_key_present(gpu, monkeypatch):
    rng = np.random.default_rng(11)
    p = _probe_frame(20_011, rng, key_hi=N_BUILD, null_keys=False)
    b = _build_frame(rng)
    got, prof, off, _ = _sql_both(monkeypatch, {"p": p, "b": b},
                                  SQL.format(t=50))
    assert _launches(prof, "k_fprobe_mask") == 1
    exp = _oracle(p, b, _mask(p, 50), ["k"], ["bk"], SEL)
    assert len(exp) == int(_mask(p, 50).sum())  # every surviving row matches
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid"])


def test_sql_composite_key(gpu, monkeypatch):
    rng = np.random.default_rng(12)
    n = 30_011
    p = _probe_frame(n, rng)
    p["k2"] = rng.integers(0, 40, n).astype(np.int64)
    p["k"] = pd.array(rng.integers(0, 50, n), dtype="Int64")
    p.loc[rng.random(n) < 0.05, "k"] = pd.NA
    pairs = rng.permutation(50 * 40)[:N_BUILD]
    b = _build_frame(rng)
    b["bk"] = (pairs // 40).astype(np.int64)
    b["bk2"] = (pairs % 40).astype(np.int64)
    sql = ("SELECT p.rid, p.k, p.k2, p.x, b.bk, b.bk2, b.bv FROM p JOIN b "
           "ON p.k = b.bk AND p.k2 = b.bk2 WHERE p.f < 50")
    got, prof, off, _ = _sql_both(monkeypatch, {"p": p, "b": b}, sql)
    assert _launches(prof, "k_fprobe_mask") == 1
    exp = _oracle(p, b, _mask(p, 50), ["k", "k2"], ["bk", "bk2"],
                  ["rid", "k", "k2", "x", "bk", "bk2", "bv"])
    assert 0 < len(exp) < n
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid"])


def test_sql_unpacked_layout(gpu, monkeypatch):
    """Key range ≥ 2^32 → (code, row id) no longer fit one table word."""
    rng = np.random.default_rng(13)
    n = 30_011
    big = 1 << 33
    p = _probe_frame(n, rng)
    far = rng.random(n) < 0.1
    p["k"] = pd.array(np.where(far, big, rng.integers(0, 1500, n)),
                      dtype="Int64")
    p.loc[rng.random(n) < 0.05, "k"] = pd.NA
    b = _build_frame(rng)
    b.loc[0, "bk"] = big  # replaces one key, still unique
    got, prof, off, _ = _sql_both(monkeypatch, {"p": p, "b": b},
                                  SQL.format(t=50))
    assert _launches(prof, "k_fprobe_mask") == 1
    exp = _oracle(p, b, _mask(p, 50), ["k"], ["bk"], SEL)
    assert (exp["bk"] == big).sum() > 0
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid"])


def test_sql_duplicate_build_key_falls_back(gpu, monkeypatch):
    rng = np.random.default_rng(14)
    p, b = _probe_frame(30_011, rng), _build_frame(rng)
    b.loc[1, "bk"] = b.loc[0, "bk"]  # one duplicate key
    got, prof, off, _ = _sql_both(monkeypatch, {"p": p, "b": b},
                                  SQL.format(t=50))
    assert _launches(prof, "k_fprobe_mask") == 1       # tried …
    assert _launches(prof, "k_fprobe_emit") == 0       # … not applicable
    assert _launches(prof, "k_hash_probe_count") == 1  # two-pass probe ran
    exp = _oracle(p, b, _mask(p, 50), ["k"], ["bk"], SEL)
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid", "bv"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid", "bv"])


def test_sql_stacked_filters(gpu, monkeypatch):
    """Two WHEREs over the scan (derived table) combine as a conjunction."""
    rng = np.random.default_rng(15)
    p, b = _probe_frame(30_011, rng), _build_frame(rng)
    sql = ("SELECT q.rid, q.k, q.nv, b.bv FROM "
           "(SELECT * FROM p WHERE f < 70) q JOIN b ON q.k = b.bk "
           "WHERE q.d32 < 5000")
    got, prof, off, _ = _sql_both(monkeypatch, {"p": p, "b": b}, sql)
    m = _mask(p, 70) & (p["d32"] < 5000).to_numpy()
    exp = _oracle(p, b, m, ["k"], ["bk"], ["rid", "k", "nv", "bv"])
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid"])


def test_lazy_filter_without_join(gpu, monkeypatch):
    rng = np.random.default_rng(16)
    p = _probe_frame(30_011, rng)
    m = _mask(p, 50)
    got, prof, off, _ = _sql_both(
        monkeypatch, {"p": p}, "SELECT rid, x + 1 AS y, nv FROM p WHERE f < 50")
    assert _launches(prof, "k_fprobe_mask") == 0
    exp = pd.DataFrame({"rid": p["rid"][m], "y": p["x"][m] + 1,
                        "nv": p["nv"][m]})
    assert_frame_close(_norm(got), _norm(exp))  # filter keeps row order
    assert_frame_close(_norm(got), _norm(off))
    got, _, off, _ = _sql_both(
        monkeypatch, {"p": p},
        "SELECT c8, COUNT(*) AS c, SUM(x) AS sx FROM p WHERE f < 50 "
        "GROUP BY c8")
    g = p[m].groupby("c8")
    exp = pd.DataFrame({"c8": list(g.groups), "c": g.size().to_numpy(),
                        "sx": g["x"].sum().to_numpy()})
    assert_frame_close(_norm(got), _norm(exp), sort_by=["c8"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["c8"])


def test_filtered_table_as_build_side(gpu, monkeypatch):
    rng = np.random.default_rng(17)
    p, b = _probe_frame(30_011, rng), _build_frame(rng)
    sql = ("SELECT p.rid, p.k, b.bk, b.bv FROM p JOIN b ON p.k = b.bk "
           "WHERE b.b32 < 50")
    got, prof, off, _ = _sql_both(monkeypatch, {"p": p, "b": b}, sql)
    assert _launches(prof, "k_fprobe_mask") == 0  # unfiltered probe side
    bm = b[b["b32"] < 50]
    exp = _oracle(p, bm, np.ones(len(p), dtype=bool), ["k"], ["bk"],
                  ["rid", "k", "bk", "bv"])
    assert 0 < len(exp)
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid"])


def test_q3_mini(gpu, monkeypatch):
    from dask_sql_amd.context import Context
    from datagen import Q3_SQL, gen_q3, register_q3_tables
    from oracle.tpch import oracle_q3
    cust, orders, li = gen_q3(sf_rows=(1_500, 15_000, 60_000))
    c = Context()
    register_q3_tables(c, cust, orders, li)
    r = c._get_runtime()
    monkeypatch.delenv("DSX_DISABLE_FILTERPROBE", raising=False)
    r.prof_enable(True)
    r.prof_reset()
    out = c.sql(Q3_SQL).compute()
    prof = r.prof_get()
    r.prof_enable(False)
    assert _launches(prof, "k_fprobe_mask") == 2  # orders and lineitem
    assert _launches(prof, "k_fprobe_emit") == 2
    assert _launches(prof, "k_keypack") == 2      # the two BUILD sides only
    assert _launches(prof, "k_hash_probe_count") == 0
    exp = oracle_q3(cust, orders, li)
    assert len(out) == len(exp)
    assert (out["l_orderkey"].to_numpy().astype(np.int64)
            == exp["l_orderkey"].to_numpy()).all()
    assert np.allclose(out["revenue"], exp["revenue"], rtol=1e-9)
    days = out["o_orderdate"].to_numpy().astype("datetime64[D]").astype(
        np.int64)
    assert (days == exp["o_orderdate"].to_numpy()).all()


# ---------------------------------------------------------------------------
# entry level: probe sides smaller than the build side, every tail shape
# ---------------------------------------------------------------------------
def _upload(r, s):
    from dask_sql_amd import runtime as rt
    if pd.api.types.is_extension_array_dtype(s.dtype):
        valid = (~s.isna()).to_numpy()
        return r.upload_column(s.fillna(0).to_numpy(dtype=np.int64),
                               valid.astype(np.uint8) if len(s) else None,
                               rt.I64)
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


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 100_003, 1_500_007])
def test_entry_row_counts(gpu, n):
    from dask_sql_amd import runtime as rt
    from dask_sql_amd.context import Context
    r = Context()._get_runtime()
    rng = np.random.default_rng(100 + n)
    p = _probe_frame(n, rng)[["rid", "k", "f", "x", "nv"]]
    b = _build_frame(rng)[["bk", "bv", "bn"]]
    pc = {c: _upload(r, p[c]) for c in p.columns}
    bc = {c: _upload(r, b[c]) for c in b.columns}
    prog = r.make_prog([(OP_COL, 0, 0), (OP_LIT_I64, 0, 50),
                        (OP_LT_I64, 0, 0)])
    mn, rng_ = 0, 1500
    bcodes, space = r.keypack([bc["bk"]], [(0, mn, rng_, False)], N_BUILD)
    table = r.hash_build(bcodes, None, code_max=space - 1)
    names = ["rid", "x", "nv", "bv", "bn"]
    try:
        # fused: predicate column 0, key column 1 of one shared list
        res = r.filter_probe_cols(
            table, prog, [pc["f"], pc["k"]], [(1, mn, rng_, False)], n,
            [pc["rid"], pc["x"], pc["nv"]], [bc["bv"], bc["bn"]])
        assert res is not None
        got = _download(res[0], names)
        assert res[1] == len(got)
        # separate passes on the same columns
        mats = [pc["rid"], pc["x"], pc["nv"], pc["k"]]
        fcols, nf = r.filter_cols(prog, [pc["f"]], n, mats)
        kcodes, _ = r.keypack([fcols[3]], [(0, mn, rng_, False)], nf)
        kval = r.eval(r.make_prog([(OP_COL, 0, 0), (OP_IS_NOT_NULL, 0, 0)]),
                      [fcols[3]], nf, rt.BOOL8, with_validity=False)
        ucols, nu = r.hash_probe_cols(table, kcodes, rt.JOIN_INNER,
                                      kval.data, fcols[:3],
                                      [bc["bv"], bc["bn"]], False)
        off = _download(ucols, names)
    finally:
        r.hash_table_free(table)
    exp = _oracle(p, b, _mask(p, 50), ["k"], ["bk"], names)
    if n >= 1000:
        assert 0 < len(exp) < n
    # deterministic order: increasing probe row
    assert (np.diff(got["rid"].to_numpy()) > 0).all()
    assert_frame_close(got, _norm(exp), sort_by=["rid"])
    assert_frame_close(got, off, sort_by=["rid"])
