"""GPU tests (-m gpu) of the ORDER BY ... LIMIT row selection:

- Runtime.topk_rows (dsx_topk_rows, csrc/topk.inc) directly against numpy:
  the returned rows are exactly those whose primary key sorts at or before
  the k-th row's, each with every column's value and validity byte;
- the SQL route through it against the sampled-threshold path
  (DSX_DISABLE_TOPK=1) and pandas' stable sort, with the kernel families
  each route launches;
- the hash table's match marks, allocated on first use: INNER, LEFT and FULL
  OUTER joins and hash_unmatched against pandas merge.
"""
import numpy as np
import pandas as pd
import pytest

from dask_sql_amd import runtime as rt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    return Context()


@pytest.fixture
def prof(ctx):
    runtime = ctx._get_runtime()
    runtime.prof_enable(True)
    runtime.prof_reset()

    def read():
        p = runtime.prof_get()
        runtime.prof_reset()
        return {k: v["launches"] for k, v in p.items()}

    yield read
    runtime.prof_enable(False)
    runtime.prof_reset()


def _cap(k):
    return min(4096, max(4 * k, 1024))


def _key(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "f64":  # ties: about 3 rows per value at the largest n
        return np.round(rng.random(n) * 2e4 - 1e4, 1)
    if kind == "i64":
        return rng.integers(-2**40, 2**40, n, dtype=np.int64)
    return rng.integers(-50_000, 50_000, n).astype(np.int32)


def _payload(n, seed):
    """One column of each dtype the call carries, two with validity."""
    rng = np.random.default_rng(seed + 1)
    return [
        (np.arange(n, dtype=np.int64) * 3 - 7, None),
        (rng.standard_normal(n), (rng.random(n) > 0.3).astype(np.uint8)),
        (rng.integers(-2**31, 2**31 - 1, n).astype(np.int32), None),
        (rng.standard_normal(n).astype(np.float32), None),
        (rng.integers(-128, 128, n).astype(np.int8),
         (rng.random(n) > 0.5).astype(np.uint8)),
    ]


def _upload(runtime, host_cols):
    return [runtime.upload_column(a, validity=v) for a, v in host_cols]


def _expected_set(key, k, desc):
    if desc:
        kth = np.sort(key)[::-1][k - 1]
        return np.nonzero(key >= kth)[0]
    kth = np.sort(key)[k - 1]
    return np.nonzero(key <= kth)[0]


def _check(res, host_cols, key, k, cap, desc):
    assert res is not None
    rowids, cols = res
    assert len(np.unique(rowids)) == len(rowids)
    assert k <= len(rowids) <= cap
    exp = _expected_set(key, k, desc)
    assert np.array_equal(np.sort(rowids.astype(np.int64)), exp)
    assert len(cols) == len(host_cols)
    for (vals, valid), (src, srcv) in zip(cols, host_cols):
        assert vals.dtype == src.dtype
        assert vals.tobytes() == src[rowids].tobytes()
        if srcv is None:
            assert valid is None
        else:
            assert np.array_equal(valid, srcv[rowids].astype(bool))


@pytest.mark.parametrize("kind", ["f64", "i64", "i32"])
@pytest.mark.parametrize("n", [4097, 65573, 300001])
def test_topk_rows_equals_numpy(ctx, n, kind):
    runtime = ctx._get_runtime()
    key = _key(kind, n, seed=n)
    host_cols = [(key, None)] + _payload(n, seed=n)
    dev = _upload(runtime, host_cols)
    for k in (1, 10, 1000):
        for desc in (False, True):
            res = runtime.topk_rows(dev, 0, desc, n, k, _cap(k))
            _check(res, host_cols, key, k, _cap(k), desc)


def test_topk_rows_key_in_the_middle_with_all_valid_validity(ctx):
    """The key need not be column 0, and a validity buffer of all ones on
    the key does not make the call decline."""
    runtime = ctx._get_runtime()
    n = 65573
    key = _key("f64", n, seed=5)
    host_cols = _payload(n, seed=5)
    host_cols.insert(2, (key, np.ones(n, dtype=np.uint8)))
    dev = _upload(runtime, host_cols)
    res = runtime.topk_rows(dev, 2, True, n, 10, _cap(10))
    _check(res, host_cols, key, 10, _cap(10), True)


def test_topk_rows_keys_differ_in_lowest_byte_only(ctx):
    """Every digit pass runs: the keys share all but their lowest 8 bits."""
    runtime = ctx._get_runtime()
    n = 65573
    rng = np.random.default_rng(3)
    key = (np.int64(0x1234_5678_9ABC_DE00)
           + rng.integers(0, 256, n).astype(np.int64))
    key[rng.choice(n, 5, replace=False)] = np.int64(0x1234_5678_9ABC_DE00) - 1
    host_cols = [(key, None)] + _payload(n, seed=3)
    dev = _upload(runtime, host_cols)
    for desc in (False, True):
        # 65573 / 256 = 256 rows per value: they fit the cap of 1024
        res = runtime.topk_rows(dev, 0, desc, n, 10, 1024)
        _check(res, host_cols, key, 10, 1024, desc)


def test_topk_rows_all_equal_key_is_not_applicable(ctx):
    runtime = ctx._get_runtime()
    n = 5000
    dev = _upload(runtime, [(np.full(n, 2.5), None)])
    assert runtime.topk_rows(dev, 0, False, n, 10, 1024) is None
    assert runtime.topk_rows(dev, 0, True, n, 10, 1024) is None


@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_topk_rows_ties_at_the_cap(ctx, kind):
    """3 rows before a tie group that crosses the k-th position: with
    cap - 3 ties the candidates fit the cap exactly, with one more they do
    not."""
    runtime = ctx._get_runtime()
    n, k, cap = 6001, 10, 1024
    dt = np.float64 if kind == "f64" else np.int64
    rng = np.random.default_rng(9)
    for extra, applicable in ((0, True), (1, False)):
        key = (1000 + rng.integers(0, 10**6, n)).astype(dt)
        pos = rng.permutation(n)
        key[pos[:3]] = np.array([1, 2, 3], dtype=dt)
        key[pos[3:cap + extra]] = dt(500)
        host_cols = [(key, None), (np.arange(n, dtype=np.int64), None)]
        dev = _upload(runtime, host_cols)
        res = runtime.topk_rows(dev, 0, False, n, k, cap)
        if applicable:
            _check(res, host_cols, key, k, cap, False)
            assert len(res[0]) == cap
        else:
            assert res is None


def test_topk_rows_nan_or_null_key_is_not_applicable(ctx):
    runtime = ctx._get_runtime()
    n = 65573
    key = _key("f64", n, seed=1)
    assert runtime.topk_rows(_upload(runtime, [(key, None)]), 0, True, n, 10,
                             1024) is not None
    bad = key.copy()
    bad[n - 7] = np.nan
    assert runtime.topk_rows(_upload(runtime, [(bad, None)]), 0, True, n, 10,
                             1024) is None
    valid = np.ones(n, dtype=np.uint8)
    valid[4100] = 0
    for kind in ("f64", "i64"):
        kk = _key(kind, n, seed=2)
        assert runtime.topk_rows(_upload(runtime, [(kk, valid)]), 0, False, n,
                                 10, 1024) is None


# ---- SQL ------------------------------------------------------------------

def _frame(n, seed=0):
    rng = np.random.default_rng(seed)
    return pd.DataFrame({
        "a": np.arange(n, dtype=np.int64),
        "v": rng.random(n) * 1e5,
        "t": rng.integers(0, 1000, n).astype(np.int64),
        "d": (np.datetime64("1995-01-01")
              + rng.integers(0, 2000, n).astype("timedelta64[D]")
              ).astype("datetime64[ns]"),
        "g": np.round(rng.random(n) * 100, 1),
    })


QUERIES = [
    ("SELECT a, v, t FROM {t} ORDER BY v DESC, t LIMIT 25",
     ["a", "v", "t"], ["v", "t"], [False, True], 0, 25),
    ("SELECT a, t FROM {t} ORDER BY t LIMIT 7 OFFSET 3",
     ["a", "t"], ["t"], [True], 3, 7),
    ("SELECT a, d, v FROM {t} ORDER BY d DESC, v LIMIT 25",
     ["a", "d", "v"], ["d", "v"], [False, True], 0, 25),
    ("SELECT a, g FROM {t} ORDER BY g LIMIT 25",
     ["a", "g"], ["g"], [True], 0, 25),
]


@pytest.fixture(scope="module")
def sql_tables(ctx):
    frames = {}
    for n in (5000, 200_000):
        frames[n] = _frame(n, seed=n)
        ctx.create_table(f"tk{n}", frames[n])
    return frames


@pytest.mark.parametrize("qi", range(len(QUERIES)))
@pytest.mark.parametrize("n", [5000, 200_000])
def test_sql_topk_equals_old_path_and_pandas(ctx, sql_tables, prof,
                                             monkeypatch, n, qi):
    sql, cols, by, asc, offset, fetch = QUERIES[qi]
    sql = sql.format(t=f"tk{n}")
    monkeypatch.delenv("DSX_DISABLE_TOPK", raising=False)
    prof()
    got = ctx.sql(sql).compute()
    p = prof()
    assert p.get("k_topk_select", 0) >= 1 and p.get("k_topk_emit", 0) >= 1, p
    assert "k_filter_mask" not in p and "k_gather" not in p, p
    monkeypatch.setenv("DSX_DISABLE_TOPK", "1")
    old = ctx.sql(sql).compute()
    p = prof()
    assert not [f for f in p if f.startswith("k_topk")], p
    assert "k_filter_mask" in p and "k_gather" in p, p
    pd.testing.assert_frame_equal(got, old)
    exp = sql_tables[n].sort_values(by, ascending=asc, kind="mergesort")
    exp = exp.iloc[offset:offset + fetch][cols].reset_index(drop=True)
    pd.testing.assert_frame_equal(got.reset_index(drop=True), exp,
                                  check_dtype=False)


def test_sql_fallbacks_take_the_old_kernels(ctx, sql_tables, prof,
                                            monkeypatch):
    monkeypatch.delenv("DSX_DISABLE_TOPK", raising=False)
    n = 200_000
    df = sql_tables[n]
    # k above 1024
    prof()
    got = ctx.sql(f"SELECT a, v FROM tk{n} ORDER BY v DESC LIMIT 2000"
                  ).compute()
    p = prof()
    assert not [f for f in p if f.startswith("k_topk")], p
    assert "k_filter_mask" in p and "k_gather" in p, p
    exp = df.sort_values("v", ascending=False, kind="mergesort")
    pd.testing.assert_frame_equal(
        got.reset_index(drop=True),
        exp.iloc[:2000][["a", "v"]].reset_index(drop=True), check_dtype=False)
    # dictionary sort key
    sdf = pd.DataFrame({"a": np.arange(n, dtype=np.int64),
                        "s": np.array(["apple", "fig", "kiwi", "pear"]
                                      )[np.arange(n) % 4]})
    ctx.create_table("tk_dict", sdf)
    prof()
    got = ctx.sql("SELECT a, s FROM tk_dict ORDER BY s, a LIMIT 5").compute()
    p = prof()
    assert not [f for f in p if f.startswith("k_topk")], p
    exp = sdf.sort_values(["s", "a"], kind="mergesort").iloc[:5]
    pd.testing.assert_frame_equal(got.reset_index(drop=True),
                                  exp.reset_index(drop=True),
                                  check_dtype=False)
    # one NaN in the primary key: the select counts it in its first pass
    # and declines (so k_topk_select does launch); the old kernels then run
    ndf = df[["a", "v"]].copy()
    ndf.loc[n - 11, "v"] = np.nan
    ctx.create_table("tk_nan", ndf)
    prof()
    got = ctx.sql("SELECT a, v FROM tk_nan ORDER BY v DESC LIMIT 25"
                  ).compute()
    p = prof()
    assert "k_filter_mask" in p and "k_gather" in p, p
    monkeypatch.setenv("DSX_DISABLE_TOPK", "1")
    old = ctx.sql("SELECT a, v FROM tk_nan ORDER BY v DESC LIMIT 25"
                  ).compute()
    p = prof()
    assert not [f for f in p if f.startswith("k_topk")], p
    pd.testing.assert_frame_equal(got, old)


# ---- match marks ------------------------------------------------------------

def _join_frames(seed):
    rng = np.random.default_rng(seed)
    lk = rng.choice(40_000, 20_000, replace=False).astype(np.int64)
    rk = rng.choice(40_000, 15_000, replace=False).astype(np.int64)
    return (pd.DataFrame({"k": lk, "a": lk * 2}),
            pd.DataFrame({"k": rk, "b": rk * 3}))


def _join_check(ctx, lt, rt_, ldf, rdf, how):
    sql_how = {"inner": "JOIN", "left": "LEFT JOIN", "outer": "FULL JOIN"}[how]
    out = ctx.sql(f"SELECT l.a, r.b FROM {lt} l {sql_how} {rt_} r "
                  "ON l.k = r.k").compute()
    exp = ldf.merge(rdf, on="k", how=how)[["a", "b"]]
    norm = lambda f: f.astype("float64").fillna(-1).sort_values(  # noqa: E731
        ["a", "b"]).reset_index(drop=True)
    pd.testing.assert_frame_equal(norm(out), norm(exp))


def test_joins_without_and_with_match_marks(ctx):
    """INNER and LEFT never allocate the marks; FULL OUTER does, and after
    the inner join's tables went back to the pool its marks come from a
    recycled buffer that must be cleared."""
    ldf, rdf = _join_frames(31)
    ctx.create_table("mm_l", ldf)
    ctx.create_table("mm_r", rdf)
    _join_check(ctx, "mm_l", "mm_r", ldf, rdf, "inner")
    _join_check(ctx, "mm_l", "mm_r", ldf, rdf, "left")
    _join_check(ctx, "mm_l", "mm_r", ldf, rdf, "outer")
    _join_check(ctx, "mm_l", "mm_r", ldf, rdf, "inner")
    _join_check(ctx, "mm_l", "mm_r", ldf, rdf, "outer")


def test_hash_unmatched_on_an_inner_probed_table(ctx):
    """A table no mark_matched probe touched reports every build row; after
    a marking probe it reports the rows no probe key hit. A dirty buffer of
    the marks' size is put into the pool first."""
    runtime = ctx._get_runtime()
    rng = np.random.default_rng(4)
    nb = 3000
    bkeys = rng.permutation(10_000)[:nb].astype(np.int64)
    pkeys = rng.integers(0, 10_000, 5000).astype(np.int64)
    slots = 64
    while slots < 2 * nb:
        slots <<= 1
    bcol = runtime.upload_column(bkeys)
    pcol = runtime.upload_column(pkeys)
    dirty = runtime.upload_column(np.full(slots, -1, dtype=np.int32))
    del dirty  # back to the pool, every byte 0xFF
    table = runtime.hash_build(bcol, code_max=10_000)
    try:
        p, b, cnt = runtime.hash_probe(table, pcol, rt.JOIN_INNER)
        runtime.wrap_sel(p, cnt)
        runtime.wrap_sel(b, cnt)
        assert cnt == int(np.isin(pkeys, bkeys).sum())
        ptr, un = runtime.hash_unmatched(table)
        got, _ = runtime.wrap_sel(ptr, un).to_numpy()
        assert sorted(got.tolist()) == list(range(nb))
        p, b, cnt = runtime.hash_probe(table, pcol, rt.JOIN_INNER,
                                       mark_matched=True)
        runtime.wrap_sel(p, cnt)
        runtime.wrap_sel(b, cnt)
        ptr, un = runtime.hash_unmatched(table)
        got, _ = runtime.wrap_sel(ptr, un).to_numpy()
        exp = np.nonzero(~np.isin(bkeys, pkeys))[0]
        assert sorted(got.tolist()) == exp.tolist()
    finally:
        runtime.hash_table_free(table)
