"""GPU tests (-m gpu) of the radix sort chain: dsx_sort_word (stable LSD
radix over 64-bit order words, csrc/radix_sort.inc) directly and through
ORDER BY on float, skewed, wide and many-key collations.

The expectation is always pandas sort_values(kind="mergesort") applied key
by key from the last key to the first — the reference's own procedure
(physical/utils/sort.py:36-60). Comparison is exact on a row-id payload,
which proves stability. Every input is one where pandas alone is
deterministic (ties are broken by position, NaN/NULL go to na_position).
"""
import numpy as np
import pandas as pd
import pytest

from dask_sql_amd import runtime as rt

pytestmark = pytest.mark.gpu

DESC, NULLS_LAST, FLOAT = 2, 4, 8
MODES = [(False, False), (False, True), (True, False), (True, True)]


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    return Context()


@pytest.fixture
def prof(ctx):
    """Profiler switched on around a test; call it to read launch counts
    per kernel family since the last reset."""
    runtime = ctx._get_runtime()
    runtime.prof_enable(True)
    runtime.prof_reset()

    def read(reset=True):
        p = runtime.prof_get()
        if reset:
            runtime.prof_reset()
        return {k: v["launches"] for k, v in p.items()}

    yield read
    runtime.prof_enable(False)
    runtime.prof_reset()


def _bits(u):
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


_DMAX = np.finfo(np.float64).max
EDGE = np.array([
    0.0, -0.0, np.inf, -np.inf,
    _bits(0x7FF8000000000000), _bits(0xFFF8000000000000),
    _bits(0x7FF0000000000001), _bits(0xFFFFFFFFFFFFFFFF),
    5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308,
    _DMAX, -_DMAX, 1.0, -1.0], dtype=np.float64)
SEVEN = np.array([-1e300, -2.5, -1e-320, 0.0, 3.0, 7.25, 1e300])


def _edge_column(n, seed):
    """f64 key: heavy ties over 7 distinct doubles, the edge values dropped
    in at random rows (as many as fit), ~12 % NULLs."""
    rng = np.random.default_rng(seed)
    x = rng.choice(SEVEN, n)
    k = min(n, len(EDGE))
    x[rng.choice(n, k, replace=False)] = rng.permutation(EDGE)[:k]
    valid = (rng.random(n) > 0.12).astype(np.uint8)
    return x, valid


def _expected_perm(x, valid, desc, nulls_last, perm_in=None):
    p = np.arange(len(x)) if perm_in is None else np.asarray(perm_in)
    s = pd.Series(np.where(valid.astype(bool), x, np.nan)[p])
    order = s.sort_values(kind="mergesort", ascending=not desc,
                          na_position="last" if nulls_last else "first")
    return p[order.index.to_numpy()]


def _sort_word_f64(runtime, x, valid, desc, nulls_last, perm_in=None):
    col = runtime.upload_column(x, validity=valid)
    mode = FLOAT | (DESC if desc else 0) | (NULLS_LAST if nulls_last else 0)
    pin = None
    if perm_in is not None:
        pin = runtime.upload_column(np.asarray(perm_in, dtype=np.uint32),
                                    dtype=rt.I32)
    out = runtime.sort_word([col], [(0, 0, 0, True, mode)], len(x), pin)
    assert out is not None
    got, _ = out.to_numpy()
    return got.astype(np.int64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sort_word_f64_edges_and_ties(ctx, n):
    runtime = ctx._get_runtime()
    x, valid = _edge_column(n, seed=100 + n)
    for desc, nulls_last in MODES:
        got = _sort_word_f64(runtime, x, valid, desc, nulls_last)
        exp = _expected_perm(x, valid, desc, nulls_last)
        assert got.tolist() == exp.tolist(), (n, desc, nulls_last)


def test_sort_word_blocks_walk_several_tiles(ctx, monkeypatch):
    """3 blocks over 5000 rows: 1667 rows per block = 6 full tiles and a
    ragged 131-row tail each (the last block 1666)."""
    monkeypatch.setenv("DSX_RSORT_GRID", "3")
    runtime = ctx._get_runtime()
    x, valid = _edge_column(5000, seed=7)
    for desc, nulls_last in MODES:
        got = _sort_word_f64(runtime, x, valid, desc, nulls_last)
        exp = _expected_perm(x, valid, desc, nulls_last)
        assert got.tolist() == exp.tolist(), (desc, nulls_last)


@pytest.mark.parametrize("n", [257, 5000])
def test_sort_word_is_stable_relative_to_perm_in(ctx, monkeypatch, n):
    if n == 5000:
        monkeypatch.setenv("DSX_RSORT_GRID", "3")
    runtime = ctx._get_runtime()
    x, valid = _edge_column(n, seed=11 + n)
    perm_in = np.arange(n)[::-1].copy()
    for desc, nulls_last in MODES:
        got = _sort_word_f64(runtime, x, valid, desc, nulls_last, perm_in)
        exp = _expected_perm(x, valid, desc, nulls_last, perm_in)
        assert got.tolist() == exp.tolist(), (n, desc, nulls_last)
        # ties keep perm_in's (descending) order, not row order
        assert got.tolist() != _expected_perm(x, valid, desc,
                                              nulls_last).tolist()


def test_sort_word_f32_column(ctx):
    runtime = ctx._get_runtime()
    rng = np.random.default_rng(3)
    x = rng.choice(np.array([-1.5, -0.0, 0.0, 2.25, np.inf, np.nan],
                            dtype=np.float32), 777)
    col = runtime.upload_column(x)
    out = runtime.sort_word([col], [(0, 0, 0, False, FLOAT | DESC)], len(x))
    got, _ = out.to_numpy()
    exp = pd.Series(x).sort_values(kind="mergesort", ascending=False,
                                   na_position="first").index
    assert got.astype(np.int64).tolist() == exp.tolist()


def test_sort_word_rejects_what_it_cannot_code(ctx):
    runtime = ctx._get_runtime()
    icol = runtime.upload_column(np.arange(10, dtype=np.int64))
    fcol = runtime.upload_column(np.arange(10, dtype=np.float64))
    # key space above 2^62 (-4), float bit on an integer column, a float
    # key sharing a word, an integer spec on a float column (-3)
    big = (0, 0, 1 << 40, False, 0)
    assert runtime.sort_word([icol], [big, big], 10) is None
    assert runtime.sort_word([icol], [(0, 0, 10, False, FLOAT)], 10) is None
    assert runtime.sort_word([icol, fcol], [(0, 0, 10, False, 0),
                                            (1, 0, 0, False, FLOAT)],
                             10) is None
    assert runtime.sort_word([fcol], [(0, 0, 10, False, 0)], 10) is None
    # n == 0: an empty permutation
    e = runtime.upload_column(np.zeros(0, dtype=np.float64))
    out = runtime.sort_word([e], [(0, 0, 0, False, FLOAT)], 0)
    assert out is not None and out.len == 0


def test_constant_digits_are_skipped(ctx, prof):
    """Range 65536 → codes fill two bytes; the other six digits are constant
    across all rows and get no pass."""
    runtime = ctx._get_runtime()
    rng = np.random.default_rng(17)
    n = 4096
    k = rng.integers(0, 65536, n).astype(np.int64)
    k[0], k[1] = 0, 65535
    col = runtime.upload_column(k)
    prof()
    out = runtime.sort_word([col], [(0, 0, 65536, False, 0)], n)
    launches = prof()
    assert launches["k_rsort_codes"] == 1
    assert launches["k_rsort_hist"] == 2
    assert launches["k_rsort_scatter"] == 2
    got, _ = out.to_numpy()
    exp = pd.Series(k).sort_values(kind="mergesort").index
    assert got.astype(np.int64).tolist() == exp.tolist()


def _pandas_order(df, keys):
    """keys: [(column, ascending, nulls_first)] in ORDER BY order."""
    exp = df
    for col, asc, nulls_first in reversed(keys):
        exp = exp.sort_values(col, ascending=asc, kind="mergesort",
                              na_position="first" if nulls_first else "last")
    return exp.reset_index(drop=True)


@pytest.fixture(scope="module")
def df700p():
    # reference tests/integration/fixtures.py:50-57 plus a row-id payload
    np.random.seed(42)
    return pd.DataFrame(
        {"a": [1.0] * 100 + [2.0] * 200 + [3.0] * 400,
         "b": 10 * np.random.rand(700),
         "p": np.arange(700, dtype=np.int64)})


REFERENCE_FLOAT_CASES = [
    ("SELECT * FROM df700p ORDER BY b DESC, a DESC",
     [("b", False, True), ("a", False, True)]),
    ("SELECT * FROM df700p ORDER BY a DESC, b",
     [("a", False, True), ("b", True, False)]),
    ("SELECT * FROM df700p ORDER BY b, a",
     [("b", True, False), ("a", True, False)]),
]


@pytest.mark.parametrize("sql,keys", REFERENCE_FLOAT_CASES)
def test_reference_float_order_by_runs_on_device(ctx, prof, monkeypatch,
                                                 df700p, sql, keys):
    """The float ORDER BY statements of the reference's sort suite
    (tests/integration/test_sort.py:16-65): exact, and on the device."""
    monkeypatch.setenv("DSX_SORT_MIN", "1")
    ctx.create_table("df700p", df700p)
    prof()
    got = ctx.sql(sql).compute().reset_index(drop=True)
    launches = prof()
    assert launches.get("k_rsort_scatter", 0) > 0, \
        "float ORDER BY did not run the device radix sort"
    exp = _pandas_order(df700p, keys)
    assert got["p"].astype(np.int64).tolist() == exp["p"].tolist()
    assert got["a"].tolist() == exp["a"].tolist()
    assert got["b"].tolist() == exp["b"].tolist()


@pytest.fixture(scope="module")
def mixed_frame():
    rng = np.random.default_rng(23)
    n = 20_000
    f = rng.choice(np.round(rng.standard_normal(40) * 100, 2), n)
    f[rng.random(n) < 0.05] = np.nan          # NaN = NULL for a float column
    f[rng.choice(n, 50, replace=False)] = -0.0
    f[rng.choice(n, 50, replace=False)] = 0.0
    s = rng.choice(np.array(["delta", "alpha", "echo", "bravo", "charlie"],
                            dtype=object), n)
    s[rng.random(n) < 0.03] = None
    k = pd.array(rng.integers(-3, 9, n), dtype="Int64")
    k[rng.random(n) < 0.04] = pd.NA
    g = rng.choice(np.array([-1.5, 0.25, 3.0, 1e10, -np.inf, np.nan],
                            dtype=np.float32), n)
    ints = {f"i{j}": rng.integers(0, 4 + j, n).astype(np.int64)
            for j in range(5)}
    return pd.DataFrame({"f": f, "s": s, "k": k, "g": g, **ints,
                         "p": np.arange(n, dtype=np.int64)})


def test_mixed_float_string_int_chain(ctx, prof, monkeypatch, mixed_frame):
    monkeypatch.setenv("DSX_SORT_MIN", "1")
    ctx.create_table("mixed", mixed_frame)
    prof()
    got = ctx.sql("SELECT f, s, k, g, p FROM mixed "
                  "ORDER BY f DESC NULLS LAST, s, k DESC, g").compute()
    launches = prof()
    # words, least significant first: [g] [s, k] [f]
    assert launches.get("k_rsort_codes", 0) == 3
    assert "k_sort_bucket" not in launches
    exp = _pandas_order(mixed_frame, [("f", False, False), ("s", True, False),
                                      ("k", False, True), ("g", True, False)])
    assert got["p"].astype(np.int64).tolist() == exp["p"].tolist()


def test_five_integer_keys(ctx, prof, monkeypatch, mixed_frame):
    monkeypatch.setenv("DSX_SORT_MIN", "1")
    ctx.create_table("mixed", mixed_frame)
    prof()
    got = ctx.sql("SELECT i0, i1, i2, i3, i4, p FROM mixed "
                  "ORDER BY i0, i1 DESC, i2, i3 DESC, i4").compute()
    launches = prof()
    assert launches.get("k_rsort_codes", 0) == 2   # 4 + 1 keys
    exp = _pandas_order(mixed_frame, [("i0", True, False),
                                      ("i1", False, True),
                                      ("i2", True, False),
                                      ("i3", False, True),
                                      ("i4", True, False)])
    assert got["p"].astype(np.int64).tolist() == exp["p"].tolist()


def test_skewed_key_stays_on_device(ctx, prof):
    """99 % of the rows share one key: the bucket path overloads a bucket
    (-6); the radix chain takes over instead of the host."""
    rng = np.random.default_rng(29)
    n = 100_000
    k = np.zeros(n, dtype=np.int64)
    hot = rng.choice(n, n // 100, replace=False)
    k[hot] = rng.integers(1, 10 ** 12, len(hot))
    k[hot[0]] = 10 ** 12
    df = pd.DataFrame({"k": k, "p": np.arange(n, dtype=np.int64)})
    ctx.create_table("skewed", df)
    prof()
    got = ctx.sql("SELECT k, p FROM skewed ORDER BY k").compute()
    launches = prof()
    assert launches.get("k_rsort_scatter", 0) > 0, \
        "skewed ORDER BY did not run the device radix sort"
    exp = _pandas_order(df, [("k", True, False)])
    assert got["p"].astype(np.int64).tolist() == exp["p"].tolist()


def test_wide_table_sorts_on_device(ctx, prof, monkeypatch):
    monkeypatch.setenv("DSX_SORT_MIN", "1")
    rng = np.random.default_rng(31)
    n = 3000
    df = pd.DataFrame({f"c{j}": rng.integers(0, 50, n).astype(np.int64)
                       for j in range(19)})
    df["p"] = np.arange(n, dtype=np.int64)   # 20 columns
    ctx.create_table("wide20", df)
    prof()
    got = ctx.sql("SELECT * FROM wide20 ORDER BY c17 DESC").compute()
    launches = prof()
    assert launches.get("k_rsort_scatter", 0) > 0, \
        "ORDER BY on a 20-column table did not run the device radix sort"
    exp = _pandas_order(df, [("c17", False, True)])
    assert list(got.columns) == list(df.columns)
    assert got["p"].astype(np.int64).tolist() == exp["p"].tolist()
    assert got["c3"].astype(np.int64).tolist() == exp["c3"].tolist()


def test_radix_chain_equals_bucket_path(ctx, prof, monkeypatch):
    rng = np.random.default_rng(37)
    n = 50_000
    k1 = pd.array(rng.integers(0, 3000, n), dtype="Int64")
    k1[rng.random(n) < 0.02] = pd.NA
    k2 = pd.array(rng.integers(-40, 40, n), dtype="Int64")
    k2[rng.random(n) < 0.02] = pd.NA
    df = pd.DataFrame({"k1": k1, "k2": k2,
                       "p": np.arange(n, dtype=np.int64)})
    monkeypatch.setenv("DSX_SORT_MIN", "1")
    ctx.create_table("twokeys", df)
    sql = "SELECT k1, k2, p FROM twokeys ORDER BY k1 DESC NULLS LAST, k2"
    prof()
    bucket = ctx.sql(sql).compute()
    launches = prof()
    assert launches.get("k_sort_bucket", 0) > 0
    assert "k_rsort_scatter" not in launches   # the default is unchanged
    monkeypatch.setenv("DSX_SORT_RADIX", "1")
    radix = ctx.sql(sql).compute()
    launches = prof()
    assert launches.get("k_rsort_scatter", 0) > 0
    assert "k_sort_bucket" not in launches
    exp = _pandas_order(df, [("k1", False, False), ("k2", True, False)])
    assert bucket["p"].astype(np.int64).tolist() == exp["p"].tolist()
    assert radix["p"].astype(np.int64).tolist() == exp["p"].tolist()


def test_disable_knob_restores_host_path(ctx, prof, monkeypatch, df700p):
    monkeypatch.setenv("DSX_SORT_MIN", "1")
    ctx.create_table("df700p", df700p)
    sql = REFERENCE_FLOAT_CASES[0][0]
    device = ctx.sql(sql).compute().reset_index(drop=True)
    monkeypatch.setenv("DSX_DISABLE_RADIXSORT", "1")
    prof()
    host = ctx.sql(sql).compute().reset_index(drop=True)
    launches = prof()
    assert not [k for k in launches if k.startswith("k_rsort_")]
    assert list(host.columns) == list(device.columns)
    for c in host.columns:
        assert host[c].tolist() == device[c].tolist()
