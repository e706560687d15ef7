"""GPU tests (-m gpu) of the word front half of the device window paths:
dsx_window_mark_word + dsx_window_seg_ids (csrc/window_words.inc) directly,
and window functions over float, NULLS FIRST, many-key, wide-range, skewed
and wide-table keys through SQL.

SQL results are compared bit for bit (values, NULL positions, dtype) with
the host path (DSX_DISABLE_DEVWINDOW=1) — the behaviour of every shape here
before the word front half existed. Values are integers and keys stay below
2^53, so nothing depends on summation order. Every device case also checks
in the kernel profile that the word front half and the expected window
kernel really ran."""
import numpy as np
import pandas as pd
import pytest

from dask_sql_amd import runtime as rt

pytestmark = pytest.mark.gpu

DESC, NULLS_LAST, FLOAT = 2, 4, 8
WORD_KERNELS = ("k_win_mark_word", "k_win_seg_ids", "k_rsort_scatter")


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    return Context()


# ---- ABI level ---------------------------------------------------------------
def _marks_ids(runtime, cols, specs, n, perm=None, marks=None):
    pcol = None
    if perm is not None:
        pcol = runtime.upload_column(np.asarray(perm, dtype=np.uint32),
                                     dtype=rt.I32)
    m = runtime.window_mark_word(cols, specs, n, pcol, marks)
    assert m is not None
    ids, nseg = runtime.window_seg_ids(m, n)
    got_m, _ = m.to_numpy()
    got_i, _ = ids.to_numpy()
    return m, got_m.astype(bool), got_i.astype(np.int64), nseg


def _expect(codes):
    """numpy statement of the contract over codes already in sorted order"""
    c = np.asarray(codes)
    marks = np.r_[True, c[1:] != c[:-1]] if len(c) else np.zeros(0, bool)
    return marks, np.cumsum(marks) - 1


def _int_word(runtime, k):
    k = np.asarray(k, dtype=np.int64)
    mn, mx = int(k.min()), int(k.max())
    return [runtime.upload_column(k)], [(0, mn, mx - mn + 1, False,
                                         NULLS_LAST)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_marks_and_ids_small_sizes(ctx, n):
    runtime = ctx._get_runtime()
    rng = np.random.default_rng(n)
    cases = {
        "all equal": np.full(n, 7, dtype=np.int64),
        "all distinct": np.arange(n, dtype=np.int64) * 3 - 5,
        "runs": np.sort(rng.integers(0, max(2, n // 3), n)).astype(np.int64),
    }
    for name, k in cases.items():
        cols, specs = _int_word(runtime, k)
        _, m, ids, nseg = _marks_ids(runtime, cols, specs, n)
        em, ei = _expect(k)
        assert m.tolist() == em.tolist(), (n, name)
        assert ids.tolist() == ei.tolist(), (n, name)
        assert nseg == int(em.sum()), (n, name)
    assert _expect(cases["all equal"])[0].sum() == 1
    assert _expect(cases["all distinct"])[0].sum() == n


def test_boundaries_on_the_halo_lanes(ctx):
    """Runs that start exactly at sorted positions 64, 128, 256 and 512 —
    the first lanes of a wave, whose left neighbour no shuffle delivers —
    and, as the counter-case, runs that end one row later so that the halo
    lanes must NOT mark."""
    runtime = ctx._get_runtime()
    n = 700
    for shift in (0, 1):
        heads = np.array([0, 64, 128, 256, 512]) + np.array([0] + [shift] * 4)
        k = np.zeros(n, dtype=np.int64)
        for j, h in enumerate(heads):
            k[h:] = j * 11
        cols, specs = _int_word(runtime, k)
        _, m, ids, nseg = _marks_ids(runtime, cols, specs, n)
        assert np.flatnonzero(m).tolist() == heads.tolist(), shift
        assert ids.tolist() == _expect(k)[1].tolist(), shift
        assert nseg == 5


def test_non_identity_perm(ctx):
    runtime = ctx._get_runtime()
    rng = np.random.default_rng(3)
    n = 1000
    k = rng.integers(-20, 20, n).astype(np.int64)
    perm = np.argsort(k, kind="stable")
    cols, specs = _int_word(runtime, k)
    _, m, ids, nseg = _marks_ids(runtime, cols, specs, n, perm)
    em, ei = _expect(k[perm])
    assert m.tolist() == em.tolist()
    assert ids.tolist() == ei.tolist()
    assert nseg == len(np.unique(k))
    # an unsorted sequence is marked wherever neighbours differ, too
    perm = rng.permutation(n)
    _, m, ids, _ = _marks_ids(runtime, cols, specs, n, perm)
    em, ei = _expect(k[perm])
    assert m.tolist() == em.tolist() and ids.tolist() == ei.tolist()


def test_or_accumulation_over_two_words(ctx):
    runtime = ctx._get_runtime()
    rng = np.random.default_rng(5)
    n = 1500
    a = rng.integers(0, 6, n).astype(np.int64)
    b = rng.integers(0, 9, n).astype(np.int64)
    perm = np.lexsort((b, a))
    ca, sa = _int_word(runtime, a)
    cb, sb = _int_word(runtime, b)
    marks, m_a, ids_a, _ = _marks_ids(runtime, ca, sa, n, perm)
    assert m_a.tolist() == _expect(a[perm])[0].tolist()
    again, m_ab, ids_ab, nseg = _marks_ids(runtime, cb, sb, n, perm, marks)
    assert again is marks
    em = _expect(a[perm])[0] | _expect(b[perm])[0]
    assert m_ab.tolist() == em.tolist()
    assert ids_ab.tolist() == (np.cumsum(em) - 1).tolist()
    assert nseg == len(set(zip(a.tolist(), b.tolist())))
    # the partition ids taken before the second word are untouched
    assert ids_a.tolist() == _expect(a[perm])[1].tolist()


def test_float_word_nan_null_zero_inf(ctx):
    runtime = ctx._get_runtime()
    vals = np.array([-np.inf, -2.5, -0.0, 0.0, 0.0, -0.0, 1.0, 1.0, np.inf,
                     np.inf, np.nan, 5.0, np.nan, 5.0], dtype=np.float64)
    valid = np.ones(len(vals), dtype=np.uint8)
    valid[[11, 13]] = 0            # NULLs whose payload is a real value
    n = len(vals)
    col = runtime.upload_column(vals, validity=valid)
    _, m, ids, nseg = _marks_ids(runtime, [col],
                                 [(0, 0, 0, True, FLOAT | NULLS_LAST)], n)
    #        -inf -2.5 -0  0  0  -0  1  1  inf inf nan NULL nan NULL
    exp = [1, 1, 1, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0]
    assert m.astype(int).tolist() == exp
    assert ids.tolist() == (np.cumsum(exp) - 1).tolist()
    assert nseg == 6
    # a float32 column, DESC NULLS FIRST: same equalities
    col32 = runtime.upload_column(vals.astype(np.float32), validity=valid)
    _, m, _, _ = _marks_ids(runtime, [col32], [(0, 0, 0, True, FLOAT | DESC)],
                            n)
    assert m.astype(int).tolist() == exp


def test_blocks_walk_several_tiles(ctx, monkeypatch):
    """3 blocks over 5000 rows: the mark kernel strides each block over 7
    tiles, the id scan gives each block 1667 rows = 6 tiles and a tail."""
    monkeypatch.setenv("DSX_RSORT_GRID", "3")
    runtime = ctx._get_runtime()
    rng = np.random.default_rng(9)
    n = 5000
    k = np.sort(rng.integers(0, 900, n)).astype(np.int64)
    cols, specs = _int_word(runtime, k)
    _, m, ids, nseg = _marks_ids(runtime, cols, specs, n)
    em, ei = _expect(k)
    assert m.tolist() == em.tolist()
    assert ids.tolist() == ei.tolist()
    assert nseg == len(np.unique(k))
    f = np.sort(rng.choice(np.array([-1.5, 0.0, 2.0, 1e300]), n))
    col = runtime.upload_column(f)
    _, m, ids, _ = _marks_ids(runtime, [col],
                              [(0, 0, 0, False, FLOAT | NULLS_LAST)], n)
    assert ids.tolist() == _expect(f)[1].tolist()


def test_refusals_and_empty_input(ctx):
    runtime = ctx._get_runtime()
    icol = runtime.upload_column(np.arange(10, dtype=np.int64))
    fcol = runtime.upload_column(np.arange(10, dtype=np.float64))
    big = (0, 0, 1 << 40, False, 0)
    # the answers of sort_word: key space above 2^62 (-4), malformed (-3)
    assert runtime.window_mark_word([icol], [big, big], 10, None) is None
    assert runtime.window_mark_word([icol], [(0, 0, 10, False, FLOAT)], 10,
                                    None) is None
    assert runtime.window_mark_word([fcol], [(0, 0, 10, False, 0)], 10,
                                    None) is None
    e = runtime.upload_column(np.zeros(0, dtype=np.float64))
    m = runtime.window_mark_word([e], [(0, 0, 0, False, FLOAT)], 0, None)
    assert m is not None and m.len == 0
    ids, nseg = runtime.window_seg_ids(m, 0)
    assert ids.len == 0 and nseg == 0


# ---- SQL level ---------------------------------------------------------------
def _run(ctx, sql):
    r = ctx._get_runtime()
    r.prof_enable(True)
    r.prof_reset()
    try:
        out = ctx.sql(sql).compute()
        prof = r.prof_get()
    finally:
        r.prof_enable(False)
    launches = {k: v["launches"] for k, v in prof.items()}
    return out.sort_values("rid").reset_index(drop=True), launches


def _host(ctx, monkeypatch, sql):
    monkeypatch.setenv("DSX_DISABLE_DEVWINDOW", "1")
    try:
        out, launches = _run(ctx, sql)
    finally:
        monkeypatch.delenv("DSX_DISABLE_DEVWINDOW")
    assert not [k for k in launches if k.startswith("k_win_")], launches
    return out


def _assert_identical(got, want, what):
    assert list(got.columns) == list(want.columns), what
    assert len(got) == len(want), what
    for c in want.columns:
        assert got[c].dtype == want[c].dtype, \
            f"{what}: {c} is {got[c].dtype}, host gives {want[c].dtype}"
        g = got[c].to_numpy(dtype=np.float64, na_value=np.nan)
        w = want[c].to_numpy(dtype=np.float64, na_value=np.nan)
        bad = np.flatnonzero(np.isnan(g) != np.isnan(w))
        assert bad.size == 0, f"{what}: {c} NULLs differ at rid {bad[:8]}"
        ok = ~np.isnan(w)
        bad = np.flatnonzero(ok)[g[ok] != w[ok]]
        assert bad.size == 0, (f"{what}: {c} differs at rid {bad[:8]}: "
                               f"{g[bad[:8]]} vs host {w[bad[:8]]}")


# ranking, shifts and running aggregates over the default frame, one tile
# frame and one prefix frame
ORDERED = {
    "rn": "ROW_NUMBER() OVER ({w})",
    "rk": "RANK() OVER ({w})",
    "dr": "DENSE_RANK() OVER ({w})",
    "lag1": "LAG(v) OVER ({w})",
    "lag2d": "LAG(v, 2, 77) OVER ({w})",
    "lead1": "LEAD(v) OVER ({w})",
    "lead3d": "LEAD(v, 3, 99) OVER ({w})",
    # over the non-NULL rid, which also names the row that came first: on a
    # NULL first row the kernel returns NULL (the reference's x.iloc[0])
    # while the host path's transform("first") skips to the first non-NULL
    # value, for integer keys as well — a difference older than this path
    "fv": "FIRST_VALUE(rid) OVER ({w})",
    "rsum": "SUM(v) OVER ({w})",
    "rcnt": "COUNT(v) OVER ({w})",
    "rmin": "MIN(v) OVER ({w})",
    "rmax": "MAX(v) OVER ({w})",
    "ravg": "AVG(v) OVER ({w})",
    "tile": "SUM(v) OVER ({w} ROWS BETWEEN 2 PRECEDING AND 1 FOLLOWING)",
    "prefix": "MAX(v) OVER ({w} ROWS BETWEEN UNBOUNDED PRECEDING AND "
              "1 FOLLOWING)",
}
ORDERED_KERNELS = ("k_win_pos", "k_win_scan", "k_win_peer",
                   "k_win_rows_tile", "k_win_rows_prefix")
# no ORDER BY: the default frame is the whole partition
UNORDERED = {
    "rn": "ROW_NUMBER() OVER ({w})",
    "psum": "SUM(v) OVER ({w})",
    "pcnt": "COUNT(v) OVER ({w})",
    "pcntstar": "COUNT(*) OVER ({w})",
    "pmin": "MIN(v) OVER ({w})",
    "pmax": "MAX(v) OVER ({w})",
    "pavg": "AVG(v) OVER ({w})",
}
UNORDERED_KERNELS = ("k_win_pos", "k_win_scan", "k_win_peer")


def _sql(table, window, exprs=ORDERED):
    cols = ", ".join(e.format(w=window) + f" AS {name}"
                     for name, e in exprs.items())
    return f"SELECT rid, {cols} FROM {table}"


def _check(ctx, monkeypatch, table, window, exprs=ORDERED,
           kernels=ORDERED_KERNELS):
    sql = _sql(table, window, exprs)
    got, launches = _run(ctx, sql)
    for k in WORD_KERNELS + tuple(kernels):
        assert launches.get(k, 0) > 0, (k, window, launches)
    _assert_identical(got, _host(ctx, monkeypatch, sql), window)
    return got, launches


def _int_v(rng, n, null_frac=0.15):
    v = pd.array(rng.integers(-1000, 1000, n), dtype="Int64")
    v[rng.random(n) < null_frac] = pd.NA
    return v


@pytest.fixture(scope="module")
def float_table(ctx):
    """f: 12 distinct doubles with heavy ties, NaN/NULL, -0.0 and +0.0, ±inf;
    g: a float partition key of the same kind; p: a small integer key."""
    rng = np.random.default_rng(41)
    n = 6001
    pool = np.array([-1e300, -7.5, -1.0, 0.0, 0.5, 1.0, 2.25, 3.0, 1e10,
                     1e300, np.inf, -np.inf])
    f = rng.choice(pool, n)
    f[rng.random(n) < 0.06] = np.nan
    f[rng.choice(n, 40, replace=False)] = -0.0
    g = rng.choice(np.array([-2.5, 0.0, 1.5, 1e200, np.inf]), n)
    g[rng.random(n) < 0.05] = np.nan
    g[rng.choice(n, 30, replace=False)] = -0.0
    df = pd.DataFrame({"f": f, "g": g,
                       "p": rng.integers(0, 7, n).astype(np.int64),
                       "v": _int_v(rng, n),
                       "rid": np.arange(n, dtype=np.int64)})
    ctx.create_table("ww_float", df)
    return df


@pytest.mark.parametrize("window", [
    "PARTITION BY p ORDER BY f",
    "PARTITION BY p ORDER BY f DESC",
    "ORDER BY f",
])
def test_float_order_key(ctx, monkeypatch, float_table, window):
    _check(ctx, monkeypatch, "ww_float", window)


@pytest.mark.parametrize("window", [
    "PARTITION BY g ORDER BY p",
    "PARTITION BY g ORDER BY f DESC",
])
def test_float_partition_key_ordered(ctx, monkeypatch, float_table, window):
    _check(ctx, monkeypatch, "ww_float", window)


def test_float_partition_key_whole_partition(ctx, monkeypatch, float_table):
    got, _ = _check(ctx, monkeypatch, "ww_float", "PARTITION BY g",
                    UNORDERED, UNORDERED_KERNELS)
    # and directly: NaN/NULL form one partition, -0.0 joins +0.0
    df = float_table
    key = df["g"].where(df["g"] != 0.0, 0.0)
    exp = df["v"].astype("float64").groupby(key, dropna=False) \
        .transform("sum")
    assert got["psum"].to_numpy(dtype=np.float64, na_value=np.nan) \
        .tolist() == exp.tolist()


@pytest.fixture(scope="module")
def int_table(ctx):
    rng = np.random.default_rng(43)
    n = 8000

    def nullable(lo, hi, frac):
        a = pd.array(rng.integers(lo, hi, n), dtype="Int64")
        a[rng.random(n) < frac] = pd.NA
        return a

    cols = {"a": nullable(-4, 5, 0.1), "b": nullable(0, 6, 0.1),
            "p1": rng.integers(0, 4, n).astype(np.int64),
            "p2": nullable(0, 3, 0.05)}
    for j in range(4):
        cols[f"o{j}"] = rng.integers(0, 3 + j, n).astype(np.int64)
    # two keys of range ~2^40 each, few distinct values so partitions have
    # many rows
    big = np.array([0, 1, (1 << 40) - 1, 1 << 39], dtype=np.int64)
    cols["w1"] = rng.choice(big, n)
    cols["w2"] = rng.choice(-big, n)
    cols["v"] = _int_v(rng, n)
    cols["rid"] = np.arange(n, dtype=np.int64)
    df = pd.DataFrame(cols)
    ctx.create_table("ww_int", df)
    return df


@pytest.mark.parametrize("window", [
    "ORDER BY a NULLS FIRST, b DESC NULLS LAST",
    "PARTITION BY p1 ORDER BY a NULLS FIRST, b DESC NULLS LAST",
    "PARTITION BY p1, p2 ORDER BY o0, o1 DESC, o2, o3 DESC",
    "PARTITION BY w1, w2 ORDER BY o3",
])
def test_integer_keys_the_bucket_sort_declines(ctx, monkeypatch, int_table,
                                               window):
    _check(ctx, monkeypatch, "ww_int", window)


def test_skewed_partition_key(ctx, monkeypatch):
    """99 % of the rows share one partition key (the ORDER BY table of
    test_gpu_sort_radix.test_skewed_key_stays_on_device): sort_perm answers
    -6 at this size, the word chain takes the window instead of the host."""
    rng = np.random.default_rng(29)
    n = 100_000
    k = np.zeros(n, dtype=np.int64)
    hot = rng.choice(n, n // 100, replace=False)
    k[hot] = rng.integers(1, 10 ** 12, len(hot))
    k[hot[0]] = 10 ** 12
    df = pd.DataFrame({"k": k, "o": rng.integers(0, 50, n).astype(np.int64),
                       "v": _int_v(rng, n),
                       "rid": np.arange(n, dtype=np.int64)})
    ctx.create_table("ww_skew", df)
    _check(ctx, monkeypatch, "ww_skew", "PARTITION BY k ORDER BY o")


def test_twenty_column_table(ctx, monkeypatch):
    rng = np.random.default_rng(31)
    n = 3000
    df = pd.DataFrame({f"c{j}": rng.integers(0, 9, n).astype(np.int64)
                       for j in range(18)})
    df["v"] = _int_v(rng, n)
    df["rid"] = np.arange(n, dtype=np.int64)   # 20 columns
    ctx.create_table("ww_wide", df)
    _check(ctx, monkeypatch, "ww_wide", "PARTITION BY c16 ORDER BY c3 DESC")


def test_front_halves_agree(ctx, monkeypatch, int_table):
    """An all-integer two-key window: the default stays on the bucket front
    half (no new kernel), DSX_WIN_WORDS=1 moves it to the word front half,
    and both give the same bits."""
    sql = _sql("ww_int", "PARTITION BY p1 ORDER BY b DESC")
    default, launches = _run(ctx, sql)
    assert launches.get("k_win_mark_word", 0) == 0, launches
    assert launches.get("k_win_seg_ids", 0) == 0, launches
    assert launches.get("k_rsort_scatter", 0) == 0, launches
    monkeypatch.setenv("DSX_WIN_WORDS", "1")
    words, launches = _run(ctx, sql)
    monkeypatch.delenv("DSX_WIN_WORDS")
    for k in WORD_KERNELS + ORDERED_KERNELS:
        assert launches.get(k, 0) > 0, (k, launches)
    assert launches.get("k_sort_bucket", 0) == 0, launches
    _assert_identical(words, default, "word vs bucket front half")
    _assert_identical(words, _host(ctx, monkeypatch, sql), "word vs host")


def test_disable_knob_restores_host_routing(ctx, monkeypatch, float_table,
                                            int_table):
    sql = _sql("ww_float", "PARTITION BY p ORDER BY f")
    monkeypatch.setenv("DSX_DISABLE_WINWORDS", "1")
    got, launches = _run(ctx, sql)
    monkeypatch.delenv("DSX_DISABLE_WINWORDS")
    for k in WORD_KERNELS + ORDERED_KERNELS:
        assert launches.get(k, 0) == 0, (k, launches)
    _assert_identical(got, _host(ctx, monkeypatch, sql), "knob vs host")
    # NULLS FIRST goes back to the host as well
    sql = _sql("ww_int", "ORDER BY a NULLS FIRST, b DESC NULLS LAST")
    monkeypatch.setenv("DSX_DISABLE_WINWORDS", "1")
    got, launches = _run(ctx, sql)
    monkeypatch.delenv("DSX_DISABLE_WINWORDS")
    assert not [k for k in launches if k.startswith("k_win_")], launches
    _assert_identical(got, _host(ctx, monkeypatch, sql), "NF knob vs host")


def test_row_number_against_pandas(ctx, float_table):
    """Independent of the host path: ROW_NUMBER over a NaN/NULL-bearing
    float key, restated with a stable pandas sort and cumcount."""
    got, launches = _run(ctx, "SELECT rid, ROW_NUMBER() OVER (PARTITION BY p "
                              "ORDER BY f) AS rn FROM ww_float")
    assert launches.get("k_rsort_scatter", 0) > 0, launches
    assert launches.get("k_win_mark_word", 0) > 0, launches
    assert launches.get("k_win_pos", 0) > 0, launches
    df = float_table
    s = df.sort_values("f", kind="mergesort", na_position="last")
    s = s.sort_values("p", kind="mergesort")
    rn = s.groupby("p", sort=False).cumcount() + 1
    exp = np.empty(len(df), dtype=np.int64)
    exp[s["rid"].to_numpy()] = rn.to_numpy()
    assert got["rn"].dtype == np.int64
    assert got["rn"].tolist() == exp.tolist()


# ---- string ORDER BY key on the word route ---------------------------------
RANKING = {"rn": "ROW_NUMBER() OVER ({w})", "rk": "RANK() OVER ({w})",
           "dr": "DENSE_RANK() OVER ({w})"}


@pytest.fixture(scope="module")
def string_table(ctx):
    """200 rows (more than one wave). s: six strings whose order of first
    appearance (the dictionary's) is not alphabetical, some NULL; f: five
    doubles with ties, some NaN; p: a small integer key."""
    rng = np.random.default_rng(47)
    n = 200
    names = np.array(["pear", "apple", "quince", "fig", "banana", "cherry"],
                     dtype=object)
    s = names[rng.integers(0, 6, n)]
    s[:6] = names                      # first appearance: this very order
    s[rng.choice(np.arange(6, n), 15, replace=False)] = None
    f = rng.choice(np.array([-3.5, -1.0, 0.25, 2.0, 1e9]), n)
    f[rng.choice(n, 9, replace=False)] = np.nan
    df = pd.DataFrame({"s": s, "f": f,
                       "p": rng.integers(0, 4, n).astype(np.int64),
                       "rid": np.arange(n, dtype=np.int64)})
    ctx.create_table("ww_str", df)
    return df


def _ranking_expected(part, order):
    """RANK, DENSE_RANK and the size of every row's peer class, by counting:
    part / order hold one hashable partition key and one comparable order
    key per row."""
    n = len(part)
    rk, dr, peers = [], [], []
    for i in range(n):
        mine = [order[j] for j in range(n) if part[j] == part[i]]
        rk.append(1 + sum(o < order[i] for o in mine))
        dr.append(1 + len({o for o in mine if o < order[i]}))
        peers.append(sum(o == order[i] for o in mine))
    return np.array(rk), np.array(dr), np.array(peers)


def _check_ranking(got, part, order, what):
    rk, dr, peers = _ranking_expected(part, order)
    for c in RANKING:
        assert got[c].dtype == np.int64, (what, c)
    assert got["rk"].tolist() == rk.tolist(), what
    assert got["dr"].tolist() == dr.tolist(), what
    # ROW_NUMBER numbers the rows of a peer class rk .. rk+peers-1, in an
    # order of its own choosing
    rn = got["rn"].to_numpy()
    assert ((rn >= rk) & (rn < rk + peers)).all(), what
    assert len(set(zip(part, rn.tolist()))) == len(rn), what


def _s_key(s):
    return (s is None, s or "")       # alphabetical, NULL last


def _f_key(f, desc=False):
    nan = bool(np.isnan(f))           # NaN last in both directions
    return (nan, 0.0 if nan else (-f if desc else f))


def _assert_word_route(launches):
    assert launches.get("k_rsort_scatter", 0) \
        + launches.get("k_rsort_codes", 0) > 0, launches
    assert launches.get("k_win_mark_word", 0) > 0, launches


def test_string_order_key_on_the_word_route(ctx, string_table):
    """The float key sends the window to the word front half, where the
    string key sorts by its alphabetic rank — compared with the ranks
    counted in Python, not with the host path (which reads a dictionary
    order key's raw codes, in first-appearance order)."""
    df = string_table
    s, f, p = df["s"].tolist(), df["f"].tolist(), df["p"].tolist()
    got, launches = _run(ctx, _sql("ww_str", "PARTITION BY p ORDER BY s, "
                                             "f DESC", RANKING))
    _assert_word_route(launches)
    _check_ranking(got, p, [_s_key(a) + _f_key(b, desc=True)
                            for a, b in zip(s, f)], "ORDER BY s, f DESC")
    # a string PARTITION BY key goes by raw code, NULL a partition of its own
    got, launches = _run(ctx, _sql("ww_str", "PARTITION BY s ORDER BY f",
                                   RANKING))
    _assert_word_route(launches)
    _check_ranking(got, s, [_f_key(b) for b in f], "PARTITION BY s")


def test_string_order_key_front_halves_agree(ctx, monkeypatch, string_table):
    """ORDER BY s alone is all-integer: the bucket front half takes it by
    default, DSX_WIN_WORDS=1 moves it to the word front half; same bits."""
    df = string_table
    sql = _sql("ww_str", "PARTITION BY p ORDER BY s", RANKING)
    bucket, launches = _run(ctx, sql)
    assert launches.get("k_win_mark_word", 0) == 0, launches
    monkeypatch.setenv("DSX_WIN_WORDS", "1")
    words, launches = _run(ctx, sql)
    monkeypatch.delenv("DSX_WIN_WORDS")
    _assert_word_route(launches)
    _assert_identical(words, bucket, "word vs bucket front half")
    _check_ranking(words, df["p"].tolist(),
                   [_s_key(a) for a in df["s"].tolist()], "ORDER BY s")
