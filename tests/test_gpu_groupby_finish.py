"""Group-by output columns written by the group-by call itself
(dsx_hash_groupby_cols, -m gpu).

Every case runs through Context.sql(...).compute() three ways: default (one
finish launch writes every key and aggregate column), DSX_DISABLE_GBFINISH=1
(the per-column dsx_eval programs) and pandas on the same frame. After sorting
by the keys the two device frames must be equal, dtypes included; float inputs
are integer-valued doubles below 2^53, so sums are exact in any order and AVG
is bit-equal. The profiler's kernel families show which code ran: no k_eval
and exactly one finish launch by default, k_eval under the knob, and the
group-by family that names the case's path in both."""
import numpy as np
import pandas as pd
import pytest

from tests.conftest import assert_frame_close

pytestmark = pytest.mark.gpu

KNOB = "DSX_DISABLE_GBFINISH"
FINISH = ("k_gbpart_finalize", "k_groupby_finish")
DIRECT, PART, GLOBAL = ("k_groupby_direct", "k_gbpart_aggregate",
                        "k_groupby_global")


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    return Context()


def _run(ctx, monkeypatch, sql, knob):
    r = ctx._get_runtime()
    if knob:
        monkeypatch.setenv(KNOB, "1")
    else:
        monkeypatch.delenv(KNOB, raising=False)
    r.prof_reset()
    r.prof_enable(True)
    try:
        out = ctx.sql(sql).compute()
        prof = r.prof_get()
    finally:
        r.prof_enable(False)
        r.prof_reset()
        monkeypatch.delenv(KNOB, raising=False)
    return out, prof


def _launches(prof, names):
    return sum(prof.get(f, {}).get("launches", 0) for f in names)


def _check(ctx, monkeypatch, name, df, sql, keys, exp, family,
           declined=False, **create_kw):
    ctx.create_table(name, df, **create_kw)
    new, pn = _run(ctx, monkeypatch, sql, knob=False)
    old, po = _run(ctx, monkeypatch, sql, knob=True)
    a = new.sort_values(keys, kind="mergesort").reset_index(drop=True)
    b = old.sort_values(keys, kind="mergesort").reset_index(drop=True)
    pd.testing.assert_frame_equal(a, b, check_dtype=True, check_exact=True)
    assert_frame_close(new, exp.reset_index(drop=True)[list(new.columns)],
                       sort_by=keys)
    if declined:
        assert "k_eval" in pn, sorted(pn)      # the new path declined
    else:
        assert "k_eval" not in pn, sorted(pn)
        assert _launches(pn, FINISH) == (1 if len(exp) else 0), pn
    if len(exp):
        assert "k_eval" in po, sorted(po)
    if family is not None:
        assert family in pn and family in po, (sorted(pn), sorted(po))
    return new


def _ints_as_f64(rng, n, lo=-1000, hi=1000):
    return rng.integers(lo, hi, n).astype(np.float64)


def _sum_count(df, keys):
    g = df.groupby(keys, dropna=False, sort=False)
    return pd.DataFrame({"s": g["v"].sum(), "c": g.size()}).reset_index()


SQL_SC = "SELECT k, SUM(v) AS s, COUNT(*) AS c FROM {t} GROUP BY k"


def test_no_group_passes_the_filter(ctx, monkeypatch):
    rng = np.random.default_rng(0)
    df = pd.DataFrame({"k": rng.integers(0, 9, 2000).astype(np.int64),
                       "v": _ints_as_f64(rng, 2000)})
    exp = _sum_count(df[df["v"] < -1e9], ["k"])
    out = _check(ctx, monkeypatch, "gbf_g0", df,
                 "SELECT k, SUM(v) AS s, COUNT(*) AS c FROM gbf_g0 "
                 "WHERE v < -1000000000 GROUP BY k", ["k"], exp, None)
    assert len(out) == 0


@pytest.mark.parametrize("G", [1, 255, 256, 257])
def test_group_counts_direct(ctx, monkeypatch, G):
    n = 3000
    rng = np.random.default_rng(G)
    df = pd.DataFrame({"k": (np.arange(n) % G).astype(np.int64),
                       "v": _ints_as_f64(rng, n)})
    _check(ctx, monkeypatch, f"gbf_d{G}", df, SQL_SC.format(t=f"gbf_d{G}"),
           ["k"], _sum_count(df, ["k"]), DIRECT)


@pytest.mark.parametrize("G", [2, 255, 256, 257])
def test_group_counts_partition(ctx, monkeypatch, G):
    """A key space too large for LDS and never-NULL inputs: the partition
    path, range-bucketed at G = 2 (space 100 001) and hashed above 4 M."""
    n = 3000
    rng = np.random.default_rng(1000 + G)
    df = pd.DataFrame({"k": ((np.arange(n) % G) * 100_000).astype(np.int64),
                       "v": _ints_as_f64(rng, n)})
    _check(ctx, monkeypatch, f"gbf_p{G}", df, SQL_SC.format(t=f"gbf_p{G}"),
           ["k"], _sum_count(df, ["k"]), PART)


def test_more_groups_than_one_grid_sweep(ctx, monkeypatch):
    """G = 2048 x 256 + 1: the finish kernel's grid-stride loop takes a
    second trip."""
    G, n = 2048 * 256 + 1, 600_000
    rng = np.random.default_rng(5)
    k = np.concatenate([np.arange(G), rng.integers(0, G, n - G)])
    df = pd.DataFrame({"k": rng.permutation(k).astype(np.int64),
                       "v": _ints_as_f64(rng, n)})
    exp = _sum_count(df, ["k"])
    assert len(exp) == G
    _check(ctx, monkeypatch, "gbf_big", df, SQL_SC.format(t="gbf_big"),
           ["k"], exp, PART)


@pytest.mark.parametrize("spread,family", [(50, DIRECT), (5000, PART)],
                         ids=["direct", "partition"])
def test_three_keys_negative_min_date_and_range_one(ctx, monkeypatch, spread,
                                                    family):
    n = 4000
    rng = np.random.default_rng(spread)
    df = pd.DataFrame({
        "a": rng.integers(-spread, spread, n).astype(np.int64),
        "d": rng.integers(9000, 9031, n).astype(np.int32),
        "p": np.full(n, 7, dtype=np.int64),
        "v": _ints_as_f64(rng, n)})
    df.loc[0, "a"], df.loc[1, "a"] = -spread, spread - 1
    g = df.groupby(["a", "d", "p"], sort=False)
    exp = pd.DataFrame({"s": g["v"].sum()}).reset_index()
    exp["d"] = pd.to_datetime(exp["d"].astype("int64"), unit="D")
    t = f"gbf_k3_{spread}"
    out = _check(ctx, monkeypatch, t, df,
                 f"SELECT a, d, p, SUM(v) AS s FROM {t} GROUP BY a, d, p",
                 ["a", "d", "p"], exp, family, date_columns=["d"])
    assert str(out["d"].dtype).startswith("datetime64")
    assert (out["p"] == 7).all() and out["a"].min() == -spread


def test_dictionary_string_key(ctx, monkeypatch):
    n = 3000
    rng = np.random.default_rng(6)
    df = pd.DataFrame({"s": rng.choice(["x", "yy", "zzz", "w w"], n),
                       "w": rng.integers(-9, 9, n).astype(np.int64)})
    g = df.groupby("s", sort=False)
    exp = pd.DataFrame({"c": g.size(), "sw": g["w"].sum()}).reset_index()
    out = _check(ctx, monkeypatch, "gbf_str", df,
                 "SELECT s, COUNT(*) AS c, SUM(w) AS sw FROM gbf_str "
                 "GROUP BY s", ["s"], exp, DIRECT)
    assert sorted(out["s"]) == ["w w", "x", "yy", "zzz"]


@pytest.mark.parametrize("nkeys", [1, 2])
def test_nullable_keys_with_rows_in_the_null_group(ctx, monkeypatch, nkeys):
    n = 3000
    rng = np.random.default_rng(70 + nkeys)
    cols = {}
    for name, lo, hi in [("k", -3, 4), ("j", 10, 13)][:nkeys]:
        a = pd.array(rng.integers(lo, hi, n), dtype="Int64")
        a[rng.random(n) < 0.2] = pd.NA
        cols[name] = a
    df = pd.DataFrame({**cols, "v": _ints_as_f64(rng, n)})
    keys = list(cols)
    exp = _sum_count(df, keys)
    for k in keys:
        exp[k] = exp[k].astype("float64")
    assert exp[keys].isna().any().all()          # rows in each NULL group
    t = f"gbf_nk{nkeys}"
    ks = ", ".join(keys)
    _check(ctx, monkeypatch, t, df,
           f"SELECT {ks}, SUM(v) AS s, COUNT(*) AS c FROM {t} GROUP BY {ks}",
           keys, exp, DIRECT)


def test_single_f64_key_with_nan_null_and_signed_zero(ctx, monkeypatch):
    n = 2000
    rng = np.random.default_rng(8)
    x = rng.choice([1.5, -2.5, 0.0, -0.0, np.nan, 1e300, -1e-300], n)
    df = pd.DataFrame({"x": x, "w": rng.integers(-9, 9, n).astype(np.int64)})
    g = df.groupby("x", dropna=False, sort=False)
    exp = pd.DataFrame({"c": g.size(), "sw": g["w"].sum()}).reset_index()
    assert len(exp) == 6                          # ±0.0 one group, NaN one
    _check(ctx, monkeypatch, "gbf_f64", df,
           "SELECT x, COUNT(*) AS c, SUM(w) AS sw FROM gbf_f64 GROUP BY x",
           ["x"], exp, GLOBAL)


def _mixed_frame(rng, n, mult):
    k = rng.integers(0, 5, n).astype(np.int64)
    x = pd.array(rng.integers(-50, 50, n), dtype="Int64")
    x[rng.random(n) < 0.3] = pd.NA
    x[k == 4] = pd.NA                             # a group with no input
    return pd.DataFrame({"k": k * mult, "f": _ints_as_f64(rng, n),
                         "i": rng.integers(-10**12, 10**12, n), "x": x})


@pytest.mark.parametrize("mult,family", [(1, DIRECT), (1_000_000, GLOBAL)],
                         ids=["direct", "global"])
def test_every_finalize_kind_in_one_query(ctx, monkeypatch, mult, family):
    """COUNT(*) sits between value aggregates, so accumulator and value-slot
    numbering differ; x is nullable (per-aggregate counts), and group k = 4
    has no non-NULL x at all."""
    df = _mixed_frame(np.random.default_rng(9 + mult), 3000, mult)
    g = df.groupby("k", sort=False)
    exp = pd.DataFrame({
        "sf": g["f"].sum(), "si": g["i"].sum(), "c": g.size(),
        "cx": g["x"].count(), "af": g["f"].mean(), "mni": g["i"].min(),
        "mxi": g["i"].max(), "mnf": g["f"].min(), "mxf": g["f"].max(),
        "sx": g["x"].sum(min_count=1).astype("float64"),
        "mnx": g["x"].min().astype("float64"),
        "ax": g["x"].mean().astype("float64")}).reset_index()
    assert exp["sx"].isna().sum() == 1 and (exp["mnf"] < 0).all()
    t = f"gbf_all{mult}"
    _check(ctx, monkeypatch, t, df,
           "SELECT k, SUM(f) AS sf, SUM(i) AS si, COUNT(*) AS c, "
           "COUNT(x) AS cx, AVG(f) AS af, MIN(i) AS mni, MAX(i) AS mxi, "
           "MIN(f) AS mnf, MAX(f) AS mxf, SUM(x) AS sx, MIN(x) AS mnx, "
           f"AVG(x) AS ax FROM {t} GROUP BY k", ["k"], exp, family)


def test_partition_path_value_slots_skip_count(ctx, monkeypatch):
    """Never-NULL inputs over a large key space: the AoS records hold no
    slot for COUNT(*), which sits between the value aggregates."""
    n = 4000
    rng = np.random.default_rng(11)
    df = pd.DataFrame({"k": rng.integers(0, 300, n).astype(np.int64) * 9973,
                       "f": _ints_as_f64(rng, n),
                       "i": rng.integers(-10**12, 10**12, n)})
    g = df.groupby("k", sort=False)
    exp = pd.DataFrame({
        "sf": g["f"].sum(), "c": g.size(), "mni": g["i"].min(),
        "mxf": g["f"].max(), "af": g["f"].mean(),
        "si": g["i"].sum()}).reset_index()
    _check(ctx, monkeypatch, "gbf_slots", df,
           "SELECT k, SUM(f) AS sf, COUNT(*) AS c, MIN(i) AS mni, "
           "MAX(f) AS mxf, AVG(f) AS af, SUM(i) AS si FROM gbf_slots "
           "GROUP BY k", ["k"], exp, PART)


def test_stddev_keeps_the_eval_programs(ctx, monkeypatch):
    n = 3000
    rng = np.random.default_rng(12)
    df = pd.DataFrame({"k": rng.integers(0, 6, n).astype(np.int64),
                       "f": _ints_as_f64(rng, n)})
    g = df.groupby("k", sort=False)
    exp = pd.DataFrame({"sd": g["f"].std(), "s": g["f"].sum()}).reset_index()
    _check(ctx, monkeypatch, "gbf_std", df,
           "SELECT k, STDDEV(f) AS sd, SUM(f) AS s FROM gbf_std GROUP BY k",
           ["k"], exp, DIRECT, declined=True)


def test_composite_key_with_float_member_keeps_the_eval_programs(
        ctx, monkeypatch):
    n = 3000
    rng = np.random.default_rng(13)
    df = pd.DataFrame({"k": rng.integers(0, 4, n).astype(np.int64),
                       "x": rng.choice([0.5, -1.25, 3.0], n),
                       "w": rng.integers(-9, 9, n).astype(np.int64)})
    g = df.groupby(["k", "x"], sort=False)
    exp = pd.DataFrame({"c": g.size(), "sw": g["w"].sum()}).reset_index()
    _check(ctx, monkeypatch, "gbf_fk", df,
           "SELECT k, x, COUNT(*) AS c, SUM(w) AS sw FROM gbf_fk "
           "GROUP BY k, x", ["k", "x"], exp, None, declined=True)


@pytest.mark.parametrize("n", [65_535, 65_793], ids=["below", "above"])
def test_partition_grid_on_both_sides_of_the_rows_per_block_rule(
        ctx, monkeypatch, n):
    """The partition grid is min(2048, ceil(n / 256), max(256, largest power
    of two g with g * nb <= n)). At a key space of 4 000 000 (nb = 984) the
    last term is 256, so the rule first lowers the grid where ceil(n / 256)
    passes 256: 256 blocks at n = 65 535 as before, and 256 instead of 258
    at n = 65 793. Neither n is a multiple of 256."""
    rng = np.random.default_rng(n)
    k = rng.integers(0, 4_000_000, n)
    k[0], k[1] = 0, 3_999_999
    df = pd.DataFrame({"k": k.astype(np.int64), "v": _ints_as_f64(rng, n)})
    t = f"gbf_grid{n}"
    _check(ctx, monkeypatch, t, df, SQL_SC.format(t=t), ["k"],
           _sum_count(df, ["k"]), PART)
