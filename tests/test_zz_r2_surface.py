"""Round-2 late SQL-surface execution tests (-m gpu), in a file that
sorts LAST so an unvalidated failure here cannot mask the established
parity suites under the driver's `pytest -x` (these paths were added while
the round's GPU pool was closed: plans and lowerings are CPU-verified, the
kernels they route through are the already-GPU-validated ones)."""
import numpy as np
import pandas as pd
import pytest

from tests.conftest import assert_frame_close
from tests.test_gpu_semantics import ctx, _rand_frame  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]
# the timeout bounds a hang in these UNVALIDATED paths to a test failure
# instead of a dead GPU box (pytest-timeout is in the image)


def test_cte_end_to_end(ctx):
    rng = np.random.default_rng(61)
    df = _rand_frame(rng, 20_000, with_nulls=False)
    ctx.create_table("tcte", df)
    out = ctx.sql(
        "WITH big AS (SELECT k, w FROM tcte WHERE w > 5) "
        "SELECT k, COUNT(*) AS n, SUM(w) AS s FROM big GROUP BY k").compute()
    sub = df[df["w"] > 5]
    exp = sub.groupby("k", as_index=False).agg(n=("w", "size"),
                                               s=("w", "sum"))
    assert_frame_close(out.sort_values("k").reset_index(drop=True),
                       exp.sort_values("k").reset_index(drop=True))


def test_cte_multiple_refs(ctx):
    # one CTE referenced twice (self-join through the definition)
    df = pd.DataFrame({"a": np.arange(50, dtype=np.int64),
                       "b": np.arange(50, dtype=np.int64) % 7})
    ctx.create_table("tcm", df)
    out = ctx.sql(
        "WITH f AS (SELECT a, b FROM tcm WHERE a < 30) "
        "SELECT x.a FROM f x JOIN f y ON x.a = y.b").compute()
    sub = df[df["a"] < 30]
    exp = sub.merge(sub, left_on="a", right_on="b")["a_x"]
    assert sorted(out["a"].astype(np.int64).tolist()) == \
        sorted(exp.tolist())


def test_intersect_except_nulls(ctx):
    # NULL keys compare EQUAL in set operations (DataFusion rewrites
    # Intersect/Except with null_equals_null=true)
    a = pd.DataFrame({"v": pd.array([1, None, 2], dtype="Int64")})
    b = pd.DataFrame({"v": pd.array([None, 2, 5], dtype="Int64")})
    ctx.create_table("tsn_a", a)
    ctx.create_table("tsn_b", b)
    out = ctx.sql("SELECT v FROM tsn_a INTERSECT SELECT v FROM tsn_b"
                  ).compute()
    got = sorted(out["v"].tolist(), key=lambda x: (x is not None
                                                   and not pd.isna(x), x))
    assert len(got) == 2  # NULL and 2
    assert any(pd.isna(x) for x in got)
    assert 2 in [x for x in got if not pd.isna(x)]
    out = ctx.sql("SELECT v FROM tsn_a EXCEPT SELECT v FROM tsn_b"
                  ).compute()
    vals = out["v"].tolist()
    assert len(vals) == 1 and vals[0] == 1  # NULL matched, 2 matched


def test_intersect_except(ctx):
    a = pd.DataFrame({"v": np.array([1, 2, 2, 3, 4, 7], dtype=np.int64)})
    b = pd.DataFrame({"v": np.array([2, 3, 3, 5], dtype=np.int64)})
    ctx.create_table("tsa", a)
    ctx.create_table("tsb", b)
    out = ctx.sql("SELECT v FROM tsa INTERSECT SELECT v FROM tsb").compute()
    assert sorted(out["v"].astype(np.int64).tolist()) == [2, 3]
    out = ctx.sql("SELECT v FROM tsa EXCEPT SELECT v FROM tsb").compute()
    assert sorted(out["v"].astype(np.int64).tolist()) == [1, 4, 7]
    # mixed chain: EXCEPT over a UNION
    out = ctx.sql("SELECT v FROM tsa UNION SELECT v FROM tsb "
                  "EXCEPT SELECT v FROM tsb").compute()
    assert sorted(out["v"].astype(np.int64).tolist()) == [1, 4, 7]


def test_ilike_similar_escape(ctx):
    df = pd.DataFrame({
        "s": pd.Series(["Apple", "apricot", "Banana", "50% off", "plum"]
                       ).astype("category"),
        "v": np.arange(5, dtype=np.int64)})
    ctx.create_table("tlk", df)
    out = ctx.sql("SELECT v FROM tlk WHERE s ILIKE 'a%'").compute()
    assert sorted(out["v"].astype(np.int64).tolist()) == [0, 1]
    out = ctx.sql("SELECT v FROM tlk WHERE s SIMILAR TO '(A|B)%'").compute()
    assert sorted(out["v"].astype(np.int64).tolist()) == [0, 2]
    out = ctx.sql("SELECT v FROM tlk WHERE s LIKE '50!%%' ESCAPE '!'"
                  ).compute()
    assert sorted(out["v"].astype(np.int64).tolist()) == [3]
    out = ctx.sql("SELECT v FROM tlk WHERE s NOT ILIKE '%p%'").compute()
    # neither "Banana" nor "50% off" contains a p/P
    assert sorted(out["v"].astype(np.int64).tolist()) == [2, 3]


def test_datetime_trunc_exec(ctx):
    ts = pd.to_datetime([
        "2021-02-01 13:45:12.345", "2020-02-29 23:59:59.999",
        "1969-07-20 20:17:40", "2000-12-31 00:00:00",
        "2021-01-01 00:00:00"], format="mixed")
    df = pd.DataFrame({"ts": ts, "v": np.arange(5, dtype=np.int64)})
    ctx.create_table("tdt", df)
    out = ctx.sql("SELECT FLOOR(ts TO DAY) AS fd, CEIL(ts TO HOUR) AS ch, "
                  "FLOOR(ts TO MONTH) AS fm, FLOOR(ts TO YEAR) AS fy, "
                  "EXTRACT(DATE FROM ts) AS ed, v FROM tdt").compute()
    out = out.sort_values("v").reset_index(drop=True)
    s = pd.Series(ts)
    assert (pd.to_datetime(out["fd"]) == s.dt.floor("D")).all()
    assert (pd.to_datetime(out["ch"]) == s.dt.ceil("h")).all()
    assert (pd.to_datetime(out["fm"])
            == s.dt.to_period("M").dt.start_time).all()
    assert (pd.to_datetime(out["fy"])
            == s.dt.to_period("Y").dt.start_time).all()
    assert (pd.to_datetime(out["ed"]) == s.dt.normalize()).all()


def test_timestampadd_exec(ctx):
    ts = pd.to_datetime(["2021-02-27 10:00:00", "2020-12-31 23:30:00"])
    df = pd.DataFrame({"ts": ts, "v": np.arange(2, dtype=np.int64)})
    ctx.create_table("tta", df)
    out = ctx.sql("SELECT TIMESTAMPADD(DAY, 5, ts) AS d5, "
                  "TIMESTAMPADD(HOUR, -3, ts) AS h3, v FROM tta").compute()
    out = out.sort_values("v").reset_index(drop=True)
    s = pd.Series(ts)
    assert (pd.to_datetime(out["d5"]) == s + pd.Timedelta(days=5)).all()
    assert (pd.to_datetime(out["h3"]) == s - pd.Timedelta(hours=3)).all()


def test_is_true_family(ctx):
    df = pd.DataFrame({"k": np.array([0, 1, 2, 3], dtype=np.int64),
                       "w": pd.array([1, 0, None, 1], dtype="Int64")})
    ctx.create_table("tit", df)
    out = ctx.sql("SELECT k FROM tit WHERE (w = 1) IS TRUE").compute()
    assert sorted(out["k"].astype(np.int64).tolist()) == [0, 3]
    out = ctx.sql("SELECT k FROM tit WHERE (w = 1) IS NOT TRUE").compute()
    assert sorted(out["k"].astype(np.int64).tolist()) == [1, 2]
    out = ctx.sql("SELECT k FROM tit WHERE (w = 1) IS FALSE").compute()
    assert sorted(out["k"].astype(np.int64).tolist()) == [1]
    out = ctx.sql("SELECT k FROM tit WHERE (w = 1) IS UNKNOWN").compute()
    assert sorted(out["k"].astype(np.int64).tolist()) == [2]


def test_position_exec(ctx):
    df = pd.DataFrame({
        "s": pd.Series(["banana", "apple", "kiwi"]).astype("category"),
        "v": np.arange(3, dtype=np.int64)})
    ctx.create_table("tpos", df)
    out = ctx.sql("SELECT POSITION('an' IN s) AS p, "
                  "POSITION('a' IN s FROM 3) AS q, v FROM tpos").compute()
    out = out.sort_values("v").reset_index(drop=True)
    assert out["p"].astype(np.int64).tolist() == [2, 0, 0]
    assert out["q"].astype(np.int64).tolist() == [4, 0, 0]


def test_interval_string_and_comments(ctx):
    d = pd.to_datetime(["2021-01-01", "2021-01-10", "2021-02-01"])
    df = pd.DataFrame({"d": d, "v": np.arange(3, dtype=np.int64)})
    ctx.create_table("tic", df)
    out = ctx.sql("SELECT v -- pick v\n"
                  "FROM tic /* range */ "
                  "WHERE d < DATE '2021-01-01' + INTERVAL '5 days'"
                  ).compute()
    assert sorted(out["v"].astype(np.int64).tolist()) == [0]


def test_regr_covar_family(ctx):
    rng = np.random.default_rng(71)
    n = 4000
    df = pd.DataFrame({
        "name": pd.Series(rng.choice(["a", "b", "c"], n)).astype("category"),
        "x": np.round(rng.random(n), 3), "y": np.round(rng.random(n), 3)})
    df.loc[rng.random(n) < 0.1, "x"] = np.nan
    df.loc[rng.random(n) < 0.1, "y"] = np.nan
    ctx.create_table("trc", df)
    out = ctx.sql(
        "SELECT name, REGR_COUNT(y, x) AS n, REGR_SXX(y, x) AS sxx, "
        "REGR_SYY(y, x) AS syy, COVAR_POP(y, x) AS cp, "
        "COVAR_SAMP(y, x) AS cs FROM trc GROUP BY name").compute()
    out = out.sort_values("name").reset_index(drop=True)
    pair = df.dropna(subset=["x", "y"])
    for i, (g, sub) in enumerate(pair.groupby("name", observed=True)):
        assert out.loc[i, "name"] == g
        N = len(sub)
        assert int(out.loc[i, "n"]) == N
        sxx = ((sub.x - sub.x.mean()) ** 2).sum()
        syy = ((sub.y - sub.y.mean()) ** 2).sum()
        cp = ((sub.x - sub.x.mean()) * (sub.y - sub.y.mean())).sum() / N
        cs = cp * N / (N - 1)
        assert abs(out.loc[i, "sxx"] - sxx) < 1e-6 * max(1, abs(sxx))
        assert abs(out.loc[i, "syy"] - syy) < 1e-6 * max(1, abs(syy))
        assert abs(out.loc[i, "cp"] - cp) < 1e-6 * max(1, abs(cp))
        assert abs(out.loc[i, "cs"] - cs) < 1e-6 * max(1, abs(cs))


# ---- reference integration cases ported verbatim ---------------------------
def test_ref_sort_with_nan_matrix(ctx):
    """reference test_sort.py:92 — full NULLS FIRST/LAST × ASC/DESC matrix
    over a float key with NaN (float sort keys take the stable host path)."""
    df = pd.DataFrame(
        {"a": [1, 2, float("nan"), 2],
         "b": [4, float("nan"), 5, float("inf")]})
    ctx.create_table("zz_sortnan", df)
    cases = [
        ("ORDER BY a", [1, 2, 2, None], [4, None, float("inf"), 5]),
        ("ORDER BY a NULLS FIRST", [None, 1, 2, 2],
         [5, 4, None, float("inf")]),
        ("ORDER BY a NULLS LAST", [1, 2, 2, None],
         [4, None, float("inf"), 5]),
        ("ORDER BY a DESC", [None, 2, 2, 1], [5, None, float("inf"), 4]),
        ("ORDER BY a DESC NULLS LAST", [2, 2, 1, None],
         [None, float("inf"), 4, 5]),
    ]
    for tail, ea, eb in cases:
        out = ctx.sql(f"SELECT * FROM zz_sortnan {tail}").compute()
        got_a = out["a"].tolist()
        got_b = out["b"].tolist()
        for g, w in zip(got_a, ea):
            if w is None:
                assert np.isnan(g), (tail, got_a)
            else:
                assert g == w, (tail, got_a)
        for g, w in zip(got_b, eb):
            if w is None:
                assert np.isnan(g), (tail, got_b)
            else:
                assert g == w, (tail, got_b)


def test_ref_sort_strings(ctx):
    # reference test_sort.py:280
    df = pd.DataFrame({"a": [1, 2, 3],
                       "b": pd.Series(["zzhsd", "öfjdf", "baba"]
                                      ).astype("category")})
    ctx.create_table("zz_sortstr", df)
    out = ctx.sql("SELECT * FROM zz_sortstr ORDER BY b").compute()
    # pandas codepoint order: baba < zzhsd < öfjdf (ö = U+00F6 sorts after
    # z — the reference compares with pandas sort_values)
    assert out["a"].astype(np.int64).tolist() == [3, 1, 2]


def test_ref_sort_by_alias(ctx):
    # reference test_sort.py:73 — ORDER BY a projected alias
    df = pd.DataFrame({"user_id": [3, 1, 2], "b": [1.0, 2.0, 3.0]})
    ctx.create_table("zz_alias", df)
    out = ctx.sql("SELECT b AS my_column FROM zz_alias "
                  "ORDER BY my_column DESC").compute()
    assert out["my_column"].tolist() == [3.0, 2.0, 1.0]


def test_ref_string_filter_like(ctx):
    # reference test_filter.py:62 — LIKE with regex metachars in the data
    df = pd.DataFrame({"a": pd.Series(
        ["a normal string", "%_%", "^|()-*[]$"]).astype("category")})
    ctx.create_table("zz_strf", df)
    out = ctx.sql("SELECT * FROM zz_strf WHERE a LIKE '%n%'").compute()
    assert out["a"].tolist() == ["a normal string"]
    out = ctx.sql("SELECT * FROM zz_strf WHERE a LIKE '%|%'").compute()
    assert out["a"].tolist() == ["^|()-*[]$"]


def test_ref_filter_year(ctx):
    # reference test_filter.py:130
    df = pd.DataFrame({"dt": pd.to_datetime(
        ["2021-01-02", "2022-03-04", "2023-05-06"]), "x": [1, 2, 3]})
    ctx.create_table("zz_fy", df)
    out = ctx.sql("SELECT x FROM zz_fy WHERE year(dt) < 2023").compute()
    assert sorted(out["x"].astype(np.int64).tolist()) == [1, 2]


def test_ref_filter_scalar_literals(ctx):
    # reference test_filter.py:20 — constant predicates
    df = _rand_frame(np.random.default_rng(5), 100, with_nulls=False)
    ctx.create_table("zz_fs", df)
    assert len(ctx.sql("SELECT * FROM zz_fs WHERE True").compute()) == 100
    assert len(ctx.sql("SELECT * FROM zz_fs WHERE False").compute()) == 0
    assert len(ctx.sql("SELECT * FROM zz_fs WHERE (1 = 1)").compute()) \
        == 100
    assert len(ctx.sql("SELECT * FROM zz_fs WHERE (1 = 0)").compute()) == 0


def test_ref_aggregations_bit_every_single(ctx):
    # reference test_groupby.py:205 — EVERY/BIT_AND/BIT_OR/MIN/
    # SINGLE_VALUE/AVG over user_table_1/2 with the exact expected frames
    u1 = pd.DataFrame({"user_id": [2, 1, 2, 3], "b": [3, 3, 1, 3]})
    u2 = pd.DataFrame({"user_id": [1, 1, 2, 4], "c": [1, 2, 3, 4]})
    ctx.create_table("zz_u1", u1)
    ctx.create_table("zz_u2", u2)
    out = ctx.sql(
        "SELECT user_id, EVERY(b = 3) AS e, BIT_AND(b) AS b, "
        "BIT_OR(b) AS bb, MIN(b) AS m, SINGLE_VALUE(b) AS s, AVG(b) AS a "
        "FROM zz_u1 GROUP BY user_id").compute()
    out = out.sort_values("user_id").reset_index(drop=True)
    assert out["user_id"].astype(np.int64).tolist() == [1, 2, 3]
    assert out["e"].astype(bool).tolist() == [True, False, True]
    assert out["b"].astype(np.int64).tolist() == [3, 1, 3]
    assert out["bb"].astype(np.int64).tolist() == [3, 3, 3]
    assert out["m"].astype(np.int64).tolist() == [3, 1, 3]
    assert out["a"].astype(float).tolist() == [3.0, 2.0, 3.0]
    out = ctx.sql(
        "SELECT user_id, EVERY(c = 3) AS e, BIT_AND(c) AS b, "
        "BIT_OR(c) AS bb, MIN(c) AS m, AVG(c) AS a "
        "FROM zz_u2 GROUP BY user_id").compute()
    out = out.sort_values("user_id").reset_index(drop=True)
    assert out["user_id"].astype(np.int64).tolist() == [1, 2, 4]
    assert out["e"].astype(bool).tolist() == [False, True, False]
    assert out["b"].astype(np.int64).tolist() == [0, 3, 4]
    assert out["bb"].astype(np.int64).tolist() == [3, 3, 4]
    assert out["a"].astype(float).tolist() == [1.5, 3.0, 4.0]


def test_ref_groupby_string_minmax(ctx):
    # reference test_groupby.py:205 tail — MIN/MAX over a string column
    df = pd.DataFrame({"a": pd.Series(
        ["a normal string", "%_%", "^|()-*[]$"]).astype("category")})
    ctx.create_table("zz_sminmax", df)
    out = ctx.sql('SELECT MAX(a) AS "max", MIN(a) AS "min" '
                  "FROM zz_sminmax").compute()
    assert out["max"].tolist() == ["a normal string"]
    assert out["min"].tolist() == ["%_%"]


def test_ref_union_cases(ctx):
    # reference test_union.py — UNION dedups, UNION ALL concatenates,
    # mixed-alias branches align positionally
    rng = np.random.default_rng(9)
    df = pd.DataFrame({"a": [1.0] * 10 + [2.0] * 20 + [3.0] * 40,
                       "b": np.round(10 * rng.random(70), 3)})
    lt = pd.DataFrame({"a": [0] * 10 + [1] * 11 + [2] * 13})
    ctx.create_table("zz_udf", df)
    ctx.create_table("zz_ult", lt)
    out = ctx.sql("SELECT * FROM zz_udf UNION SELECT * FROM zz_udf "
                  "UNION SELECT * FROM zz_udf").compute()
    exp = df.drop_duplicates()
    assert len(out) == len(exp)
    out = ctx.sql("SELECT * FROM zz_udf UNION ALL SELECT * FROM zz_udf "
                  "UNION ALL SELECT * FROM zz_udf").compute()
    assert len(out) == 3 * len(df)
    out = ctx.sql('SELECT a AS "I", b AS "II" FROM zz_udf UNION ALL '
                  'SELECT a AS "I", a AS "II" FROM zz_ult').compute()
    exp_i = sorted(df["a"].tolist() + [float(x) for x in lt["a"]])
    assert sorted(out["I"].astype(float).tolist()) == exp_i
    assert len(out.columns) == 2


def test_ref_cross_join(ctx):
    # reference test_join.py cross join via comma-FROM with TRUE condition
    d1 = pd.DataFrame({"a": [1, 2, 3]})
    d2 = pd.DataFrame({"b": [10, 20]})
    ctx.create_table("zz_c1", d1)
    ctx.create_table("zz_c2", d2)
    out = ctx.sql("SELECT * FROM zz_c1 CROSS JOIN zz_c2").compute()
    assert len(out) == 6
    assert sorted(out["a"].astype(np.int64).tolist()) == [1, 1, 2, 2, 3, 3]


def test_float_key_join(ctx):
    # f64 equi-join keys densify to consistent ids (bits-mode groupby over
    # the concatenated pair); NaN matches NaN like pandas merge, NULL drops
    lhs = pd.DataFrame({"x": [1.5, 2.5, np.nan, -0.0, 7.25],
                        "lv": np.arange(5, dtype=np.int64)})
    rhs = pd.DataFrame({"x": [2.5, np.nan, 0.0, 9.0],
                        "rv": np.arange(4, dtype=np.int64)})
    ctx.create_table("zz_fl", lhs)
    ctx.create_table("zz_fr", rhs)
    out = ctx.sql("SELECT l.lv, r.rv FROM zz_fl l JOIN zz_fr r "
                  "ON l.x = r.x").compute()
    got = sorted(zip(out["lv"].astype(np.int64),
                     out["rv"].astype(np.int64)))
    # 2.5↔2.5 and -0.0↔0.0 match. A NaN in a float64 frame IS the NULL
    # (pandas has no other), and an INNER join drops NULL keys on both
    # sides: the reference filters `isna()` keys before its merge
    # (rel/logical/join.py:198-213), as SQL requires and as the sqlite
    # corpus (test_zz_sqlite_compat.py joins on NULL-bearing float keys)
    # checks — so the NaN rows pair with nothing.
    assert got == [(1, 0), (3, 2)], got


def test_ref_complex_query(ctx):
    """reference test_complex.py:4 — self-join of a timeseries on
    (name, MAX(x)) — a composite join key with a FLOAT member."""
    rng = np.random.default_rng(13)
    n = 5000
    df = pd.DataFrame({
        "name": pd.Series(rng.choice(["Alice", "Bob", "Xavier"], n)
                          ).astype("category"),
        "id": rng.integers(0, 100, n).astype(np.int64),
        "x": np.round(rng.random(n) * 2 - 1, 6)})
    ctx.create_table("zz_timeseries", df)
    result = ctx.sql(
        "SELECT lhs.name, lhs.id, lhs.x FROM zz_timeseries AS lhs "
        "JOIN (SELECT name AS max_name, MAX(x) AS max_x "
        "      FROM zz_timeseries GROUP BY name) AS rhs "
        "ON lhs.name = rhs.max_name AND lhs.x = rhs.max_x").compute()
    assert len(result) > 0
    exp = df.merge(
        df.groupby("name", observed=True)["x"].max().reset_index()
          .rename(columns={"name": "max_name", "x": "max_x"}),
        left_on=["name", "x"], right_on=["max_name", "max_x"])
    assert len(result) == len(exp)
    assert sorted(result["x"].tolist()) == sorted(exp["x"].tolist())


def test_ref_overlay(ctx):
    # reference test_rex.py OVERLAY rows (the exact expected strings from
    # OverlayOperation semantics)
    df = pd.DataFrame({"a": pd.Series(["a normal string"]
                                      ).astype("category")})
    ctx.create_table("zz_ov", df)
    out = ctx.sql(
        "SELECT OVERLAY(a PLACING 'XXX' FROM -1) AS l, "
        "OVERLAY(a PLACING 'XXX' FROM 2 FOR 4) AS m, "
        "OVERLAY(a PLACING 'XXX' FROM 2 FOR 1) AS n FROM zz_ov").compute()
    s = "a normal string"
    def ov(s, repl, start, length=None):
        st = 0 if start <= 0 else start - 1
        ln = len(repl) if length is None else length
        return s[:st] + repl + s[st + ln:]
    assert out["l"].tolist() == [ov(s, "XXX", -1)]
    assert out["m"].tolist() == [ov(s, "XXX", 2, 4)]
    assert out["n"].tolist() == [ov(s, "XXX", 2, 1)]


# ---- TPC-H shapes unlocked by round-2 planner work -------------------------
@pytest.fixture(scope="module")
def tpch2(ctx):
    rng = np.random.default_rng(21)
    n = 30_000
    lineitem = pd.DataFrame({
        "l_suppkey": rng.integers(0, 200, n).astype(np.int64),
        "l_partkey": rng.integers(0, 400, n).astype(np.int64),
        "l_quantity": rng.integers(1, 50, n).astype(np.int64),
        "l_extendedprice": np.round(rng.random(n) * 1000, 2),
        "l_discount": np.round(rng.random(n) * 0.1, 2),
        "l_shipdate": pd.to_datetime("1995-01-01")
        + pd.to_timedelta(rng.integers(0, 700, n), unit="D"),
    })
    supplier = pd.DataFrame({
        "s_suppkey": np.arange(200, dtype=np.int64),
        "s_nationkey": rng.integers(0, 25, 200).astype(np.int64)})
    part = pd.DataFrame({
        "p_partkey": np.arange(400, dtype=np.int64),
        "p_brand": pd.Series(rng.choice(["Brand#1", "Brand#2", "Brand#3"],
                                        400)).astype("category"),
        "p_size": rng.integers(1, 50, 400).astype(np.int64)})
    ctx.create_table("t2_lineitem", lineitem)
    ctx.create_table("t2_supplier", supplier)
    ctx.create_table("t2_part", part)
    return lineitem, supplier, part


def test_q15_shape_cte_scalar_max(ctx, tpch2):
    """Q15: CTE revenue view + uncorrelated scalar MAX subquery over it."""
    lineitem, supplier, part = tpch2
    out = ctx.sql(
        "WITH revenue AS ("
        "  SELECT l_suppkey AS supplier_no, "
        "         SUM(l_extendedprice * (1 - l_discount)) AS total_rev "
        "  FROM t2_lineitem "
        "  WHERE l_shipdate >= DATE '1995-06-01' "
        "    AND l_shipdate < DATE '1995-06-01' + INTERVAL '3' MONTH "
        "  GROUP BY l_suppkey) "
        "SELECT s_suppkey, total_rev FROM t2_supplier "
        "JOIN revenue ON s_suppkey = supplier_no "
        "WHERE total_rev = (SELECT MAX(total_rev) FROM revenue)").compute()
    li = lineitem[(lineitem.l_shipdate >= "1995-06-01")
                  & (lineitem.l_shipdate < "1995-09-01")]
    rev = li.assign(r=li.l_extendedprice * (1 - li.l_discount)) \
        .groupby("l_suppkey")["r"].sum()
    best = rev.max()
    exp = rev[np.isclose(rev, best)]
    assert len(out) == len(exp)
    assert sorted(out["s_suppkey"].astype(np.int64).tolist()) == \
        sorted(exp.index.tolist())


def test_q16_shape_not_in_count_distinct(ctx, tpch2):
    """Q16: NOT IN subquery + COUNT(DISTINCT) grouped by part attrs."""
    lineitem, supplier, part = tpch2
    out = ctx.sql(
        "SELECT p_brand, COUNT(DISTINCT l_suppkey) AS supplier_cnt "
        "FROM t2_lineitem JOIN t2_part ON l_partkey = p_partkey "
        "WHERE p_size < 25 AND l_suppkey NOT IN "
        "  (SELECT s_suppkey FROM t2_supplier WHERE s_nationkey = 7) "
        "GROUP BY p_brand").compute()
    bad = set(supplier[supplier.s_nationkey == 7].s_suppkey)
    j = lineitem.merge(part, left_on="l_partkey", right_on="p_partkey")
    j = j[(j.p_size < 25) & ~j.l_suppkey.isin(bad)]
    exp = j.groupby("p_brand", observed=True)["l_suppkey"].nunique()
    got = dict(zip(out["p_brand"], out["supplier_cnt"].astype(np.int64)))
    assert got == exp.to_dict()


def test_q19_shape_or_groups(ctx, tpch2):
    """Q19: disjunction of conjunct groups over join output."""
    lineitem, supplier, part = tpch2
    out = ctx.sql(
        "SELECT SUM(l_extendedprice * (1 - l_discount)) AS revenue "
        "FROM t2_lineitem JOIN t2_part ON p_partkey = l_partkey "
        "WHERE (p_brand = 'Brand#1' AND l_quantity BETWEEN 1 AND 11) "
        "   OR (p_brand = 'Brand#2' AND l_quantity BETWEEN 10 AND 20) "
        "   OR (p_brand = 'Brand#3' AND l_quantity BETWEEN 20 AND 30)"
        ).compute()
    j = lineitem.merge(part, left_on="l_partkey", right_on="p_partkey")
    m = ((j.p_brand == "Brand#1") & j.l_quantity.between(1, 11)) \
        | ((j.p_brand == "Brand#2") & j.l_quantity.between(10, 20)) \
        | ((j.p_brand == "Brand#3") & j.l_quantity.between(20, 30))
    exp = (j[m].l_extendedprice * (1 - j[m].l_discount)).sum()
    assert abs(float(out["revenue"][0]) - exp) < 1e-6 * max(1.0, abs(exp))


def test_q18_shape_in_grouped_having(ctx, tpch2):
    """Q18: IN over a grouped HAVING subquery."""
    lineitem, supplier, part = tpch2
    out = ctx.sql(
        "SELECT l_suppkey, SUM(l_quantity) AS tq FROM t2_lineitem "
        "WHERE l_suppkey IN (SELECT l_suppkey FROM t2_lineitem "
        "                    GROUP BY l_suppkey HAVING SUM(l_quantity) > "
        "                    4000) "
        "GROUP BY l_suppkey").compute()
    tq = lineitem.groupby("l_suppkey")["l_quantity"].sum()
    big = tq[tq > 4000]
    assert len(out) == len(big)
    got = dict(zip(out["l_suppkey"].astype(np.int64),
                   out["tq"].astype(np.int64)))
    assert got == {int(k): int(v) for k, v in big.items()}


def test_to_timestamp_exec(ctx):
    # reference ToTimestampOperation: integer seconds, string strptime
    df = pd.DataFrame({
        "secs": np.array([0, 86_400, 1_600_000_000], dtype=np.int64),
        "txt": pd.Series(["01/02/2021", "03/15/2020", "12/31/1999"]
                         ).astype("category"),
        "v": np.arange(3, dtype=np.int64)})
    ctx.create_table("zz_tts", df)
    out = ctx.sql('SELECT to_timestamp(secs) AS a, '
                  'to_timestamp(txt, "%m/%d/%Y") AS b, v FROM zz_tts'
                  ).compute()
    out = out.sort_values("v").reset_index(drop=True)
    assert (pd.to_datetime(out["a"])
            == pd.to_datetime(df["secs"], unit="s")).all()
    assert (pd.to_datetime(out["b"])
            == pd.to_datetime(df["txt"].astype(str),
                              format="%m/%d/%Y")).all()


def test_trig_math_family(ctx):
    # reference rex/core/call.py trigonometry + da.degrees/log10/cbrt/
    # sign/trunc — vs numpy on the same values
    x = np.array([0.5, -1.2, 0.0, 2.9, -0.001], dtype=np.float64)
    a = np.array([3, -4, 0, 7, -1], dtype=np.int64)
    df = pd.DataFrame({"x": x, "a": a, "v": np.arange(5, dtype=np.int64)})
    ctx.create_table("zz_trig", df)
    out = ctx.sql(
        "SELECT SIN(x) AS s, COS(x) AS c, TAN(x) AS t, ATAN(x) AS at, "
        "ATAN2(x, 1 + 0 * v) AS a2, COT(x + 2) AS ct, DEGREES(x) AS dg, "
        "RADIANS(x) AS rd, LOG10(ABS(x) + 1) AS lg, CBRT(x) AS cb, "
        "SIGN(x) AS sgf, SIGN(a) AS sgi, TRUNCATE(x * 3) AS tr, v "
        "FROM zz_trig").compute()
    out = out.sort_values("v").reset_index(drop=True)
    np.testing.assert_allclose(out["s"], np.sin(x), rtol=1e-12)
    np.testing.assert_allclose(out["c"], np.cos(x), rtol=1e-12)
    np.testing.assert_allclose(out["t"], np.tan(x), rtol=1e-12)
    np.testing.assert_allclose(out["at"], np.arctan(x), rtol=1e-12)
    np.testing.assert_allclose(out["a2"], np.arctan2(x, 1.0), rtol=1e-12)
    np.testing.assert_allclose(out["ct"], 1 / np.tan(x + 2), rtol=1e-12)
    np.testing.assert_allclose(out["dg"], np.degrees(x), rtol=1e-12)
    np.testing.assert_allclose(out["rd"], np.radians(x), rtol=1e-12)
    np.testing.assert_allclose(out["lg"], np.log10(np.abs(x) + 1),
                               rtol=1e-12)
    np.testing.assert_allclose(out["cb"], np.cbrt(x), rtol=1e-12)
    np.testing.assert_allclose(out["sgf"], np.sign(x))
    assert out["sgi"].astype(np.int64).tolist() == [1, -1, 0, 1, -1]
    np.testing.assert_allclose(out["tr"], np.trunc(x * 3))


def test_float_mod_and_mean(ctx):
    # reference MOD on floats = operator.mod (floor semantics); MEAN = AVG
    df = pd.DataFrame({"b": [7.5, -7.5, 2.3], "a": [3, 3, 3],
                       "v": np.arange(3, dtype=np.int64)})
    ctx.create_table("zz_fm", df)
    out = ctx.sql("SELECT MOD(b, 4) AS m, v FROM zz_fm").compute()
    out = out.sort_values("v").reset_index(drop=True)
    np.testing.assert_allclose(out["m"], df["b"] % 4, rtol=1e-12)
    out = ctx.sql("SELECT MEAN(b) AS mb, MEAN(a) AS ma FROM zz_fm"
                  ).compute()
    assert abs(float(out["mb"][0]) - df["b"].mean()) < 1e-12
    assert abs(float(out["ma"][0]) - 3.0) < 1e-12


def test_month_interval_on_column(ctx):
    # calendar month/year arithmetic on a COLUMN runs the host UDF path
    # (pandas DateOffset — end-of-month clamping included)
    ts = pd.to_datetime(["2021-01-31 10:00:00", "2020-02-29 23:00:00",
                         "2019-12-15 00:30:00"])
    df = pd.DataFrame({"t": ts, "v": np.arange(3, dtype=np.int64)})
    ctx.create_table("zz_mi", df)
    out = ctx.sql("SELECT t + INTERVAL '1' MONTH AS a, "
                  "t - INTERVAL '2' MONTH AS b, "
                  "TIMESTAMPADD(YEAR, 1, t) AS y, v FROM zz_mi").compute()
    out = out.sort_values("v").reset_index(drop=True)
    s = pd.Series(ts)
    assert (pd.to_datetime(out["a"])
            == s + pd.DateOffset(months=1)).all()
    assert (pd.to_datetime(out["b"])
            == s - pd.DateOffset(months=2)).all()
    assert (pd.to_datetime(out["y"])
            == s + pd.DateOffset(months=12)).all()


def test_month_interval_on_date_column(ctx):
    d = pd.to_datetime(["2021-01-31", "2020-02-29", "2019-12-15"])
    df = pd.DataFrame({"d": d, "v": np.arange(3, dtype=np.int64)})
    ctx.create_table("zz_mid", df)
    out = ctx.sql("SELECT d + INTERVAL '1' MONTH AS a, v FROM zz_mid"
                  ).compute()
    out = out.sort_values("v").reset_index(drop=True)
    assert (pd.to_datetime(out["a"])
            == pd.Series(d) + pd.DateOffset(months=1)).all()


def test_extract_week_exec(ctx):
    d = pd.to_datetime(["2021-01-04", "2021-01-03", "2020-12-31",
                        "2019-12-30"])
    df = pd.DataFrame({"d": d, "v": np.arange(4, dtype=np.int64)})
    ctx.create_table("zz_wk", df)
    out = ctx.sql("SELECT EXTRACT(WEEK FROM d) AS w, v FROM zz_wk"
                  ).compute()
    out = out.sort_values("v").reset_index(drop=True)
    want = pd.Series(d).dt.isocalendar().week.tolist()
    assert out["w"].astype(np.int64).tolist() == [int(x) for x in want]


def test_case_sensitive_quoted_aliases(ctx):
    # reference test_select.py casing test: quoted aliases differing only
    # in case resolve by exact match
    df = pd.DataFrame({"a": np.array([5, 6], dtype=np.int64),
                       "b": np.array([10, 20], dtype=np.int64)})
    ctx.create_table("zz_case", df)
    out = ctx.sql('SELECT "AAA", "aaa", "aAa" FROM '
                  '(SELECT a - 1 AS "aAa", 2*b AS "aaa", a + b AS "AAA" '
                  ' FROM zz_case) x').compute()
    assert out["AAA"].astype(np.int64).tolist() == [15, 26]
    assert out["aaa"].astype(np.int64).tolist() == [20, 40]
    assert out["aAa"].astype(np.int64).tolist() == [4, 5]


def test_window_rows_frames(ctx):
    # reference test_over.py ROWS BETWEEN cases — host rolling path
    df = pd.DataFrame({"a": np.array([1, 2, 3, 4, 5], dtype=np.int64),
                       "u": np.array([0, 0, 0, 1, 1], dtype=np.int64)})
    ctx.create_table("zz_wf", df)
    out = ctx.sql(
        'SELECT a, '
        'SUM(a) OVER (ORDER BY a ROWS BETWEEN 2 PRECEDING AND CURRENT '
        'ROW) AS o1, '
        'SUM(a) OVER (PARTITION BY u ORDER BY a ROWS BETWEEN 1 PRECEDING '
        'AND 1 FOLLOWING) AS o2, '
        'COUNT(a) OVER (ORDER BY a ROWS BETWEEN 1 PRECEDING AND CURRENT '
        'ROW) AS o3 FROM zz_wf').compute()
    out = out.sort_values("a").reset_index(drop=True)
    assert out["o1"].astype(np.int64).tolist() == [1, 3, 6, 9, 12]
    assert out["o2"].astype(np.int64).tolist() == [3, 6, 5, 9, 9]
    assert out["o3"].astype(np.int64).tolist() == [1, 2, 2, 2, 2]


def test_window_last_value_and_rowid_order(ctx):
    df = pd.DataFrame({"u": np.array([1, 1, 2, 2], dtype=np.int64),
                       "b": np.array([5.0, 7.0, 1.0, 3.0])})
    ctx.create_table("zz_lv", df)
    out = ctx.sql("SELECT u, b, "
                  "LAST_VALUE(b) OVER (PARTITION BY u ORDER BY b) AS lv, "
                  "SINGLE_VALUE(b) OVER (PARTITION BY u ORDER BY b) AS sv,"
                  " ROW_NUMBER() OVER (PARTITION BY u) AS rn "
                  "FROM zz_lv").compute()
    out = out.sort_values(["u", "b"]).reset_index(drop=True)
    # ordered default frame: LAST_VALUE = current row, SINGLE/FIRST = head
    assert out["lv"].tolist() == [5.0, 7.0, 1.0, 3.0]
    assert out["sv"].tolist() == [5.0, 5.0, 1.0, 1.0]
    assert sorted(out[out.u == 1]["rn"].astype(np.int64).tolist()) == [1, 2]


def test_q2_shape_correlated_min(ctx):
    """Q2: correlated scalar MIN subquery with an UNQUALIFIED outer
    reference, over a 4-table join."""
    rng = np.random.default_rng(41)
    part = pd.DataFrame({"p_partkey": np.arange(50, dtype=np.int64),
                         "p_size": rng.integers(1, 10, 50).astype(np.int64)})
    supplier = pd.DataFrame({
        "s_suppkey": np.arange(20, dtype=np.int64),
        "s_nationkey": rng.integers(0, 5, 20).astype(np.int64),
        "s_acctbal": np.round(rng.random(20) * 1000, 2)})
    partsupp = pd.DataFrame({
        "ps_partkey": rng.integers(0, 50, 300).astype(np.int64),
        "ps_suppkey": rng.integers(0, 20, 300).astype(np.int64),
        "ps_supplycost": np.round(rng.random(300) * 100, 2)})
    nation = pd.DataFrame({"n_nationkey": np.arange(5, dtype=np.int64),
                           "n_regionkey": np.arange(5, dtype=np.int64) % 2})
    ctx.create_table("q2_part", part)
    ctx.create_table("q2_supplier", supplier)
    ctx.create_table("q2_partsupp", partsupp)
    ctx.create_table("q2_nation", nation)
    out = ctx.sql("""
        SELECT s_acctbal, s_suppkey, p_partkey
        FROM q2_part, q2_supplier, q2_partsupp, q2_nation
        WHERE p_partkey = ps_partkey AND s_suppkey = ps_suppkey
          AND p_size = 5 AND s_nationkey = n_nationkey
          AND ps_supplycost = (SELECT MIN(ps_supplycost) FROM q2_partsupp
                               WHERE p_partkey = ps_partkey)
        ORDER BY s_acctbal DESC, p_partkey LIMIT 10""").compute()
    mn = partsupp.groupby("ps_partkey")["ps_supplycost"].min()
    j = partsupp.merge(part[part.p_size == 5], left_on="ps_partkey",
                       right_on="p_partkey")
    j = j[np.isclose(j.ps_supplycost,
                     mn.reindex(j.ps_partkey).to_numpy())]
    j = j.merge(supplier, left_on="ps_suppkey", right_on="s_suppkey") \
         .merge(nation, left_on="s_nationkey", right_on="n_nationkey")
    exp = j.sort_values(["s_acctbal", "p_partkey"],
                        ascending=[False, True]).head(10)
    assert len(out) == len(exp)
    np.testing.assert_allclose(out["s_acctbal"].to_numpy(np.float64),
                               exp["s_acctbal"].to_numpy(), rtol=1e-9)


def test_q20_shape_nested_in_correlated(ctx):
    """Q20: IN subquery containing another IN and a correlated scalar
    expression-over-SUM subquery."""
    rng = np.random.default_rng(43)
    part = pd.DataFrame({"p_partkey": np.arange(40, dtype=np.int64),
                         "p_size": rng.integers(1, 20, 40).astype(np.int64)})
    partsupp = pd.DataFrame({
        "ps_partkey": rng.integers(0, 40, 200).astype(np.int64),
        "ps_suppkey": rng.integers(0, 15, 200).astype(np.int64),
        "ps_availqty": rng.integers(1, 100, 200).astype(np.int64)})
    lineitem = pd.DataFrame({
        "l_partkey": rng.integers(0, 40, 1000).astype(np.int64),
        "l_suppkey": rng.integers(0, 15, 1000).astype(np.int64),
        "l_quantity": rng.integers(1, 50, 1000).astype(np.int64)})
    supplier = pd.DataFrame({"s_suppkey": np.arange(15, dtype=np.int64)})
    ctx.create_table("q20_part", part)
    ctx.create_table("q20_partsupp", partsupp)
    ctx.create_table("q20_lineitem", lineitem)
    ctx.create_table("q20_supplier", supplier)
    out = ctx.sql("""
        SELECT s_suppkey FROM q20_supplier
        WHERE s_suppkey IN (
          SELECT ps_suppkey FROM q20_partsupp
          WHERE ps_partkey IN (SELECT p_partkey FROM q20_part
                               WHERE p_size < 10)
            AND ps_availqty > (SELECT 0.5 * SUM(l_quantity)
                               FROM q20_lineitem
                               WHERE l_partkey = ps_partkey
                                 AND l_suppkey = ps_suppkey)
        )""").compute()
    small = set(part[part.p_size < 10].p_partkey)
    half = lineitem.groupby(["l_partkey", "l_suppkey"])["l_quantity"] \
        .sum() * 0.5
    ps = partsupp[partsupp.ps_partkey.isin(small)]
    keep = []
    for r in ps.itertuples(index=False):
        h = half.get((r.ps_partkey, r.ps_suppkey))
        if h is not None and r.ps_availqty > h:
            keep.append(r.ps_suppkey)
    exp = sorted(set(keep))
    assert sorted(out["s_suppkey"].astype(np.int64).tolist()) == exp


def test_numeric_leading_column_name(ctx):
    # reference test_compatibility.py:1078 — quoted "1b" column
    df = pd.DataFrame({"a": np.arange(5, dtype=np.int64),
                       "1b": np.arange(5, dtype=np.int64)})
    ctx.create_table("zz_numcol", df)
    out = ctx.sql('SELECT "1b" AS x FROM zz_numcol').compute()
    assert out["x"].astype(np.int64).tolist() == [0, 1, 2, 3, 4]
    out = ctx.sql('SELECT (CASE WHEN "1b"=1 THEN 0 END) AS x '
                  "FROM zz_numcol").compute()
    vals = out["x"].tolist()
    assert vals[1] == 0 and sum(pd.isna(v) for v in vals) == 4


def test_timezone_roundtrip(ctx):
    # reference test_select.py:116 — tz-aware columns survive SELECT
    df = pd.DataFrame({
        "timezone": pd.date_range("2014-08-01 09:00", freq="8h",
                                  periods=6, tz="Europe/Berlin"),
        "no_timezone": pd.date_range("2014-08-01 09:00", freq="8h",
                                     periods=6),
        "utc_timezone": pd.date_range("2014-08-01 09:00", freq="8h",
                                      periods=6, tz="UTC")})
    ctx.create_table("zz_tz", df)
    out = ctx.sql("SELECT * FROM zz_tz").compute()
    assert (pd.to_datetime(out["timezone"]) == df["timezone"]).all()
    assert (pd.to_datetime(out["no_timezone"])
            == df["no_timezone"]).all()
    assert (pd.to_datetime(out["utc_timezone"])
            == df["utc_timezone"]).all()


def test_trim_variants_and_now(ctx):
    df = pd.DataFrame({"s": pd.Series(["  pad  ", "xxvxx"]
                                      ).astype("category"),
                       "v": np.arange(2, dtype=np.int64)})
    ctx.create_table("zz_trimv", df)
    out = ctx.sql("SELECT LTRIM(s) AS l, RTRIM(s) AS r, BTRIM(s) AS b, "
                  "BTRIM(s, 'x') AS bx, v FROM zz_trimv").compute()
    out = out.sort_values("v").reset_index(drop=True)
    assert out["l"].tolist() == ["pad  ", "xxvxx"]
    assert out["r"].tolist() == ["  pad", "xxvxx"]
    assert out["b"].tolist() == ["pad", "xxvxx"]
    assert out["bx"].tolist() == ["  pad  ", "v"]
    out = ctx.sql("SELECT CURRENT_TIMESTAMP AS n, v FROM zz_trimv"
                  ).compute()
    now = pd.Timestamp.now()
    got = pd.to_datetime(out["n"]).iloc[0]
    assert abs((now - got).total_seconds()) < 3600


def test_rand_exec(ctx):
    df = pd.DataFrame({"a": np.arange(100, dtype=np.int64)})
    ctx.create_table("zz_rand", df)
    out = ctx.sql("SELECT RAND(0) AS r, RAND_INTEGER(0, 10) AS ri, a "
                  "FROM zz_rand").compute()
    r = out["r"].astype(float)
    assert ((r >= 0) & (r < 1)).all() and r.nunique() > 50
    ri = out["ri"].astype(np.int64)
    assert ((ri >= 0) & (ri < 10)).all()


def test_last_day_and_datepart_exec(ctx):
    from pandas.tseries.offsets import MonthEnd
    ts = pd.to_datetime(["2021-01-15 10:30:00", "2021-01-31 23:59:59",
                         "2020-02-29 00:00:00"])
    df = pd.DataFrame({"t": ts, "v": np.arange(3, dtype=np.int64)})
    ctx.create_table("zz_ld", df)
    out = ctx.sql("SELECT LAST_DAY(t) AS ld, DATEPART('YEAR', t) AS y, "
                  "DATEPART('week', t) AS w, v FROM zz_ld").compute()
    out = out.sort_values("v").reset_index(drop=True)
    assert (pd.to_datetime(out["ld"]) == pd.Series(ts) + MonthEnd(1)).all()
    assert out["y"].astype(np.int64).tolist() == [2021, 2021, 2020]
    want_w = pd.Series(ts).dt.isocalendar().week.tolist()
    assert out["w"].astype(np.int64).tolist() == [int(x) for x in want_w]


def test_create_view_exec(ctx):
    df = pd.DataFrame({"a": np.arange(10, dtype=np.int64),
                       "b": np.arange(10, dtype=np.int64) % 3})
    ctx.create_table("zz_vt", df)
    ctx.sql("CREATE VIEW zz_vv AS SELECT a, b FROM zz_vt WHERE a >= 4")
    out = ctx.sql("SELECT b, COUNT(*) AS n FROM zz_vv GROUP BY b").compute()
    exp = df[df.a >= 4].groupby("b").size()
    got = dict(zip(out["b"].astype(np.int64), out["n"].astype(np.int64)))
    assert got == exp.to_dict()
    ctx.sql("DROP VIEW zz_vv")
