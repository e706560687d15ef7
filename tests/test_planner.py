"""CPU tests: planner shapes + duck-typed plan API + Rex
compiler. No GPU needed."""
import numpy as np
import pandas as pd
import pytest

from dask_sql_amd.context import Context
from dask_sql_amd.planner.plan import Call, InputRef, Literal


@pytest.fixture
def c(user_table_1, user_table_2, df_simple):
    c = Context()
    c.create_table("user_table_1", user_table_1)
    c.create_table("user_table_2", user_table_2)
    c.create_table("df_simple", df_simple)
    return c


def test_scan_shape(c):
    rel = c._get_ral("SELECT * FROM user_table_1")
    assert rel.get_current_node_type() == "Projection"
    scan = rel.get_inputs()[0]
    assert scan.get_current_node_type() == "TableScan"
    assert scan.getRowType().getFieldNames() == ["user_id", "b"]
    assert scan.table_scan().getTableName() == "user_table_1"


def test_filter_shape(c):
    # conjuncts may be pushed down as stacked Filter nodes (PushDownFilter
    # analog); collect every condition on the chain
    rel = c._get_ral("SELECT * FROM user_table_1 WHERE b < 3 AND user_id = 2")
    node = rel.get_inputs()[0]
    ops = []
    while node.get_current_node_type() == "Filter":
        cond = node.filter().getCondition()
        assert str(cond.getRexType()) == "RexType.Call"
        ops.append(cond.getOperatorName())
        node = node.get_inputs()[0]
    assert node.get_current_node_type() == "TableScan"
    assert sorted(ops) == ["<", "="] or ops == ["AND"]


def test_join_shape_and_condition(c):
    rel = c._get_ral(
        "SELECT lhs.user_id, lhs.b, rhs.c FROM user_table_1 AS lhs "
        "JOIN user_table_2 AS rhs ON lhs.user_id = rhs.user_id"
    )
    join = rel.get_inputs()[0]
    assert join.get_current_node_type() == "Join"
    j = join.join()
    assert str(j.getJoinType()) == "INNER"
    cond = j.getCondition()
    assert cond.getOperatorName() == "="
    ops = cond.getOperands()
    assert [o.getIndex() for o in ops] == [0, 2]  # lhs idx 0, rhs idx 2


def test_aggregate_shape(c):
    rel = c._get_ral(
        "SELECT user_id, SUM(b) AS S FROM user_table_1 GROUP BY user_id"
    )
    agg = rel.get_inputs()[0]
    assert agg.get_current_node_type() == "Aggregate"
    a = agg.aggregate()
    groups = a.getGroupSets()
    assert len(groups) == 1 and isinstance(groups[0], InputRef)
    calls = a.getNamedAggCalls()
    assert len(calls) == 1
    assert a.getAggregationFuncName(calls[0]) == "sum"
    args = a.getArgs(calls[0])
    assert len(args) == 1 and isinstance(args[0], InputRef)
    assert calls[0].getFilterExpr() is None
    assert not calls[0].isDistinctAgg()


def test_aggregate_filter_clause(c):
    rel = c._get_ral(
        "SELECT SUM(b) FILTER (WHERE user_id = 2) AS S1, SUM(b) AS S2 "
        "FROM user_table_1"
    )
    agg = rel.get_inputs()[0]
    a = agg.aggregate()
    calls = a.getNamedAggCalls()
    assert len(calls) == 2
    filters = [cc.getFilterExpr() for cc in calls]
    assert sum(f is not None for f in filters) == 1


def test_fq_disambiguation(c):
    # context.py:890-898: duplicated output names become fully qualified
    rel = c._get_ral(
        "SELECT lhs.user_id, lhs.b, rhs.user_id, rhs.c FROM user_table_1 lhs "
        "JOIN user_table_2 rhs ON lhs.user_id = rhs.user_id"
    )
    assert rel.getRowType().getFieldNames() == \
        ["lhs.user_id", "b", "rhs.user_id", "c"]


def test_implicit_join_becomes_inner(c):
    rel = c._get_ral(
        "SELECT lhs.b FROM user_table_1 lhs, user_table_2 rhs "
        "WHERE lhs.user_id = rhs.user_id AND lhs.b > 1"
    )
    # find join node
    node = rel
    while node.get_current_node_type() != "Join":
        node = node.get_inputs()[0]
    assert node.join().getJoinType() == "INNER"
    assert node.join().getCondition() is not None


def test_filter_pushdown_below_join(c):
    rel = c._get_ral(
        "SELECT lhs.b FROM user_table_1 lhs, user_table_2 rhs "
        "WHERE lhs.user_id = rhs.user_id AND lhs.b > 1"
    )
    node = rel
    while node.get_current_node_type() != "Join":
        node = node.get_inputs()[0]
    lhs = node.get_inputs()[0]
    assert lhs.get_current_node_type() == "Filter"  # b > 1 pushed down


def test_order_limit_shape(c):
    rel = c._get_ral(
        "SELECT user_id, SUM(b) AS S FROM user_table_1 GROUP BY user_id "
        "ORDER BY S DESC LIMIT 2"
    )
    assert rel.get_current_node_type() == "Limit"
    srt = rel.get_inputs()[0]
    assert srt.get_current_node_type() == "Sort"
    keys = srt.sort().getCollation()
    assert keys[0][0] == 1 and keys[0][1] is False


def test_distinct_shape(c):
    rel = c._get_ral("SELECT DISTINCT user_id FROM user_table_1")
    assert rel.get_current_node_type() == "Distinct"
    assert rel.aggregate().isDistinctNode()


def test_plugin_replacement():
    # the drop-in boundary: add_plugin_class(cls, replace=True) swaps the
    # converter (reference physical/rel/convert.py:32-36, utils.py:61-91)
    from dask_sql_amd.physical.convert import RelConverter
    from dask_sql_amd.physical.rel_plugins import DaskFilterPlugin

    class MyFilter(DaskFilterPlugin):
        class_name = "Filter"

    orig = RelConverter._plugins["Filter"]
    try:
        RelConverter.add_plugin_class(MyFilter, replace=True)
        assert isinstance(RelConverter._plugins["Filter"], MyFilter)
        RelConverter.add_plugin_class(DaskFilterPlugin, replace=False)
        assert isinstance(RelConverter._plugins["Filter"], MyFilter)
    finally:
        RelConverter._plugins["Filter"] = orig


def test_case_when_parse(c):
    rel = c._get_ral(
        "SELECT CASE WHEN b > 2 THEN 1 ELSE 0 END AS x FROM user_table_1"
    )
    proj = rel.projection().getNamedProjects()
    assert proj[0][1] == "x"
    assert proj[0][0].getOperatorName() == "CASE"


def test_between_parse(c):
    # BETWEEN expands to >= AND <= (reference rex/core/call.py:963 semantics)
    rel = c._get_ral("SELECT * FROM user_table_1 WHERE b BETWEEN 1 AND 3")
    node = rel.get_inputs()[0]
    ops = []
    while node.get_current_node_type() == "Filter":
        ops.append(node.filter().getCondition().getOperatorName())
        node = node.get_inputs()[0]
    assert sorted(ops) in (["<=", ">="], ["AND"])


def test_date_literal(c):
    c.create_table("d", pd.DataFrame({"x": np.array([0, 10000], np.int32)}),
                   date_columns=["x"])
    rel = c._get_ral("SELECT * FROM d WHERE x < DATE '1995-03-15'")
    cond = rel.get_inputs()[0].filter().getCondition()
    lit = cond.getOperands()[1]
    assert str(lit.getRexType()) == "RexType.Literal"
    assert lit.getValue() == 9204  # days since epoch


def test_rex_compiler_programs(c, user_table_1):
    """Compile over fake CPU column stubs (no GPU needed)."""
    from dask_sql_amd.physical.rex import compile_expr
    from dask_sql_amd import runtime as rt

    class FakeCol:
        def __init__(self, dtype):
            self.dtype = dtype
            self.validity = None

    rel = c._get_ral("SELECT * FROM user_table_1 WHERE b < 3 OR user_id = 2")
    cond = rel.get_inputs()[0].filter().getCondition()
    cols = [FakeCol(rt.I64), FakeCol(rt.I64)]
    prog, kind = compile_expr(cond, cols)
    assert kind == "b"
    ops = [p[0] for p in prog]
    assert 41 in ops  # OR
    assert 30 in ops and 34 in ops  # int compares


def test_like_parses_and_types():
    from dask_sql_amd.planner.parser import Parser
    ast = Parser("SELECT a FROM t WHERE b LIKE 'x%' AND c NOT LIKE '_y'"
                 ).parse()
    s = repr(ast)
    assert "LIKE" in s


def test_like_regex_translation():
    from dask_sql_amd.physical.rex import _like_regex
    rx = _like_regex("AB%c_d.e")
    assert rx.fullmatch("ABzzzcXd.e")
    assert not rx.fullmatch("ABcXdYe")  # literal dot must match
    assert rx.fullmatch("AB%c_d.e".replace("%", "").replace("_", "Q"))


def test_create_table_from_files(tmp_path):
    """File-path create_table (reference context.py:168 +
    input_utils/location.py extension dispatch)."""
    import pandas as pd
    import numpy as np
    from dask_sql_amd.context import Context
    df = pd.DataFrame({"a": np.arange(5, dtype=np.int64),
                       "b": np.linspace(0, 1, 5)})
    pq = tmp_path / "t.parquet"
    cv = tmp_path / "t.csv"
    df.to_parquet(pq)
    df.to_csv(cv, index=False)
    c = Context()
    c.create_table("tp", str(pq))
    c.create_table("tc", str(cv))
    for t in ("tp", "tc"):
        fields = dict(c.tables[t].fields())
        assert fields["a"] == "BIGINT" and fields["b"] == "DOUBLE"
    import pytest
    with pytest.raises(NotImplementedError):
        c.create_table("tx", "no_such.xyz")


def test_union_parses_and_folds():
    from dask_sql_amd.planner.parser import Parser, UnionStmt
    u = Parser("SELECT a FROM t UNION ALL SELECT b FROM u "
               "UNION SELECT c FROM w ORDER BY a LIMIT 5").parse()
    assert isinstance(u, UnionStmt)
    assert u.alls == [True, False]
    assert u.limit == 5 and len(u.order_by) == 1
    assert u.branches[2].order_by == [] and u.branches[2].limit is None


def test_show_commands():
    """SHOW SCHEMAS/TABLES/COLUMNS — expected frames per reference
    tests/integration/test_show.py:9-62."""
    import pandas as pd
    from dask_sql_amd.context import Context
    c = Context()
    c.create_table("user_table_1", pd.DataFrame(
        {"user_id": [1], "b": [2]}))
    s = c.sql("SHOW SCHEMAS").compute()
    assert s["Schema"].tolist() == ["root", "information_schema"]
    t = c.sql('SHOW TABLES FROM "root"').compute()
    assert t["Table"].tolist() == ["user_table_1"]
    cols = c.sql('SHOW COLUMNS FROM "root"."user_table_1"').compute()
    assert cols["Column"].tolist() == ["user_id", "b"]
    assert cols["Type"].tolist() == ["bigint", "bigint"]
    import pytest
    with pytest.raises(KeyError):
        c.sql('SHOW COLUMNS FROM "root"."missing"')


PLAN_BATTERY = [
    # every supported construct must at least PLAN (conversion is gpu-only)
    "SELECT a, b FROM t WHERE a > 1 AND b < 2.5",
    "SELECT a + b * 2 - 1 AS x, a % 3 AS m FROM t",
    "SELECT COUNT(*), SUM(a), AVG(b), MIN(a), MAX(b) FROM t",
    "SELECT a, STDDEV(b), VAR_POP(b) FROM t GROUP BY a HAVING COUNT(*) > 2",
    "SELECT a, SUM(b) FILTER (WHERE a > 0) FROM t GROUP BY a",
    "SELECT COUNT(DISTINCT a) FROM t",
    "SELECT DISTINCT a, b FROM t",
    "SELECT t.a, u.d FROM t JOIN u ON t.a = u.c",
    "SELECT t.a FROM t LEFT JOIN u ON t.a = u.c AND u.d > 1",
    "SELECT t.a FROM t LEFT SEMI JOIN u ON t.a = u.c",
    "SELECT t.a FROM t LEFT ANTI JOIN u ON t.a = u.c",
    "SELECT * FROM t, u WHERE t.a = u.c",
    "SELECT a FROM t WHERE a IN (1, 2, 3) OR b BETWEEN 0 AND 1",
    "SELECT a FROM t WHERE a IN (SELECT c FROM u WHERE d > 0)",
    "SELECT a FROM t WHERE NOT EXISTS (SELECT 1 FROM u WHERE u.c = t.a)",
    "SELECT a FROM t WHERE b > (SELECT AVG(b) FROM t)",
    "SELECT x.a2 FROM (SELECT a AS a2 FROM t WHERE b > 0) x",
    "SELECT a FROM t UNION ALL SELECT c FROM u ORDER BY a LIMIT 3",
    "SELECT a, ROW_NUMBER() OVER (PARTITION BY a ORDER BY b DESC) FROM t",
    "SELECT SUM(b) OVER (PARTITION BY a) AS s FROM t",
    "SELECT LAG(b, 2, 0.0) OVER (PARTITION BY a ORDER BY b) FROM t",
    "SELECT FIRST_VALUE(b) OVER (PARTITION BY a ORDER BY b) FROM t",
    "SELECT CASE WHEN a > 1 THEN 'x' ELSE 'y' END FROM t",
    "SELECT CASE a WHEN 1 THEN 10 ELSE 0 END FROM t",
    "SELECT COALESCE(a, 0), NULLIF(a, 1) FROM t",
    "SELECT ABS(a), FLOOR(b), CEIL(b), ROUND(b, 2), EXP(b), LN(b + 1), "
    "POWER(b, 2), SQRT(ABS(b)), MOD(a, 2) FROM t",
    "SELECT CAST(b AS BIGINT), CAST(a AS DOUBLE) FROM t",
    "SELECT 1 + 1 AS two",
    "SELECT a FROM t ORDER BY a DESC NULLS LAST LIMIT 10 OFFSET 5",
    "SELECT a, SUM(b) AS s FROM t GROUP BY a ORDER BY SUM(b) DESC LIMIT 5",
    # round-2 constructs
    "SELECT a, (SELECT MAX(u.d) FROM u WHERE u.c = t.a) AS m FROM t",
    "SELECT * FROM t WHERE b < (SELECT AVG(u.d) FROM u WHERE u.c = t.a)",
    "SELECT a FROM t WHERE a NOT IN (SELECT c FROM u)",
    "SELECT a + 1 AS g, SUM(CASE WHEN b > 1 THEN 1 END) FROM t "
    "GROUP BY a + 1",
    "SELECT a FROM t ORDER BY a DESC, b",
    "SELECT RANK() OVER (PARTITION BY a ORDER BY b) AS r, "
    "DENSE_RANK() OVER (ORDER BY b) AS d FROM t",
    # round-2 late additions: CTEs, set ops, IS TRUE, comments, aliases
    "WITH big AS (SELECT a, b FROM t WHERE a > 1) "
    "SELECT a, COUNT(*) AS n FROM big GROUP BY a",
    "WITH x AS (SELECT a FROM t), y AS (SELECT c AS a FROM u) "
    "SELECT x.a FROM x JOIN y ON x.a = y.a",
    "SELECT a FROM t INTERSECT SELECT c FROM u",
    "SELECT a FROM t EXCEPT SELECT c FROM u",
    "SELECT a FROM t UNION SELECT c FROM u INTERSECT SELECT a FROM t",
    "SELECT a FROM t INTERSECT SELECT c FROM u ORDER BY a LIMIT 2",
    "SELECT a + 1 AS date FROM t WHERE a > 0",
    "SELECT a IS TRUE AS x, a IS NOT TRUE AS y, a IS FALSE AS z, "
    "a IS NOT UNKNOWN AS w FROM t",
    "SELECT a -- line comment\n FROM t /* block\n comment */ WHERE a > 0",
    "SELECT * FROM (SELECT a FROM t LIMIT 2) JOIN u ON a = c",
    "SELECT TIMESTAMPDIFF(DAY, a, b) FROM t",
    "SELECT t.* FROM t",
    "SELECT u.c, t.* FROM t JOIN u ON t.a = u.c",
    "SELECT a, REGR_COUNT(b, a) AS n, REGR_SXX(b, a) AS sxx, "
    "COVAR_POP(b, a) AS cp, COVAR_SAMP(b, a) AS cs FROM t GROUP BY a",
    "SELECT a, b, FROM t",
    "SELECT * FROM t DISTRIBUTE BY a",
    "SELECT a FROM t WHERE CAST(b AS DECIMAL) < DECIMAL '100.2'",
    "SELECT TIME '08:08:00.091' AS tm FROM t",
]


def test_plan_battery():
    import pandas as pd
    from dask_sql_amd.context import Context
    c = Context()
    c.create_table("t", pd.DataFrame({"a": [1, 2], "b": [0.5, 1.5]}))
    c.create_table("u", pd.DataFrame({"c": [1], "d": [2]}))
    for q in PLAN_BATTERY:
        c.explain(q)  # must not raise


def test_plan_battery_dates():
    import pandas as pd
    from dask_sql_amd.context import Context
    c = Context()
    c.create_table("t", pd.DataFrame(
        {"d": pd.to_datetime(["2020-01-01"]),
         "ts": pd.to_datetime(["2020-01-01 10:30:00"]),
         "s": pd.Series(["x"]).astype("category"), "v": [1.0]}))
    for q in [
        "SELECT v FROM t WHERE d >= DATE '2020-01-01' - INTERVAL '90' DAY",
        "SELECT v FROM t WHERE d < DATE '2020-01-01' + INTERVAL '2' MONTH",
        "SELECT EXTRACT(YEAR FROM d), YEAR(d), MONTH(d), DAY(d) FROM t",
        "SELECT EXTRACT(HOUR FROM ts), EXTRACT(MINUTE FROM ts) FROM t",
        "SELECT v FROM t WHERE ts > TIMESTAMP '2020-01-01 09:00:00'",
        "SELECT v FROM t WHERE ts > DATE '2020-01-01'",
        "SELECT UPPER(s), LOWER(s), SUBSTRING(s, 1, 1), s || '!' FROM t",
        "SELECT TRIM('x' FROM s), INITCAP(s), REPLACE(s, 'x', 'y'), "
        "CHAR_LENGTH(s) FROM t",
        "SELECT v FROM t WHERE s LIKE 'x%' AND UPPER(s) = 'X'",
        "SELECT v FROM t WHERE s ILIKE 'X%' OR s NOT ILIKE '%y'",
        "SELECT v FROM t WHERE s SIMILAR TO '(x|y)%'",
        "SELECT v FROM t WHERE s LIKE 'x!%%' ESCAPE '!'",
        "SELECT v FROM t WHERE d >= d - INTERVAL '90 days'",
        "SELECT TIMESTAMPADD(DAY, 5, ts) AS ts2 FROM t",
        "SELECT TIMESTAMPADD(HOUR, -3, ts) AS ts3 FROM t",
        "SELECT FLOOR(ts TO DAY), CEIL(ts TO HOUR), FLOOR(ts TO YEAR), "
        "FLOOR(d TO MONTH), CEIL(ts TO MONTH), CEIL(d TO YEAR) FROM t",
        "SELECT EXTRACT(DATE FROM ts) AS dt FROM t",
        "SELECT LAST_DAY(ts) AS ld, LAST_DAY(d) AS ldd FROM t",
        "SELECT EXTRACT(CENTURY FROM ts), EXTRACT(DOW FROM d), "
        "EXTRACT(DOY FROM ts), EXTRACT(QUARTER FROM d), "
        "EXTRACT(MILLISECOND FROM ts), EXTRACT(DECADE FROM ts) FROM t",
        "SELECT POSITION('x' IN s) AS p, POSITION('x' IN s FROM 2) FROM t",
        "SELECT OVERLAY(s PLACING 'XX' FROM 2 FOR 3) AS o FROM t",
        "SELECT ts + INTERVAL '1' HOUR, ts - INTERVAL '30' MINUTE FROM t",
        "SELECT to_timestamp(v) AS t1, "
        "to_timestamp('2021-03-02 10:00:00') AS t2, "
        "TIMESTAMPADD(DAY, 2, to_timestamp(v)) AS t3 FROM t",
    ]:
        c.explain(q)


def test_plan_errors_are_loud():
    import pandas as pd
    import pytest
    from dask_sql_amd.context import Context
    c = Context()
    c.create_table("t", pd.DataFrame({"a": [1], "b": [2]}))
    with pytest.raises(KeyError):
        c.explain("SELECT missing FROM t")
    with pytest.raises(KeyError):
        c.explain("SELECT a FROM missing_table")
    # ROW_NUMBER without ORDER BY is legal (input order, like the
    # reference); RANK still needs an ordering
    c.explain("SELECT ROW_NUMBER() OVER (PARTITION BY a) FROM t")
    with pytest.raises(ValueError):
        c.explain("SELECT RANK() OVER (PARTITION BY a) FROM t")
    with pytest.raises((ValueError, NotImplementedError)):
        c.explain("SELECT a FROM t WHERE a IN (SELECT a, b FROM t)")


def test_interval_folding_unit():
    """_date_interval folds literal date arithmetic exactly (day-int and ns
    forms; month-end clamping like pandas DateOffset)."""
    import numpy as np
    from dask_sql_amd.planner.builder import Builder, _date_to_days
    from dask_sql_amd.planner.plan import Literal, SqlType

    def date_lit(s):
        return Literal(_date_to_days(s), SqlType("DATE"))

    def iv(n, u):
        return Literal((n, u), SqlType("INTERVAL"))

    r = Builder._date_interval("-", [date_lit("1998-12-01"), iv(90, "DAY")])
    assert r.getValue() == _date_to_days("1998-09-02")
    r = Builder._date_interval("+", [date_lit("1996-01-31"), iv(1, "MONTH")])
    assert r.getValue() == _date_to_days("1996-02-29")  # leap clamp
    r = Builder._date_interval("+", [date_lit("1995-03-15"), iv(2, "WEEK")])
    assert r.getValue() == _date_to_days("1995-03-29")
    r = Builder._date_interval("-", [date_lit("2000-03-31"), iv(1, "YEAR")])
    assert r.getValue() == _date_to_days("1999-03-31")
    ns = int(np.datetime64("2020-01-01T06:00:00", "ns").astype("int64"))
    r = Builder._date_interval(
        "+", [Literal(ns, SqlType("TIMESTAMP")), iv(1, "DAY")])
    assert r.getValue() == ns + 86_400_000_000_000
    assert r.getType().getSqlType() == "TIMESTAMP"


def test_fold_string_literal_unit():
    from dask_sql_amd.physical.rex import fold_string_literal
    from dask_sql_amd.planner.plan import Call, Literal, SqlType

    def lit(v, t="VARCHAR"):
        return Literal(v, SqlType(t))

    assert fold_string_literal(
        Call("REPLACE", [lit("Another String"), lit("th"), lit("b")])
    ) == "Anober String"  # reference test_rex.py:660 "x"
    assert fold_string_literal(
        Call("UPPER", [Call("SUBSTRING",
                            [lit("abcdef"), lit(2, "BIGINT"),
                             lit(3, "BIGINT")])])) == "BCD"
    assert fold_string_literal(
        Call("CONCAT", [lit("a"), lit("b"), lit("c")])) == "abc"
    assert fold_string_literal(Call("+", [lit("a"), lit("b")])) is None


def _join_chain(rel):
    """Walk down from the root to the first Join; return (join, nodes_above)."""
    node = rel
    above = []
    while node.get_current_node_type() != "Join":
        above.append(node.get_current_node_type())
        node = node.get_inputs()[0]
    return node, above


def test_no_pushdown_below_null_supplying_side():
    # WHERE on the null-supplying side of an outer join
    # must NOT be pushed below the join (DataFusion PushDownFilter pushes
    # only to preserved sides). `SELECT ... LEFT JOIN r ... WHERE r.x = 5`
    # keeps the predicate as a post-join Filter.
    c = Context()
    c.create_table("l", pd.DataFrame({"k": [1, 2, 3]}))
    c.create_table("r", pd.DataFrame({"k": [1, 2], "x": [5, 6]}))

    rel = c._get_ral(
        "SELECT l.k FROM l LEFT JOIN r ON l.k = r.k WHERE r.x = 5")
    join, above = _join_chain(rel)
    assert "Filter" in above, "WHERE r.x=5 must stay above the LEFT join"
    rhs = join.get_inputs()[1]
    assert rhs.get_current_node_type() == "TableScan", \
        "no Filter below the null-supplying rhs of a LEFT join"

    # RIGHT join: lhs is null-supplying — WHERE l.* stays post-join,
    # WHERE r.* (preserved side) is pushed below.
    rel = c._get_ral(
        "SELECT r.k FROM l RIGHT JOIN r ON l.k = r.k WHERE l.k = 1 AND r.x = 5")
    join, above = _join_chain(rel)
    assert "Filter" in above
    assert join.get_inputs()[0].get_current_node_type() == "TableScan"
    assert join.get_inputs()[1].get_current_node_type() == "Filter"

    # INNER join still pushes both sides down (no post-join Filter).
    rel = c._get_ral(
        "SELECT l.k FROM l JOIN r ON l.k = r.k WHERE r.x = 5")
    join, above = _join_chain(rel)
    assert "Filter" not in above
    assert join.get_inputs()[1].get_current_node_type() == "Filter"


def test_q3_real_text_plans():
    """The REAL Q3 text ('BUILDING', DATE '1995-03-15') must plan against
    dictionary/DATE-typed tables (bench headline path)."""
    import sys
    from tests.conftest import REPO
    sys.path.insert(0, str(REPO))
    from datagen import Q3_SQL, gen_q3, register_q3_tables
    c = Context()
    cust, orders, li = gen_q3(sf_rows=(200, 1000, 4000))
    register_q3_tables(c, cust, orders, li)
    rel = c._get_ral(Q3_SQL)
    # Limit over Sort over Projection/Aggregate chain
    assert rel.get_current_node_type() == "Limit"
    node = rel.get_inputs()[0]
    assert node.get_current_node_type() == "Sort"
    # date literal folded to day-int compare, segment to dict-code compare
    txt = rel.explain()
    assert "Join" in txt and "Aggregate" in txt


def test_q1_real_text_plans():
    import sys
    from tests.conftest import REPO
    sys.path.insert(0, str(REPO))
    from datagen import Q1_SQL, gen_lineitem_q1, register_q1_table
    c = Context()
    register_q1_table(c, gen_lineitem_q1(n=1000, seed=3))
    rel = c._get_ral(Q1_SQL)
    assert rel is not None
    txt = rel.explain()
    assert "Aggregate" in txt


def test_from_arrow_ingest(tmp_path):
    """Direct parquet→columnar ingest: _from_arrow bypasses
    pandas; dtypes/validity/dictionary/date mapping checked host-side."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    from dask_sql_amd.context import _from_arrow
    import dask_sql_amd.runtime as rt

    n = 1000
    t = pa.table({
        "i": pa.array(list(range(n)), type=pa.int64()),
        "f": pa.array([float(x) / 7 for x in range(n)], type=pa.float64()),
        "ni": pa.array([None if x % 10 == 0 else x for x in range(n)],
                       type=pa.int64()),
        "s": pa.array(["BUILDING", "AUTO", "FURN"][x % 3] for x in range(n)),
        "d": pa.array([x % 3000 for x in range(n)], type=pa.date32()),
        "b": pa.array([x % 2 == 0 for x in range(n)]),
    })
    f = tmp_path / "t.parquet"
    pq.write_table(t, f)
    cols = _from_arrow(pq.read_table(f))
    assert cols["i"].dtype == rt.I64 and cols["i"].validity is None
    assert cols["f"].dtype == rt.F64
    assert cols["ni"].validity is not None
    assert cols["ni"].validity.sum() == n - 100
    assert cols["s"].dictionary is not None and cols["s"].sql_type == "VARCHAR"
    import numpy as np
    dec = [cols["s"].dictionary[c] for c in cols["s"].arr[:6]]
    assert dec == ["BUILDING", "AUTO", "FURN", "BUILDING", "AUTO", "FURN"]
    assert cols["d"].sql_type == "DATE" and cols["d"].arr.dtype == np.int32
    assert cols["b"].dtype == rt.BOOL8
    assert cols["i"].arr[-1] == n - 1
    assert abs(cols["f"].arr[7] - 1.0) < 1e-12


def test_udf_agg_plan_rewrite():
    """Registered aggregate UDFs parse as plain calls but must plan as
    Aggregate nodes (builder._rewrite_udf_aggs; reference
    register_aggregation routes through the Aggregate rel)."""
    c = Context()
    c.create_table("t", pd.DataFrame({"k": [1, 2], "b": [1.0, 2.0]}))

    class A:
        def __init__(self):
            self.chunk = lambda s: s.sum()
            self.agg = lambda s: s.sum()

    c.register_aggregation(A(), "fagg", [("x", np.float64)], np.float64)
    rel = c._get_ral("SELECT k, FAGG(b) AS f FROM t GROUP BY k")
    node = rel
    while node.get_current_node_type() != "Aggregate":
        node = node.get_inputs()[0]
    agg = node.aggregate()
    names = [agg.getAggregationFuncName(call)
             for call in agg.getNamedAggCalls()]
    assert "udf:fagg" in names


def test_udf_scalar_plan_typing():
    c = Context()
    c.create_table("t", pd.DataFrame({"a": [1.0, 2.0]}))

    def f(x):
        return x ** 2

    c.register_function(f, "f", [("x", np.float64)], np.float64)
    rel = c._get_ral("SELECT F(a) AS y FROM t")
    proj = rel.projection().getNamedProjects()
    expr, name = proj[0]
    assert name == "y"
    assert expr.getOperatorName() == "UDF:f"
    assert expr.getType().getSqlType() == "DOUBLE"
    # plan cache keyed on schema version: registering bumps it
    v0 = c._schema_version
    c.register_function(f, "g", [("x", np.float64)], np.float64)
    assert c._schema_version > v0


def test_correlated_scalar_subquery_plan():
    """Equality-correlated scalar subqueries decorrelate into a grouped
    subplan LEFT-joined on the correlation keys (DataFusion's rewrite;
    round-1 raised on these)."""
    c = Context()
    c.create_table("t", pd.DataFrame({"k": [1, 2], "x": [1.0, 2.0]}))
    c.create_table("u", pd.DataFrame({"k": [1, 1, 2], "y": [5.0, 7.0, 9.0]}))
    rel = c._get_ral(
        "SELECT t.k, t.x, (SELECT MAX(u.y) FROM u WHERE u.k = t.k) AS m "
        "FROM t")
    txt = rel.explain()
    assert "Join" in txt and "Aggregate" in txt
    # the output row type keeps exactly the user columns
    assert rel.getRowType().getFieldNames() == ["k", "x", "m"]
    # star expansion must NOT leak the internal __ssub columns
    rel2 = c._get_ral(
        "SELECT * FROM t WHERE t.x < (SELECT AVG(u.y) FROM u "
        "WHERE u.k = t.k)")
    assert rel2.getRowType().getFieldNames() == ["k", "x"]


def test_from_arrow_multichunk(tmp_path):
    """_from_arrow with multi-chunk columns (row-group-split parquet) and
    large_string dictionary encoding."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    import dask_sql_amd.runtime as rt
    from dask_sql_amd.context import _from_arrow

    n = 5000
    t = pa.table({
        "i": pa.array(range(n), type=pa.int64()),
        "s": pa.array((["A", "B"][x % 2] for x in range(n)),
                      type=pa.large_string()),
    })
    f = tmp_path / "m.parquet"
    pq.write_table(t, f, row_group_size=700)  # 8 row groups → chunks
    rd = pq.read_table(f)
    assert rd.column("i").num_chunks > 1
    cols = _from_arrow(rd)
    assert cols["i"].arr[-1] == n - 1 and cols["i"].dtype == rt.I64
    assert cols["s"].dictionary is not None
    dec = [cols["s"].dictionary[c] for c in cols["s"].arr[:4]]
    assert dec == ["A", "B", "A", "B"]


def test_order_by_hidden_column_plan():
    """ORDER BY on a column not in the SELECT list: hidden sort column
    appended, sorted, then stripped (DataFusion plans Sort below the final
    projection)."""
    c = Context()
    c.create_table("t", pd.DataFrame({"a": [1, 2], "b": [0.5, 1.5]}))
    rel = c._get_ral("SELECT a FROM t ORDER BY b DESC")
    assert rel.getRowType().getFieldNames() == ["a"]
    assert rel.get_current_node_type() == "Projection"
    srt = rel.get_inputs()[0]
    assert srt.get_current_node_type() == "Sort"
    assert srt.getRowType().getFieldNames() == ["a", "__sort_h0"]
    (idx, asc, _nf), = srt.sort().getCollation()
    assert idx == 1 and asc is False
    # with LIMIT the fusion shape Sort→Limit is preserved under the strip
    rel2 = c._get_ral("SELECT a FROM t ORDER BY b LIMIT 1")
    assert rel2.get_current_node_type() == "Projection"
    assert rel2.get_inputs()[0].get_current_node_type() == "Limit"


def test_parser_truncation_errors_are_clean():
    """Every truncated prefix of every battery query must fail with a
    clean ValueError-family error, never IndexError/AttributeError (the
    reference surfaces ParsingException the same way)."""
    from dask_sql_amd.planner.parser import Parser
    for q in PLAN_BATTERY:
        for cut in range(len(q)):
            try:
                Parser(q[:cut]).parse()
            except (ValueError, NotImplementedError, KeyError):
                pass


def test_window_frame_apply_cpu():
    """_frame_apply is pure pandas — verify the ROWS-frame computation
    against hand-rolled windows (reference map_on_each_group semantics)."""
    import types

    import numpy as np
    import pandas as pd

    from dask_sql_amd.physical.rel_plugins import DaskWindowPlugin

    plug = DaskWindowPlugin.__new__(DaskWindowPlugin)
    df = pd.DataFrame({"p0": [0, 0, 0, 0, 1, 1, 1],
                       "v": [1.0, 2.0, 3.0, 4.0, 10.0, 20.0, 30.0]})
    grp = df.groupby(["p0"], dropna=False, sort=False)

    def run(func, frame):
        spec = types.SimpleNamespace(func=func, frame=frame, arg_idx=0)
        return plug._frame_apply(df.copy(), grp, ["p0"], spec).tolist()

    # 2 PRECEDING..CURRENT sums
    got = run("sum", ("rows", ("preceding", 2), ("current", 0)))
    assert got == [1, 3, 6, 9, 10, 30, 60]
    # 1 PRECEDING..1 FOLLOWING
    got = run("sum", ("rows", ("preceding", 1), ("following", 1)))
    assert got == [3, 6, 9, 7, 30, 60, 50]
    # UNBOUNDED..CURRENT max
    got = run("max", ("rows", ("unbounded_preceding", None),
                      ("current", 0)))
    assert got == [1, 2, 3, 4, 10, 20, 30]
    # CURRENT..UNBOUNDED FOLLOWING first_value = current
    got = run("first_value", ("rows", ("current", 0),
                              ("unbounded_following", None)))
    assert got == [1, 2, 3, 4, 10, 20, 30]
    # UNBOUNDED..UNBOUNDED last_value = partition tail
    got = run("last_value", ("rows", ("unbounded_preceding", None),
                             ("unbounded_following", None)))
    assert got == [4, 4, 4, 4, 30, 30, 30]
    # counts over 1 PRECEDING..CURRENT
    got = run("count", ("rows", ("preceding", 1), ("current", 0)))
    assert got == [1, 2, 2, 2, 1, 2, 2]


def test_sqlite_corpus_plans_cpu():
    """Every query of the sqlite-differential corpus must PLAN on CPU
    (execution runs on the GPU tier, tests/test_zz_sqlite_compat.py)."""
    import pandas as pd

    import tests.test_zz_sqlite_compat as m
    from dask_sql_amd.context import Context

    c = Context()
    m.PLAN_ONLY = True
    try:
        for name in dir(m):
            if name.startswith("test_sqlc_"):
                getattr(m, name)(c)
    finally:
        m.PLAN_ONLY = False


def test_ingest_materialize_roundtrip_cpu():
    """_from_pandas → materialize._convert is the identity for every
    supported input dtype (CPU halves of the device round trip: the arrays
    _convert sees are exactly what upload/download would carry)."""
    import types

    import numpy as np
    import pandas as pd

    from dask_sql_amd.context import _from_pandas
    from dask_sql_amd.materialize import _convert

    df = pd.DataFrame({
        "i64": np.array([1, -2, 3], dtype=np.int64),
        "i16": np.array([1, 2, 3], dtype=np.int16),
        "u8": np.array([0, 255, 7], dtype=np.uint8),
        "f64": [1.5, np.nan, -2.25],
        "f32": np.array([1.5, 2.5, 3.5], dtype=np.float32),
        "b": [True, False, True],
        "bn": pd.array([True, None, False], dtype="boolean"),
        "in64": pd.array([5, None, -7], dtype="Int64"),
        "s": ["x", None, "y"],
        "cat": pd.Series(["a", "b", "a"]).astype("category"),
        "sd": pd.array(["p", None, "q"], dtype="string"),
        "d": pd.to_datetime(["2021-01-01", "1969-12-31", "2100-06-01"]),
        "ts": pd.to_datetime(["2021-01-01 10:11:12", "1969-12-31 23:00:00",
                              "2100-06-01 00:00:01"]),
        "tz": pd.date_range("2014-08-01 09:00", periods=3, freq="8h",
                            tz="Europe/Berlin"),
    })
    cols = _from_pandas(df)
    for name, h in cols.items():
        stub = types.SimpleNamespace(dictionary=h.dictionary,
                                     tz=getattr(h, "tz", None))
        valid = h.validity.astype(bool) if h.validity is not None else None
        out = _convert(np.asarray(h.arr), valid, stub, h.sql_type)
        orig = df[name]
        if name == "tz":
            assert (pd.to_datetime(out) == orig).all(), name
            continue
        if str(orig.dtype).startswith("datetime"):
            assert (pd.to_datetime(out) == orig).all(), name
            continue
        o = pd.Series(out).reset_index(drop=True)
        e = orig.reset_index(drop=True)
        for a, b in zip(o, e):
            if pd.isna(b):
                assert pd.isna(a), (name, a, b)
            elif isinstance(b, str):
                assert str(a) == b, (name, a, b)
            else:
                assert float(a) == float(b), (name, a, b)


def test_plan_audit_gpu_suites_cpu():
    """The GPU suites' registrations + first queries must PLAN on CPU
    (scripts/plan_audit_gpu_tests.py in a subprocess — it patches
    Context.sql class-wide). The small allowed-failure budget covers the
    tests that construct a live runtime before their first query."""
    import re
    import subprocess
    import sys
    from pathlib import Path

    repo = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, "scripts/plan_audit_gpu_tests.py"],
                       capture_output=True, text=True, timeout=600,
                       cwd=str(repo))
    m = re.search(r"TOTAL planned-ok (\d+), not-auditable (\d+), "
                  r"FAILED (\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) >= 180, r.stdout[-2000:]
    assert int(m.group(3)) <= 9, r.stdout[-2000:]


def test_reference_string_op_unit_vectors():
    """reference tests/unit/test_call.py:178-199 string-op expectations,
    evaluated through the dictionary-function compilers the engine uses."""
    from dask_sql_amd.physical.rex import dict_int_fn, dict_string_fn
    from dask_sql_amd.planner.plan import Call, InputRef, Literal, SqlType

    a = "a normal string"
    dicts = [[a]]

    def sfn(op, *lits):
        e = Call(op, [InputRef(0, SqlType("VARCHAR"))]
                 + [Literal(v, SqlType("VARCHAR" if isinstance(v, str)
                                       else "BIGINT")) for v in lits],
                 SqlType("VARCHAR"))
        i, f = dict_string_fn(e, dicts)
        return f(a)

    def ifn(op, *lits):
        e = Call(op, [InputRef(0, SqlType("VARCHAR"))]
                 + [Literal(v, SqlType("VARCHAR" if isinstance(v, str)
                                       else "BIGINT")) for v in lits],
                 SqlType("BIGINT"))
        i, f = dict_int_fn(e, dicts)
        return f(a)

    assert ifn("CHAR_LENGTH") == 15
    assert sfn("UPPER") == "A NORMAL STRING"
    assert sfn("LOWER") == "a normal string"
    # POSITION(needle IN hay FROM start) — operand order (hay, needle[, n])
    assert ifn("POSITION", "a", 4) == 7
    assert ifn("POSITION", "ZL") == 0
    assert sfn("TRIM", "BOTH", "a") == " normal string"
    assert sfn("TRIM", "LEADING", "a") == " normal string"
    assert sfn("TRIM", "TRAILING", "a") == "a normal string"
    assert sfn("OVERLAY", "XXX", 2) == "aXXXrmal string"
    assert sfn("OVERLAY", "XXX", 2, 4) == "aXXXmal string"
    assert sfn("OVERLAY", "XXX", 2, 1) == "aXXXnormal string"
    assert sfn("SUBSTRING", -1) == "a normal string"
    assert sfn("SUBSTRING", 10) == "string"
    assert sfn("SUBSTRING", 2) == " normal string"
    assert sfn("SUBSTRING", 2, 2) == " n"
    assert sfn("INITCAP") == "A Normal String"
    assert sfn("REPLACE", "nor", "") == "a mal string"
    assert sfn("REPLACE", "normal", "new") == "a new string"


def test_alter_table_rename():
    """reference tests/unit/test_context.py:301 — ALTER TABLE RENAME."""
    import pandas as pd
    import pytest

    from dask_sql_amd.context import Context
    c = Context()
    c.create_table("maths", pd.DataFrame({"a": [1]}))
    c.sql("ALTER TABLE maths RENAME TO physics")
    assert "physics" in c.tables and "maths" not in c.tables
    c.explain("SELECT a FROM physics")
    with pytest.raises(KeyError):
        c.sql("ALTER TABLE four_legs RENAME TO two_legs")
    c.sql("ALTER TABLE IF EXISTS alien RENAME TO humans")


def test_create_view():
    """CREATE VIEW re-plans its SELECT per use (reference CreateView,
    persist=False); DROP VIEW unregisters."""
    import pandas as pd
    import pytest

    from dask_sql_amd.context import Context
    c = Context()
    c.create_table("t", pd.DataFrame({"a": [1, 2, 3], "b": [1.0, 2.0, 3.0]}))
    c.sql("CREATE VIEW big AS SELECT a, b FROM t WHERE a > 1")
    c.explain("SELECT a, COUNT(*) AS n FROM big GROUP BY a")
    c.explain("SELECT x.a FROM big x JOIN big y ON x.a = y.a")
    c.sql("CREATE OR REPLACE VIEW big AS SELECT a FROM t")
    c.explain("SELECT a FROM big")
    c.sql("DROP VIEW big")
    with pytest.raises(KeyError):
        c.explain("SELECT a FROM big")


def test_create_table_with_location():
    """reference test_create.py:14-40 — CREATE TABLE ... WITH (location,
    format) registers from a file path (parquet via arrow, csv via
    pandas)."""
    import os
    import tempfile

    import pandas as pd

    from dask_sql_amd.context import Context
    df = pd.DataFrame({"a": [1, 2], "b": [0.5, 1.5]})
    d = tempfile.mkdtemp()
    pqf = os.path.join(d, "x.parquet")
    csvf = os.path.join(d, "y.csv")
    df.to_parquet(pqf)
    df.to_csv(csvf, index=False)
    c = Context()
    c.sql(f"CREATE TABLE tp WITH (location = '{pqf}', "
          f"format = 'parquet')")
    c.sql(f"CREATE TABLE tc WITH (location = '{csvf}', format = 'csv', "
          f"gpu = False)")
    c.explain("SELECT a, b FROM tp")
    c.explain("SELECT a FROM tc")


def test_explain_statement_and_inline_dataframes():
    """reference test_explain.py:13-23 — EXPLAIN returns the plan string;
    sql(dataframes=...) registers frames inline."""
    import pandas as pd

    from dask_sql_amd.context import Context
    c = Context()
    c.create_table("df", pd.DataFrame({"a": [1, 2, 3]}))
    s = c.sql("EXPLAIN SELECT * FROM df")
    assert isinstance(s, str) and "Projection" in s
    s2 = c.sql("EXPLAIN SELECT MIN(a) AS a_min FROM other_df GROUP BY a",
               dataframes={"other_df": pd.DataFrame({"a": [1]})})
    assert isinstance(s2, str) and "a_min" in s2 or "MIN" in s2


def test_show_like_filtering():
    """reference test_show.py — SHOW ... LIKE filters the first column."""
    import pandas as pd

    from dask_sql_amd.context import Context
    c = Context()
    c.create_table("table", pd.DataFrame({"x": [1]}))
    out = c.sql("SHOW SCHEMAS LIKE 'information_schema'").compute()
    assert out["Schema"].tolist() == ["information_schema"]
    out = c.sql('SHOW TABLES FROM "root"').compute()
    assert out["Table"].tolist() == ["table"]
    out = c.sql("SHOW TABLES LIKE 'no_such%'").compute()
    assert out["Table"].tolist() == []


def test_hidden_host_builtins_cpu():
    """The hidden UDF builtins (month arithmetic, isoweek, rand) are pure
    pandas — pin them directly."""
    import numpy as np
    import pandas as pd

    from dask_sql_amd.planner.builder import (_add_months_host,
                                              _isoweek_host, _rand_host)

    ts = pd.to_datetime(["2021-01-31 10:00:00", "2020-02-29 23:00:00"])
    vals = pd.Series(ts.view("int64"))
    out = _add_months_host(False)(vals, pd.Series([1]))
    want = pd.Series(ts) + pd.DateOffset(months=1)
    assert (pd.to_datetime(out.astype("int64")) == want).all()

    days = pd.Series(((pd.Series(ts).dt.normalize()
                       - pd.Timestamp(0)).dt.days).astype("int64"))
    out = _add_months_host(True)(days, pd.Series([2]))
    want_d = (pd.Series(ts).dt.normalize() + pd.DateOffset(months=2)
              - pd.Timestamp(0)).dt.days
    assert out.astype("int64").tolist() == want_d.tolist()

    wk = _isoweek_host(False)(vals)
    want_w = pd.Series(ts).dt.isocalendar().week
    assert wk.astype("int64").tolist() == [int(x) for x in want_w]

    r = _rand_host(False)(pd.Series([0, 0, 0]))
    assert len(r) == 3 and ((r >= 0) & (r < 1)).all()
    ri = _rand_host(True)(pd.Series([10] * 5), pd.Series([0] * 5))
    assert len(ri) == 5 and ((ri >= 0) & (ri < 10)).all()
