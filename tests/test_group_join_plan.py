"""Group-join eligibility (physical/group_join.py): a pure function of plan
facts, so it runs without a device. The join row is lhs columns then rhs
columns; Q3's last join is (orders ⋈ customer) as lhs with o_orderkey,
o_orderdate, o_shippriority, and lineitem as rhs with l_orderkey,
l_extendedprice, l_discount, l_shipdate, probing from the right."""
import ctypes as ct
from pathlib import Path

import pytest

from dask_sql_amd.physical import group_join as gj

I64, F64, I32 = "i64", "f64", "i32"

# join-row columns
O_KEY, O_DATE, O_PRIO, L_KEY, L_PRICE, L_DISC, L_SHIP = range(7)


def q3(**over):
    facts = dict(
        join_type="inner", residual=False, null_equal=False, probe_side="r",
        n_lhs_cols=3, lhs_on=[0], rhs_on=[0], key_dtypes=[(I64, I64)],
        group_cols=[L_KEY, O_DATE, O_PRIO],
        aggs=[gj.AggFact("sum", frozenset({L_PRICE, L_DISC}))],
        max_aggs=16, max_keys=4)
    facts.update(over)
    return gj.verdict(**facts)


def test_q3_shape_is_accepted():
    v = q3()
    assert v.ok and bool(v)
    # l_orderkey comes out as its build-side twin, the rest as they are
    assert v.key_sources == (("key", 0), ("build", O_DATE), ("build", O_PRIO))


def test_build_side_key_and_count_star_are_accepted():
    v = q3(group_cols=[O_KEY],
           aggs=[gj.AggFact("count", None), gj.AggFact("avg",
                                                       frozenset({L_PRICE}))])
    assert v.ok
    assert v.key_sources == (("build", O_KEY),)


def test_probe_on_the_left():
    # lineitem as lhs (4 columns), orders side as rhs
    v = q3(probe_side="l", n_lhs_cols=4, lhs_on=[0], rhs_on=[0],
           group_cols=[0, 5], aggs=[gj.AggFact("sum", frozenset({1, 2}))])
    assert v.ok
    assert v.key_sources == (("key", 0), ("build", 5))


@pytest.mark.parametrize("over, word", [
    (dict(group_cols=[O_DATE, O_PRIO]), "miss a join key"),
    (dict(group_cols=[L_KEY, None]), "not a column"),
    (dict(group_cols=[L_KEY, L_SHIP]), "probe side"),
    (dict(aggs=[gj.AggFact("sum", frozenset({L_PRICE, O_PRIO}))]),
     "build column"),
    (dict(join_type="left"), "left"),
    (dict(join_type="leftanti"), "leftanti"),
    (dict(residual=True), "residual"),
    (dict(null_equal=True), "null-equal"),
    (dict(aggs=[gj.AggFact("sum", frozenset({L_PRICE}), distinct=True)]),
     "DISTINCT"),
    (dict(aggs=[gj.AggFact("sum", frozenset({L_PRICE}), filtered=True)]),
     "FILTER"),
    (dict(aggs=[gj.AggFact("stddev", frozenset({L_PRICE}))]), "stddev"),
    (dict(aggs=[gj.AggFact("var_pop", frozenset({L_PRICE}))]), "var_pop"),
    (dict(probe_side=None), "no pending WHERE"),
    (dict(key_dtypes=[(I64, I32)]), "dtypes differ"),
    (dict(key_dtypes=[(("dict", "l"), ("dict", "r"))]), "dtypes differ"),
    (dict(lhs_on=[], rhs_on=[], key_dtypes=[]), "no equi keys"),
    (dict(aggs=[]), "no aggregate"),
    (dict(aggs=[gj.AggFact("count", None)] * 17), "too many aggregates"),
    (dict(group_cols=[L_KEY, O_KEY, O_DATE, O_PRIO, O_PRIO]), "group keys"),
])
def test_declines(over, word):
    v = q3(**over)
    assert not v.ok and not v
    assert word in v.reason
    assert v.key_sources == ()


def test_composite_key_needs_every_part():
    two = dict(lhs_on=[0, 1], rhs_on=[0, 3], key_dtypes=[(I64, I64),
                                                         (I32, I32)])
    assert q3(group_cols=[L_KEY, L_SHIP, O_PRIO], **two).ok
    assert q3(group_cols=[L_KEY, O_DATE], **two).ok  # one part per side
    assert "miss a join key" in q3(group_cols=[L_KEY, O_PRIO], **two).reason


def test_knobs_are_read_per_call(monkeypatch):
    monkeypatch.delenv("DSX_DISABLE_GROUPJOIN", raising=False)
    monkeypatch.delenv("DSX_GROUPJOIN_MIN_ROWS", raising=False)
    assert not gj.disabled()
    assert gj.min_rows() == 1_048_576
    monkeypatch.setenv("DSX_DISABLE_GROUPJOIN", "1")
    monkeypatch.setenv("DSX_GROUPJOIN_MIN_ROWS", "0")
    assert gj.disabled()
    assert gj.min_rows() == 0
    monkeypatch.setenv("DSX_DISABLE_GROUPJOIN", "0")
    monkeypatch.setenv("DSX_GROUPJOIN_MIN_ROWS", "many")
    assert not gj.disabled()
    assert gj.min_rows() == 1_048_576


def test_generated_accumulate_kernel_compiles():
    """hipRTC compiles j_fprobe_agg for Q3's shape and for a composite
    unpacked key with every op; needs the built library, no device."""
    so = Path(gj.__file__).resolve().parents[1] / "libdsxhip.so"
    if not so.exists():
        pytest.skip("libdsxhip.so not built")
    lib = ct.CDLL(str(so))
    lib.dsx_jit_fprobe_agg_selftest.restype = ct.c_int
    assert lib.dsx_jit_fprobe_agg_selftest() == 0
