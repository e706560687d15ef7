"""physical/join_plan.py: the join's one routing decision as a pure function
of plan facts — no device, no library. The rows follow tests/join_trace.py's
case list wherever the routing differs."""
import inspect

import pytest

from dask_sql_amd import runtime as rt
from dask_sql_amd.physical import filter_build as fb
from dask_sql_amd.physical import join_plan as jp

INT, FLT = rt.I64, rt.F64
K = jp.Knobs(disable_radix=False, radix_min_build=8_000_000,
             radix_min_probe=4_000_000, disable_joinfuse=False,
             disable_filterprobe=False, disable_filterbuild=False,
             filterbuild_max_rows=fb.DEFAULT_MAX_ROWS, filterbuild_min_rows=0)
RADIX = K._replace(radix_min_build=50, radix_min_probe=50)


def side(rows, pend=False, mat=None, n_cols=None, deferred=None):
    """n_cols: program + key columns while pending (two by default: one
    predicate column and the key)"""
    return jp.Side(rows, pend if deferred is None else deferred, pend, mat,
                   (2 if pend else 0) if n_cols is None else n_cols)


def facts(jt="inner", l=side(300), r=side(200), keys=((INT, INT, False),),
          **kw):
    return jp.JoinFacts(jt, tuple(keys), l, r,
                        n_mat=kw.pop("n_mat", 10), **kw)


P = dict(pend=True)
# (name, facts, knobs, expected fields of the route)
TABLE = [
    ("inner_l_larger", facts(l=side(400), r=side(100)), K,
     dict(path="fused", swap=False, ktype=rt.JOIN_INNER,
          build_from_cols=True, materialize=())),
    ("inner_l_smaller", facts(l=side(100), r=side(400)), K,
     dict(path="fused", swap=True, ktype=rt.JOIN_INNER)),
    ("left", facts("left"), K, dict(path="fused", swap=False,
                                    ktype=rt.JOIN_LEFT)),
    ("right", facts("right"), K, dict(path="fused", swap=True,
                                      ktype=rt.JOIN_LEFT)),
    ("leftanti", facts("leftanti"), K,
     dict(path="fused", swap=False, ktype=rt.JOIN_LEFTANTI)),
    ("below_min_rows", facts(), K._replace(filterbuild_min_rows=4096),
     dict(path="fused", build_from_cols=False)),
    ("pend_probe_r", facts(l=side(100), r=side(400, **P)), K,
     dict(path="fused", fprobe="r", fbuild=None, swap=True,
          build_from_cols=True, materialize=())),
    ("pend_probe_l", facts(l=side(400, **P), r=side(100)), K,
     dict(path="fused", fprobe="l", swap=False)),
    ("pend_build_stays", facts(l=side(100, **P), r=side(400)), K,
     dict(path="fused", fprobe=None, fbuild="l", swap=True,
          build_from_cols=True, materialize=())),
    ("pend_build_below_min", facts(l=side(100, **P), r=side(400)),
     K._replace(filterbuild_min_rows=4096),
     dict(path=None, fbuild=None, materialize=("l",))),
    ("pend_build_below_min_ran",
     facts(l=side(100, mat=3, **P), r=side(400)),
     K._replace(filterbuild_min_rows=4096),
     dict(path="fused", fbuild=None, swap=True, build_from_cols=False,
          materialize=("l",))),
    ("pend_build_above_max", facts(l=side(100, **P), r=side(400)),
     K._replace(filterbuild_max_rows=50),
     dict(path=None, fbuild=None, materialize=("l",))),
    ("pend_both", facts(l=side(100, **P), r=side(400, **P)), K,
     dict(path="fused", fprobe="r", fbuild="l", swap=True,
          build_from_cols=True, materialize=())),
    ("pend_build_left", facts("left", r=side(200, **P)), K,
     dict(path=None, fbuild=None, materialize=("r",))),
    ("pend_build_left_ran", facts("left", r=side(200, mat=3, **P)), K,
     dict(path="fused", build_from_cols=False, ktype=rt.JOIN_LEFT)),
    ("pend_build_right", facts("right", l=side(300, **P)), K,
     dict(path=None, materialize=("l",))),
    ("pend_build_anti", facts("leftanti", r=side(200, **P)), K,
     dict(path=None, materialize=("r",))),
    ("dict_other_on_build",
     facts(l=side(400), r=side(100), keys=((rt.I32, rt.I32, True),)), K,
     dict(path="fused", swap=False, build_from_cols=False)),
    ("dict_other_on_probe",
     facts(l=side(100), r=side(400), keys=((rt.I32, rt.I32, True),)), K,
     dict(path="fused", swap=True, build_from_cols=True)),
    ("dict_other_pend_build",
     facts(l=side(400), r=side(100, **P), keys=((rt.I32, rt.I32, True),)), K,
     dict(path=None, fbuild=None, materialize=("r",))),
    ("float_key", facts(keys=((FLT, FLT, False),)), K, dict(path="pairs")),
    ("float_key_pending",
     facts(l=side(100, **P), r=side(400, **P), keys=((FLT, FLT, False),)), K,
     dict(path=None, fprobe=None, fbuild=None, materialize=("l", "r"))),
    ("mixed_int_float", facts(keys=((INT, FLT, False),)), K,
     dict(path="pairs")),
    ("wide_output_17", facts(n_mat=17), K, dict(path="pairs")),
    ("wide_probe_17", facts(l=side(100), r=side(400, n_cols=17, **P)), K,
     dict(path=None, fprobe=None, fbuild=None, materialize=("r",))),
    # the wide side, a plain table now, is the smaller one and builds
    ("wide_probe_17_ran",
     facts(l=side(100), r=side(400, n_cols=17, mat=3, **P)), K,
     dict(path="fused", fprobe=None, swap=False, build_from_cols=True)),
    # the build side stays pending whatever the probe side shrinks to
    ("wide_probe_17_pend_build",
     facts(l=side(100, **P), r=side(400, n_cols=17, **P)), K,
     dict(path=None, fprobe=None, fbuild="l", swap=True,
          materialize=("r",))),
    ("wide_probe_17_pend_build_ran",
     facts(l=side(100, **P), r=side(400, n_cols=17, mat=3, **P)), K,
     dict(path="fused", fprobe=None, fbuild="l", swap=True,
          build_from_cols=True, materialize=("r",))),
    # the one outcome that differs from before: the row minimum is asked of
    # the side that builds (100 base rows), where the old late check looked
    # at the filtered probe side's 3 rows, ran the build side's WHERE and
    # packed its keys
    ("wide_probe_17_pend_build_row_minimum",
     facts(l=side(100, n_cols=17, mat=3, **P), r=side(100, **P)),
     K._replace(filterbuild_min_rows=80),
     dict(path="fused", fprobe=None, fbuild="r", swap=False,
          build_from_cols=True, materialize=("l",))),
    ("wide_build_17", facts(l=side(400), r=side(100, n_cols=17, **P)), K,
     dict(path=None, fbuild=None, materialize=("r",))),
    ("radix", facts(l=side(100), r=side(400)), RADIX,
     dict(path="radix", swap=True, fallback="fused")),
    ("radix_pending", facts(l=side(100, **P), r=side(400, **P)), RADIX,
     dict(path=None, fprobe=None, fbuild=None, materialize=("l", "r"))),
    ("radix_pending_ran",
     facts(l=side(100, mat=3, **P), r=side(400, mat=3, **P)), RADIX,
     dict(path="fused", swap=False, build_from_cols=False)),
    ("radix_pending_ran_large",
     facts(l=side(100, mat=60, **P), r=side(400, mat=70, **P)), RADIX,
     dict(path="radix", swap=True)),
    ("radix_probe_too_small", facts(l=side(100), r=side(400)),
     RADIX._replace(radix_min_probe=500), dict(path="fused")),
    ("radix_float_key", facts(keys=((FLT, FLT, False),)), RADIX,
     dict(path="pairs")),
    ("no_radix", facts(), RADIX._replace(disable_radix=True),
     dict(path="fused")),
    ("no_radix_pending", facts(l=side(100, **P), r=side(400, **P)),
     RADIX._replace(disable_radix=True),
     dict(path="fused", fprobe="r", fbuild="l")),
    ("no_joinfuse", facts(l=side(300, **P)), K._replace(disable_joinfuse=True),
     dict(path=None, fprobe=None, fbuild=None, materialize=("l",))),
    ("no_joinfuse_ran", facts(l=side(300, mat=3, **P)),
     K._replace(disable_joinfuse=True), dict(path="pairs")),
    ("no_joinfuse_radix", facts(), RADIX._replace(disable_joinfuse=True),
     dict(path="radix", fallback="pairs")),
    ("no_filterprobe", facts(l=side(100, **P), r=side(400, **P)),
     K._replace(disable_filterprobe=True),
     dict(path=None, fprobe=None, fbuild="l", materialize=("r",))),
    ("no_filterbuild", facts(l=side(100, **P), r=side(400, **P)),
     K._replace(disable_filterbuild=True),
     dict(path=None, fprobe="r", fbuild=None, materialize=("l",))),
    ("residual_inner", facts(residual=True), K, dict(path="pairs")),
    ("residual_anti", facts("leftanti", residual=True), K,
     dict(path="anti_residual", swap=False, ktype=rt.JOIN_INNER)),
    ("outer", facts("outer"), K, dict(path="pairs", swap=False,
                                      ktype=rt.JOIN_LEFT)),
    ("null_equal", facts(null_eq=True), K, dict(path="pairs")),
    ("cross", facts(keys=()), K, dict(path="cross")),
    # a WHERE that ran before the join (a shared one) builds the old way
    ("deferred_build_already_run",
     facts(l=side(400), r=side(100, deferred=True)), K,
     dict(path="fused", build_from_cols=False)),
    ("group_join_keeps_no_build_side",
     facts(l=side(100, **P), r=side(400, **P)), K,
     dict(path=None, fprobe="r", fbuild=None, swap=True,
          materialize=("l",))),
]


@pytest.mark.parametrize("name,f,k,exp", TABLE, ids=[t[0] for t in TABLE])
def test_route(name, f, k, exp):
    r = jp.route(f, k, group_join=name.startswith("group_join"))
    assert {a: getattr(r, a) for a in exp} == exp, r
    assert r.reason
    if r.path is not None:  # asked again, the answer stands
        assert jp.route(f, k, group_join=name.startswith("group_join")) == r


def test_group_join_route_builds_from_a_deferred_side():
    f = facts(l=side(100, mat=3, **P), r=side(400, **P))
    assert not jp.route(f, K._replace(disable_filterbuild=True)
                        ).build_from_cols
    r = jp.route(f, K, group_join=True)
    assert (r.path, r.fprobe, r.fbuild, r.build_from_cols) == (
        "fused", "r", None, True)
    wide = facts(l=side(100), r=side(400, n_cols=17, **P))
    assert jp.route(wide, K, group_join=True).fprobe == "r"


@pytest.mark.parametrize("jt", ["inner", "left", "right", "leftanti",
                                "outer", "cross"])
def test_fusable_per_join_type(jt):
    ok = jt in ("inner", "left", "right", "leftanti")
    assert jp.fusable(facts(jt), K) is ok
    assert not jp.fusable(facts(jt, keys=()), K)
    assert not jp.fusable(facts(jt, residual=True), K)
    assert not jp.fusable(facts(jt, null_eq=True), K)
    assert not jp.fusable(facts(jt, n_mat=17), K)
    assert jp.fusable(facts(jt, n_mat=16), K) is ok
    assert not jp.fusable(facts(jt), K._replace(disable_joinfuse=True))


@pytest.mark.parametrize("jt,small_l,large_l", [
    ("inner", (True, rt.JOIN_INNER), (False, rt.JOIN_INNER)),
    ("left", (False, rt.JOIN_LEFT), (False, rt.JOIN_LEFT)),
    ("right", (True, rt.JOIN_LEFT), (True, rt.JOIN_LEFT)),
    ("leftanti", (False, rt.JOIN_LEFTANTI), (False, rt.JOIN_LEFTANTI)),
    ("outer", (False, rt.JOIN_LEFT), (False, rt.JOIN_LEFT)),
])
def test_sides_per_join_type(jt, small_l, large_l):
    assert jp.sides(jt, 10, 20) == small_l
    assert jp.sides(jt, 20, 10) == large_l
    assert jp.sides(jt, 10, 10) == large_l  # a tie builds on the rhs
    # one rule with filter_build.build_side
    for n_l, n_r in ((10, 20), (20, 10)):
        assert jp.sides(jt, n_l, n_r)[0] == (
            fb.build_side(jt, None, n_l, n_r) == "l")


def test_forced_sides():
    assert jp.sides("inner", 10, 20, fprobe="l") == (False, rt.JOIN_INNER)
    assert jp.sides("inner", 20, 10, fprobe="r") == (True, rt.JOIN_INNER)
    assert jp.sides("inner", 20, 10, fbuild="l") == (True, rt.JOIN_INNER)
    assert jp.sides("inner", 10, 20, fbuild="r") == (False, rt.JOIN_INNER)
    assert jp.sides("inner", 10, 20, "r", "l") == (True, rt.JOIN_INNER)


JOIN_ENV = ("DSX_DISABLE_RADIX", "DSX_RADIX_MIN_BUILD", "DSX_RADIX_MIN_PROBE",
            "DSX_DISABLE_JOINFUSE", "DSX_DISABLE_FILTERPROBE",
            "DSX_DISABLE_FILTERBUILD", "DSX_FILTERBUILD_MAX_ROWS",
            "DSX_FILTERBUILD_MIN_ROWS")


def test_knobs(monkeypatch):
    for name in JOIN_ENV:
        monkeypatch.delenv(name, raising=False)
    assert jp.knobs() == jp.Knobs(
        False, 8_000_000, 4_000_000, False, False, False,
        fb.DEFAULT_MAX_ROWS, fb.DEFAULT_MIN_ROWS)
    for name in JOIN_ENV:
        monkeypatch.setenv(name, "1")
    assert jp.knobs() == jp.Knobs(True, 1, 1, True, True, True, 1, 1)
    # "0": the join's own switches are on when set at all, the build-from-
    # columns one reads "0" as off — each as before
    for name in JOIN_ENV:
        monkeypatch.setenv(name, "0")
    assert jp.knobs() == jp.Knobs(True, 0, 0, True, True, False, 0, 0)
    for name in JOIN_ENV:
        monkeypatch.setenv(name, "")
    monkeypatch.setenv("DSX_RADIX_MIN_BUILD", "12")
    monkeypatch.setenv("DSX_RADIX_MIN_PROBE", "13")
    monkeypatch.setenv("DSX_FILTERBUILD_MAX_ROWS", "many")
    monkeypatch.setenv("DSX_FILTERBUILD_MIN_ROWS", "few")
    assert jp.knobs() == jp.Knobs(
        False, 12, 13, False, False, False, fb.DEFAULT_MAX_ROWS,
        fb.DEFAULT_MIN_ROWS)
    # a radix size that is no integer was an error and is one
    monkeypatch.setenv("DSX_RADIX_MIN_BUILD", "big")
    with pytest.raises(ValueError):
        jp.knobs()
    monkeypatch.setenv("DSX_RADIX_MIN_BUILD", "12")
    monkeypatch.setenv("DSX_RADIX_MIN_PROBE", "big")
    with pytest.raises(ValueError):
        jp.knobs()


def test_the_join_reads_no_environment_itself():
    from dask_sql_amd.physical import join
    src = inspect.getsource(join)
    assert "os.environ" not in src and "import os" not in src
