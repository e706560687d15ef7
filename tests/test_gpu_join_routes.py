"""Every flat route of the join (physical/join_plan.py) end to end, -m gpu:
one SQL statement per route over three small tables, compared with pandas
and, by its per-kernel launch counts, with tests/golden/join_route_launches.json
(recorded with this file's statements at the commit before the routing moved
into physical/join_plan.py; `python -m tests.test_gpu_join_routes` prints it).
The radix route needs its own sizes and stays in test_gpu_semantics.py.

Rows: 4,097 (one past a block multiple), 1,031 (odd, a few blocks) and 257
(under one block). About one key in five has no partner, some keys are NULL,
and one column is a dictionary string. The tables are smaller than the row
minimums from which the planner takes the build-from-columns entry and the
group-join, so both are lifted, as the neighbouring SQL tests do."""
import json
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests.conftest import assert_frame_close
from tests.test_gpu_filter_probe import _norm

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "join_route_launches.json"
KNOBS = ("DSX_DISABLE_RADIX", "DSX_RADIX_MIN_BUILD", "DSX_RADIX_MIN_PROBE",
         "DSX_DISABLE_JOINFUSE", "DSX_DISABLE_FILTERPROBE",
         "DSX_DISABLE_FILTERBUILD", "DSX_FILTERBUILD_MAX_ROWS",
         "DSX_DISABLE_GROUPJOIN")
LIFTED = {"DSX_FILTERBUILD_MIN_ROWS": "0", "DSX_GROUPJOIN_MIN_ROWS": "0"}
NA, NB, NC = 4097, 1031, 257


def make_tables():
    rng = np.random.default_rng(13)
    # a.k → b.bk, b.ck → c.ckey: the key range is a quarter wider than the
    # unique build keys drawn from it, so about one probe key in five misses
    rb, rc = NB + NB // 4, NC + NC // 4
    k = pd.array(rng.integers(0, rb, NA), dtype="Int64")
    k[rng.random(NA) < 0.03] = pd.NA
    a = pd.DataFrame({
        "rid": np.arange(NA, dtype=np.int64), "k": k,
        "kf": k.astype("float64"),
        "f": rng.integers(0, 100, NA).astype(np.int64),
        "x": rng.random(NA),
        "s": rng.choice(["ash", "birch", "cedar", "elm"], NA)})
    ck = pd.array(rng.integers(0, rc, NB), dtype="Int64")
    ck[rng.random(NB) < 0.03] = pd.NA
    bk = rng.permutation(rb)[:NB].astype(np.int64)
    b = pd.DataFrame({
        "bk": bk, "bkf": bk.astype(np.float64), "ck": ck,
        "b32": rng.integers(0, 100, NB).astype(np.int32),
        "bv": rng.integers(0, 1 << 40, NB).astype(np.int64)})
    bdup = b.copy()
    bdup.loc[1, "bk"] = bdup.loc[0, "bk"]  # one duplicate build key
    c = pd.DataFrame({
        "ckey": rng.permutation(rc)[:NC].astype(np.int64),
        "cv": rng.integers(0, 1000, NC).astype(np.int64)})
    return {"a": a, "b": b, "bdup": bdup, "c": c}


def _inner(a, b):
    return a.merge(b, left_on="k", right_on="bk")


def _exp_fused(t):
    return _inner(t["a"], t["b"])[["rid", "k", "s", "bv"]]


def _exp_filter_probe(t):
    a = t["a"]
    return _inner(a[a["f"] < 50], t["b"])[["rid", "k", "s", "bv"]]


def _exp_filter_build(t):
    b = t["b"]
    return _inner(t["a"], b[b["b32"] < 20])[["rid", "k", "s", "bv"]]


def _exp_filter_build_left(t):
    b = t["b"]
    j = t["a"].merge(b[b["b32"] < 20], left_on="k", right_on="bk",
                     how="left")
    return j[["rid", "k", "bk", "bv"]]


def _exp_group_join(t):
    a = t["a"]
    j = _inner(a[a["f"] < 50], t["b"])
    g = j.groupby(["bk", "bv"], as_index=False).agg(
        sx=("x", "sum"), n=("x", "size"))
    return g[["bk", "bv", "sx", "n"]]


def _exp_duplicate_keys(t):
    a = t["a"]
    return _inner(a[a["f"] < 50], t["bdup"])[["rid", "k", "s", "bv"]]


def _exp_float_key(t):
    a, b = t["a"], t["b"]
    j = a[a["kf"].notna()].merge(b, left_on="kf", right_on="bkf")
    return j[["rid", "kf", "bv"]]


def _exp_full_outer(t):
    b, c = t["b"], t["c"]
    hit = b[b["ck"].notna()].merge(c, left_on="ck", right_on="ckey")
    lone_b = b[~b["bk"].isin(hit["bk"])]
    lone_c = c[~c["ckey"].isin(hit["ckey"])]
    j = pd.concat([hit, lone_b, lone_c], ignore_index=True)
    return j[["bk", "ck", "ckey", "cv"]]


def _exp_residual(t):
    j = _inner(t["a"], t["b"])
    return j[j["f"] < j["b32"]][["rid", "k", "f", "b32"]]


_SEL = "SELECT a.rid, a.k, a.s, b.bv FROM a JOIN "
# route → (statement, pandas result, sort columns[, knobs])
ROUTES = {
    # below the build-row minimum: keypack + hash_build
    "fused": (_SEL + "b ON a.k = b.bk", _exp_fused, ["rid"],
              {"DSX_FILTERBUILD_MIN_ROWS": "4096"}),
    "filter_build_materialized": (_SEL + "b ON a.k = b.bk", _exp_fused,
                                  ["rid"]),
    "filter_probe": (_SEL + "b ON a.k = b.bk WHERE a.f < 50",
                     _exp_filter_probe, ["rid"]),
    "filter_build_pending": (_SEL + "b ON a.k = b.bk WHERE b.b32 < 20",
                             _exp_filter_build, ["rid"]),
    # a LEFT join's filtered build side runs its WHERE first
    "left_filtered_build": (
        "SELECT a.rid, a.k, q.bk, q.bv FROM a LEFT JOIN "
        "(SELECT * FROM b WHERE b32 < 20) q ON a.k = q.bk",
        _exp_filter_build_left, ["rid"]),
    "group_join": (
        "SELECT b.bk, b.bv, SUM(a.x) AS sx, COUNT(*) AS n FROM a JOIN b "
        "ON a.k = b.bk WHERE a.f < 50 GROUP BY b.bk, b.bv",
        _exp_group_join, ["bk"]),
    "duplicate_keys": (
        "SELECT a.rid, a.k, a.s, bdup.bv FROM a JOIN bdup "
        "ON a.k = bdup.bk WHERE a.f < 50", _exp_duplicate_keys,
        ["rid", "bv"]),
    "float_key": ("SELECT a.rid, a.kf, b.bv FROM a JOIN b ON a.kf = b.bkf",
                  _exp_float_key, ["rid"]),
    "full_outer": ("SELECT b.bk, b.ck, c.ckey, c.cv FROM b FULL JOIN c "
                   "ON b.ck = c.ckey", _exp_full_outer, ["bk", "ckey"]),
    "residual": ("SELECT a.rid, a.k, a.f, b.b32 FROM a JOIN b "
                 "ON a.k = b.bk AND a.f < b.b32", _exp_residual, ["rid"]),
}


@pytest.fixture(scope="module")
def world():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    tables = make_tables()
    ctx = Context()
    for name, df in tables.items():
        ctx.create_table(name, df)
    return ctx, tables


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k in LIFTED:
        monkeypatch.delenv(k, raising=False)


def run_route(ctx, route):
    """(frame, {kernel: launches}) of one statement, on its second run: the
    first one computes and caches the base columns' statistics."""
    import os
    r = ctx._get_runtime()
    saved = {k: os.environ.get(k) for k in LIFTED}
    os.environ.update(LIFTED)
    os.environ.update(ROUTES[route][3] if len(ROUTES[route]) > 3 else {})
    try:
        ctx.sql(ROUTES[route][0]).compute()
        r.prof_enable(True)
        r.prof_reset()
        out = ctx.sql(ROUTES[route][0]).compute()
        prof = r.prof_get()
    finally:
        r.prof_enable(False)
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out, {k: v["launches"] for k, v in sorted(prof.items())
                 if v["launches"]}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route_matches_pandas_and_recorded_launches(world, route):
    ctx, tables = world
    expected, sort_by = ROUTES[route][1:3]
    got, launches = run_route(ctx, route)
    exp = expected(tables)
    assert 0 < len(exp)
    got, exp = _norm(got), _norm(exp)
    assert_frame_close(got, exp, sort_by=sort_by)
    print(route, launches)
    assert launches == json.loads(GOLDEN.read_text())[route]


def test_the_statements_take_their_routes():
    """The recorded counts tell the routes apart as their names say."""
    rec = json.loads(GOLDEN.read_text())
    assert sorted(rec) == sorted(ROUTES)

    def n(route, kernel):
        return rec[route].get(kernel, 0)

    assert n("fused", "k_keypack") == 2 and n("fused", "k_hash_probe_mat")
    assert n("filter_build_materialized", "k_keypack") == 1
    assert n("filter_build_materialized", "k_hash_build") == 1
    assert n("filter_probe", "k_fprobe_emit") == 1
    assert not n("filter_probe", "k_filter_mask")
    assert n("filter_build_pending", "k_hash_build") == 1
    assert not n("filter_build_pending", "k_filter_mask")
    assert n("left_filtered_build", "k_filter_mask") == 1
    assert n("group_join", "k_fprobe_agg") == 1
    assert n("duplicate_keys", "k_fprobe_mask") == 1
    assert not n("duplicate_keys", "k_fprobe_emit")
    assert n("duplicate_keys", "k_hash_probe_count") == 1
    for route in ("float_key", "full_outer", "residual"):
        assert n(route, "k_hash_probe_emit") and n(route, "k_gather"), route


if __name__ == "__main__":
    import os
    import sys
    from dask_sql_amd.context import Context
    for k in KNOBS:
        os.environ.pop(k, None)
    ctx = Context()
    for name, df in make_tables().items():
        ctx.create_table(name, df)
    rec = {route: run_route(ctx, route)[1] for route in sorted(ROUTES)}
    sys.stdout.write(json.dumps(rec, indent=1, sort_keys=True) + "\n")
