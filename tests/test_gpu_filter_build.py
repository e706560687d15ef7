"""Hash build straight from source columns (dsx_hash_build_cols, -m gpu).

Entry level: a table built by Runtime.hash_build_cols is probed with
hash_probe and the (probe row, build row) pairs are compared with numpy; and
for each key-filter mode the fused probe (filter_probe_cols) over it equals
the fused probe over a table from the old entry (keypack + hash_build) built
on the compacted rows, a gathered build-side value standing for the row id.
The probe side of those cases holds EVERY code of the key range, so an exact
bitmap is checked bit for bit (in that mode a hit is the bit alone).

SQL level: the planner's routing (physical/filter_build.py) against the
oracle / pandas and against DSX_DISABLE_FILTERBUILD=1, with the launch counts
that tell the two paths apart. These tables are smaller than the build-row
minimum from which the planner takes the entry, so the SQL cases lift it
(DSX_FILTERBUILD_MIN_ROWS=0), as the group-join's cases lift theirs; one case
checks the default."""
import numpy as np
import pandas as pd
import pytest

from tests.conftest import assert_frame_close
from tests.test_gpu_filter_probe import _norm

pytestmark = pytest.mark.gpu

SIZES = [4097, 65573]  # one past a block multiple; many blocks
OP_COL, OP_LIT_I64, OP_LT_I64 = 1, 3, 30
NONE, EXACT, HASHED = 0, 1, 2
KNOBS = ("DSX_DISABLE_FILTERBUILD", "DSX_FILTERBUILD_MAX_ROWS",
         "DSX_FILTERBUILD_MIN_ROWS",
         "DSX_DISABLE_JOINFILTER", "DSX_JOIN_FILTER_MAX_BYTES",
         "DSX_JOIN_FILTER_MIN_BITS", "DSX_GROUPJOIN_MIN_ROWS",
         "DSX_DISABLE_BUILD_RUNCOMBINE")
OLD_KERNELS = ("k_filter_mask", "k_filter_emit_cols", "k_keypack", "k_eval")


@pytest.fixture(scope="module")
def runtime():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    return Context()._get_runtime()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _launches(prof, name):
    return prof.get(name, {}).get("launches", 0)


def _up(r, arr, valid=None):
    return r.upload_column(np.ascontiguousarray(arr),
                           None if valid is None else valid.astype(np.uint8))


def _lt_prog(r, thresh):
    """column 0 < thresh (NULL -> not kept)"""
    return r.make_prog([(OP_COL, 0, 0), (OP_LIT_I64, 0, thresh),
                        (OP_LT_I64, 0, 0)])


def _pred_col(n, rng):
    f = rng.integers(0, 100, n).astype(np.int64)
    fv = rng.random(n) >= 0.1
    return f, fv


def _sel_to_np(r, ptr, count):
    sel = r.wrap_sel(ptr, count)  # owns the buffer either way
    if count == 0:
        return np.empty(0, dtype=np.int64)
    arr, _ = sel.to_numpy()
    return arr.astype(np.uint32).astype(np.int64)


def _pairs(r, table, pcodes):
    from dask_sql_amd import runtime as rt
    p, b, cnt = r.hash_probe(table, pcodes, rt.JOIN_INNER, None)
    got = np.stack([_sel_to_np(r, p, cnt), _sel_to_np(r, b, cnt)], axis=1)
    return got[np.lexsort((got[:, 1], got[:, 0]))]


def _expected_pairs(bcodes, kept, pcodes):
    e = pd.DataFrame({"c": pcodes, "p": np.arange(len(pcodes))}).merge(
        pd.DataFrame({"c": bcodes[kept], "b": np.flatnonzero(kept)}), on="c")
    e = e[["p", "b"]].to_numpy(dtype=np.int64)
    return e[np.lexsort((e[:, 1], e[:, 0]))]


# ---------------------------------------------------------------------------
# entry level: pairs against numpy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["no_predicate", "one_in_five", "no_row",
                                  "every_row", "null_keys", "composite",
                                  "unpacked"])
@pytest.mark.parametrize("n", SIZES)
def test_pairs_equal_numpy(runtime, n, case):
    r = runtime
    rng = np.random.default_rng(n + len(case))
    f, fv = _pred_col(n, rng)
    if case == "every_row":
        fv[:] = True
    thresh = {"one_in_five": 20, "no_row": -1, "every_row": 1000}.get(case)
    kept = np.ones(n, dtype=bool) if thresh is None else (f < thresh) & fv
    kv = None
    m = n + 13
    if case == "composite":
        r1, r2 = 1 << 9, (2 * n >> 9) + 1
        flat = rng.choice(r1 * r2, n, replace=False)
        k1, k2 = flat % r1, flat // r1 + 5       # second key's minimum is 5
        pflat = rng.integers(0, r1 * r2, m)
        bkeys, pkeys = [k1, k2], [pflat % r1, pflat // r1 + 5]
        specs = [(0, r1), (5, r2)]
        bcodes, pcodes = flat, pflat
    else:
        rg = 2 * n
        k = rng.choice(rg, n, replace=False).astype(np.int64)
        pk = rng.integers(0, rg, m).astype(np.int64)
        if case == "unpacked":  # codes >= 2^32: (code, row id) in two words
            rg = (1 << 33) + 2 * n
            k[::3] += 1 << 33
            pk[::2] += 1 << 33
        if case == "null_keys":
            kv = rng.random(n) >= 0.2
            kept &= kv
        bkeys, pkeys, specs = [k], [pk], [(0, rg)]
        bcodes, pcodes = k, pk
    space = int(np.prod([rg_ for _, rg_ in specs], dtype=object))
    src = [_up(r, f, fv)] + [
        _up(r, np.asarray(c, dtype=np.int64), kv if i == 0 else None)
        for i, c in enumerate(bkeys)]
    keyspecs = [(1 + i, mn, rg_, False) for i, (mn, rg_) in enumerate(specs)]
    prog = None if thresh is None else _lt_prog(r, thresh)
    r.prof_enable(True)
    r.prof_reset()
    table = r.hash_build_cols(prog, src, keyspecs, n, code_max=space - 1)
    prof = r.prof_get()
    r.prof_enable(False)
    try:
        assert _launches(prof, "k_hash_build") == 1
        for name in OLD_KERNELS:  # a nullable key costs no k_eval either
            assert _launches(prof, name) == 0, name
        pc, _ = r.keypack(
            [_up(r, np.asarray(c, dtype=np.int64)) for c in pkeys],
            [(i, mn, rg_, False) for i, (mn, rg_) in enumerate(specs)], m)
        got = _pairs(r, table, pc)
    finally:
        r.hash_table_free(table)
    exp = _expected_pairs(np.asarray(bcodes, dtype=np.int64), kept,
                          np.asarray(pcodes, dtype=np.int64))
    if case == "no_row":
        assert len(exp) == 0
    elif case == "one_in_five":
        assert 0.1 * n < kept.sum() < 0.3 * n and len(exp) > 0
    else:
        assert len(exp) > 0.2 * n
    if case == "unpacked":
        assert (np.asarray(bcodes)[exp[:, 1]] >= 1 << 32).any()
    assert got.shape == exp.shape and (got == exp).all()


# ---------------------------------------------------------------------------
# entry level: the three filter modes, every key order, new entry = old entry
# ---------------------------------------------------------------------------
MODE_ENV = {
    EXACT: {},
    HASHED: {"DSX_JOIN_FILTER_MAX_BYTES": "64",
             "DSX_JOIN_FILTER_MIN_BITS": "0"},
    NONE: {"DSX_JOIN_FILTER_MAX_BYTES": "64"},
}


def _fused_probe(r, table, pf, pk, rg, bval):
    """rid and the build-side value of every match, by probe row"""
    res = r.filter_probe_cols(table, _lt_prog(r, 1000), [pf, pk],
                              [(1, 0, rg, False)], pk.len, [pk], [bval])
    if res is None:
        return None
    cols, cnt = res
    k, _ = cols[0].to_numpy()
    v, _ = cols[1].to_numpy()
    assert cnt == len(k)
    return pd.DataFrame({"k": k, "bv": v})


@pytest.mark.parametrize("mode", [EXACT, HASHED, NONE],
                         ids=["exact", "hashed", "none"])
@pytest.mark.parametrize("order", ["sorted", "reversed", "shuffled"])
@pytest.mark.parametrize("n", SIZES)
def test_filter_modes_equal_old_entry(runtime, monkeypatch, n, order, mode):
    """Dense keys, so that sorted keys put 32 neighbouring lanes into one
    filter word (the longest run there is), reversed keys run the other way
    and shuffled keys give runs of one; with the predicate on, dropped rows
    break the runs at random places."""
    r = runtime
    rng = np.random.default_rng(n)
    rg = n + 100
    k = rng.choice(rg, n, replace=False).astype(np.int64)
    if order != "shuffled":
        k.sort()
    if order == "reversed":
        k = k[::-1].copy()
    f, fv = _pred_col(n, rng)
    val = rng.integers(0, 1 << 40, n).astype(np.int64)
    allk = rng.permutation(rg).astype(np.int64)  # every code of the range
    pk, pf = _up(r, allk), _up(r, np.zeros(rg, dtype=np.int64))
    for k_, v_ in MODE_ENV[mode].items():
        monkeypatch.setenv(k_, v_)
    for thresh in (None, 20):
        kept = np.ones(n, dtype=bool) if thresh is None else (f < thresh) & fv
        new = r.hash_build_cols(
            None if thresh is None else _lt_prog(r, thresh),
            [_up(r, f, fv), _up(r, k)], [(1, 0, rg, False)], n,
            code_max=rg - 1, key_filter=True)
        codes, space = r.keypack([_up(r, k[kept])], [(0, 0, rg, False)],
                                 int(kept.sum()))
        old = r.hash_build(codes, None, code_max=space - 1, key_filter=True)
        try:
            assert r.hash_table_filter(new)[0] == mode
            assert r.hash_table_filter(new) == r.hash_table_filter(old)
            got = _fused_probe(r, new, pf, pk, rg, _up(r, val))
            ref = _fused_probe(r, old, pf, pk, rg, _up(r, val[kept]))
        finally:
            r.hash_table_free(new)
            r.hash_table_free(old)
        lut = np.full(rg, -1, dtype=np.int64)
        lut[k[kept]] = val[kept]
        exp = pd.DataFrame({"k": allk, "bv": lut[allk]})
        exp = exp[exp["bv"] >= 0].reset_index(drop=True)
        assert len(exp) == kept.sum()
        pd.testing.assert_frame_equal(got, ref)   # same rows, same order
        pd.testing.assert_frame_equal(got, exp, check_dtype=False)


def test_run_combine_knob_gives_the_same_bitmap(runtime, monkeypatch):
    """one atomic per row (knob) and one per run: the same exact filter"""
    r = runtime
    n, rg = 65573, 65573 + 100
    rng = np.random.default_rng(5)
    k = np.sort(rng.choice(rg, n, replace=False)).astype(np.int64)
    allk = np.arange(rg, dtype=np.int64)
    pk, pf = _up(r, allk), _up(r, np.zeros(rg, dtype=np.int64))
    frames = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("DSX_DISABLE_BUILD_RUNCOMBINE", "1")
        t = r.hash_build_cols(None, [_up(r, k)], [(0, 0, rg, False)], n,
                              code_max=rg - 1, key_filter=True)
        try:
            assert r.hash_table_filter(t)[0] == EXACT
            frames.append(_fused_probe(r, t, pf, pk, rg, _up(r, k)))
        finally:
            r.hash_table_free(t)
    pd.testing.assert_frame_equal(frames[0], frames[1])
    assert (frames[0]["k"].to_numpy() == k).all()


def test_duplicate_build_keys_not_applicable(runtime):
    r = runtime
    n, rg = 4097, 8194
    rng = np.random.default_rng(6)
    k = rng.choice(rg, n, replace=False).astype(np.int64)
    f = np.zeros(n, dtype=np.int64)
    k[4000] = k[17]            # a duplicate among the kept rows …
    pk, pf = _up(r, np.arange(rg, dtype=np.int64)), _up(
        r, np.zeros(rg, dtype=np.int64))
    t = r.hash_build_cols(_lt_prog(r, 20), [_up(r, f), _up(r, k)],
                          [(1, 0, rg, False)], n, code_max=rg - 1,
                          key_filter=True)
    try:
        assert _fused_probe(r, t, pf, pk, rg, _up(r, k)) is None
    finally:
        r.hash_table_free(t)
    f[4000] = 50               # … and the same one filtered away
    t = r.hash_build_cols(_lt_prog(r, 20), [_up(r, f), _up(r, k)],
                          [(1, 0, rg, False)], n, code_max=rg - 1,
                          key_filter=True)
    try:
        got = _fused_probe(r, t, pf, pk, rg, _up(r, k))
        assert got is not None and len(got) == n - 1
    finally:
        r.hash_table_free(t)


# ---------------------------------------------------------------------------
# SQL level
# ---------------------------------------------------------------------------
def _sql_on_off(monkeypatch, tables, sql, env=None):
    """(frame, prof) with the build from columns, then with the knob off"""
    from dask_sql_amd.context import Context
    c = Context()
    for name, df in tables.items():
        c.create_table(name, df)
    r = c._get_runtime()
    monkeypatch.setenv("DSX_FILTERBUILD_MIN_ROWS", "0")
    for k_, v_ in (env or {}).items():
        monkeypatch.setenv(k_, v_)
    r.prof_enable(True)
    res = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("DSX_DISABLE_FILTERBUILD", "1")
        else:
            monkeypatch.delenv("DSX_DISABLE_FILTERBUILD", raising=False)
        r.prof_reset()
        res += [c.sql(sql).compute(), r.prof_get()]
    monkeypatch.delenv("DSX_DISABLE_FILTERBUILD", raising=False)
    r.prof_enable(False)
    return tuple(res)


def _tables(n, rng, dup=False):
    """p: n rows, key k (nullable) into b's bk; b: n // 4 rows, unique bk,
    a predicate column b32 and value columns."""
    nb = n // 4
    k = pd.array(rng.integers(0, nb + nb // 2, n), dtype="Int64")
    k[rng.random(n) < 0.05] = pd.NA
    p = pd.DataFrame({"rid": np.arange(n, dtype=np.int64), "k": k,
                      "f": rng.integers(0, 100, n).astype(np.int64),
                      "x": rng.random(n)})
    bk = rng.permutation(nb + nb // 2)[:nb].astype(np.int64)
    if dup:
        bk[1] = bk[0]
    b = pd.DataFrame({"bk": bk,
                      "b32": rng.integers(0, 100, nb).astype(np.int32),
                      "bv": rng.integers(0, 1 << 40, nb).astype(np.int64),
                      "bf": rng.random(nb)})
    return p, b


def _pandas_join(p, b, how="inner"):
    j = p.merge(b, left_on="k", right_on="bk", how=how)
    return j[["rid", "k", "bk", "bv", "bf"]]


SQL_BUILD_WHERE = ("SELECT p.rid, p.k, b.bk, b.bv, b.bf FROM p {j} b "
                   "ON p.k = b.bk WHERE b.b32 < 20")
SQL_BOTH_WHERE = ("SELECT p.rid, p.k, b.bk, b.bv, b.bf FROM p JOIN b "
                  "ON p.k = b.bk WHERE b.b32 < 20 AND p.f < 50")


@pytest.mark.parametrize("n", [5000, 200_000])
def test_q3_mini(runtime, monkeypatch, n):
    from datagen import Q3_SQL, gen_q3, register_q3_tables
    from dask_sql_amd.context import Context
    from oracle.tpch import oracle_q3
    cust, orders, li = gen_q3(sf_rows=(n // 10, n, 4 * n))
    c = Context()
    register_q3_tables(c, cust, orders, li)
    r = c._get_runtime()
    monkeypatch.setenv("DSX_GROUPJOIN_MIN_ROWS", "0")  # as at benchmark size
    monkeypatch.setenv("DSX_FILTERBUILD_MIN_ROWS", "0")
    r.prof_enable(True)
    r.prof_reset()
    out = c.sql(Q3_SQL).compute()
    prof = r.prof_get()
    monkeypatch.setenv("DSX_DISABLE_FILTERBUILD", "1")
    r.prof_reset()
    off = c.sql(Q3_SQL).compute()
    prof_off = r.prof_get()
    r.prof_enable(False)
    print({k_: v_["launches"] for k_, v_ in prof.items()})
    print({k_: v_["launches"] for k_, v_ in prof_off.items()})
    assert _launches(prof, "k_hash_build") == 2
    for name in OLD_KERNELS:
        assert _launches(prof, name) == 0, name
    assert _launches(prof_off, "k_keypack") == 2
    assert _launches(prof_off, "k_filter_mask") == 1
    exp = oracle_q3(cust, orders, li)
    assert len(out) == len(exp)
    assert (out["l_orderkey"].to_numpy().astype(np.int64)
            == exp["l_orderkey"].to_numpy()).all()
    assert np.allclose(out["revenue"], exp["revenue"], rtol=1e-9)
    days = out["o_orderdate"].to_numpy().astype("datetime64[D]").astype(
        np.int64)
    assert (days == exp["o_orderdate"].to_numpy()).all()
    # the knob changes how the tables are built, not what they hold
    assert list(out.columns) == list(off.columns) and len(out) == len(off)
    for col in out.columns:
        a, b = out[col].to_numpy(), off[col].to_numpy()
        if col == "revenue":  # summed by atomics: the project's 16 ulp bound
            assert np.allclose(a, b, rtol=16 * 2.0 ** -53, atol=0)
        else:
            assert (a == b).all(), col


@pytest.mark.parametrize("both", [False, True], ids=["build", "both"])
@pytest.mark.parametrize("n", [5000, 200_000])
def test_sql_inner_join_gathers_base_rows(runtime, monkeypatch, n, both):
    """a build-side value column under a build-side WHERE: the table's row
    ids index the base columns and must gather the right rows"""
    rng = np.random.default_rng(n)
    p, b = _tables(n, rng)
    sql = SQL_BOTH_WHERE if both else SQL_BUILD_WHERE.format(j="JOIN")
    got, prof, off, prof_off = _sql_on_off(monkeypatch, {"p": p, "b": b}, sql)
    assert _launches(prof, "k_hash_build") == 1
    # an unfiltered probe side still packs its own codes (and evaluates its
    # nullable key's validity); the build side's passes are gone either way
    gone = OLD_KERNELS if both else OLD_KERNELS[:2]
    for name in gone:
        assert _launches(prof, name) == 0, name
    assert _launches(prof_off, "k_filter_mask") == 1
    assert _launches(prof_off, "k_filter_emit_cols") == 1
    assert _launches(prof_off, "k_keypack") == _launches(prof, "k_keypack") + 1
    exp = _pandas_join(p[p["f"] < 50] if both else p, b[b["b32"] < 20])
    assert 0 < len(exp) < n
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid"])


@pytest.mark.parametrize("n", [5000, 200_000])
def test_sql_left_join_takes_the_old_path(runtime, monkeypatch, n):
    rng = np.random.default_rng(n + 1)
    p, b = _tables(n, rng)
    # b LEFT JOIN p would probe with b; p LEFT JOIN (filtered b) builds on b
    sql = ("SELECT p.rid, p.k, q.bk, q.bv, q.bf FROM p LEFT JOIN "
           "(SELECT * FROM b WHERE b32 < 20) q ON p.k = q.bk")
    got, prof, off, prof_off = _sql_on_off(monkeypatch, {"p": p, "b": b}, sql)
    for pr in (prof, prof_off):  # the old kernels, with the knob and without
        assert _launches(pr, "k_filter_mask") == 1
        assert _launches(pr, "k_filter_emit_cols") == 1
        assert _launches(pr, "k_keypack") >= 1
    exp = _pandas_join(p, b[b["b32"] < 20], how="left")
    assert len(exp) == n
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid"])


@pytest.mark.parametrize("n", [5000, 200_000])
def test_sql_cap_exceeded(runtime, monkeypatch, n):
    rng = np.random.default_rng(n + 2)
    p, b = _tables(n, rng)
    got, prof, off, _ = _sql_on_off(
        monkeypatch, {"p": p, "b": b}, SQL_BUILD_WHERE.format(j="JOIN"),
        env={"DSX_FILTERBUILD_MAX_ROWS": str(len(b) - 1)})
    assert _launches(prof, "k_filter_mask") == 1      # the filter ran first
    assert _launches(prof, "k_keypack") >= 1          # … and the old build
    exp = _pandas_join(p, b[b["b32"] < 20])
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid"])
    # exactly at the cap the side stays pending
    got2, prof2, _, _ = _sql_on_off(
        monkeypatch, {"p": p, "b": b}, SQL_BUILD_WHERE.format(j="JOIN"),
        env={"DSX_FILTERBUILD_MAX_ROWS": str(len(b))})
    assert _launches(prof2, "k_filter_mask") == 0
    assert_frame_close(_norm(got2), _norm(exp), sort_by=["rid"])


def test_sql_row_minimum_default(runtime, monkeypatch):
    """Default knobs: a build side below the minimum keeps the old kernels,
    one at it goes through the entry; both give the pandas rows."""
    from dask_sql_amd.physical import filter_build as fb
    for nb, old in ((fb.DEFAULT_MIN_ROWS - 1, True),
                    (fb.DEFAULT_MIN_ROWS, False)):
        rng = np.random.default_rng(nb)
        p, b = _tables(4 * nb + 4, rng)
        b = b.iloc[:nb].reset_index(drop=True)
        got, prof, _, _ = _sql_on_off(
            monkeypatch, {"p": p, "b": b}, SQL_BOTH_WHERE,
            env={"DSX_FILTERBUILD_MIN_ROWS": str(fb.DEFAULT_MIN_ROWS)})
        assert _launches(prof, "k_filter_mask") == (1 if old else 0)
        assert _launches(prof, "k_keypack") == (1 if old else 0)
        exp = _pandas_join(p[p["f"] < 50], b[b["b32"] < 20])
        assert len(exp) > 0
        assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])


@pytest.mark.parametrize("n", [5000, 200_000])
def test_sql_duplicate_build_keys_fall_back(runtime, monkeypatch, n):
    rng = np.random.default_rng(n + 3)
    p, b = _tables(n, rng, dup=True)
    b.loc[[0, 1], "b32"] = 0  # both rows of the duplicate key survive
    got, prof, off, _ = _sql_on_off(monkeypatch, {"p": p, "b": b},
                                    SQL_BOTH_WHERE)
    assert _launches(prof, "k_fprobe_mask") == 1       # tried …
    assert _launches(prof, "k_fprobe_emit") == 0       # … not applicable
    assert _launches(prof, "k_hash_probe_count") == 1  # same table, two-pass
    assert _launches(prof, "k_hash_build") == 1
    exp = _pandas_join(p[p["f"] < 50], b[b["b32"] < 20])
    assert (exp["bk"] == b.loc[0, "bk"]).sum() >= 2
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid", "bv"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid", "bv"])
