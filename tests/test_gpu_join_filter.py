"""Key-membership filter of the fused filter-probe join (dsx_hash_build_filtered
+ dsx_filter_probe_cols, -m gpu).

Direct Runtime calls over a 1 000-row build side with keys in a range of
1 500. Every case is compared, after sorting, with the oracle join
(oracle/frame.py) over pandas-filtered inputs and with the same calls under
DSX_DISABLE_JOINFILTER=1; the table's filter mode is read back, so a case
cannot pass on another path than the one it names; and every case runs with
the generated mask kernel and with the interpreter (DSX_DISABLE_JIT_FPROBE=1).

Two knobs place the hashed mode where these sizes would not: an exact bitmap
over 1 500 codes is 188 bytes, less than a hashed filter of 1 000 keys at the
minimum density, so the packed hashed case takes DSX_JOIN_FILTER_MAX_BYTES=64
together with DSX_JOIN_FILTER_MIN_BITS=0 (64 bytes for 1 000 keys: nearly
every bit set, false positives all over, the result still exact). The same cap
at the default minimum density is the "filter dropped" case."""
import numpy as np
import pandas as pd
import pytest

from tests.conftest import assert_frame_close
from tests.test_gpu_filter_probe import (_download, _mask, _norm, _oracle,
                                         _probe_frame, _upload)

pytestmark = pytest.mark.gpu

N_BUILD, KEY_RANGE = 1000, 1500
OP_COL, OP_LIT_I64, OP_LT_I64 = 1, 3, 30
NONE, EXACT, HASHED = 0, 1, 2
KNOBS = ("DSX_DISABLE_JOINFILTER", "DSX_JOIN_FILTER_MAX_BYTES",
         "DSX_JOIN_FILTER_MIN_BITS", "DSX_DISABLE_JIT_FPROBE",
         "DSX_DISABLE_FILTERPROBE")
KERNELS = pytest.mark.parametrize("interp", [False, True],
                                  ids=["generated", "interpreter"])
NAMES = ["rid", "x", "nv", "bv", "bn"]


@pytest.fixture(scope="module")
def runtime():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    return Context()._get_runtime()


def _build(rng, n=N_BUILD, key_range=KEY_RANGE, ends=True):
    keys = rng.choice(key_range, n, replace=False).astype(np.int64)
    if ends and n >= 2:  # both ends of the code range are build keys
        rest = keys[~np.isin(keys, [0, key_range - 1])]
        keys = np.concatenate([[0, key_range - 1], rest])[:n]
    bn = pd.array(rng.integers(0, 50, n), dtype="Int64")
    if n:
        bn[rng.random(n) < 0.3] = pd.NA
    return pd.DataFrame({"bk": keys,
                         "bv": rng.integers(0, 1 << 40, n).astype(np.int64),
                         "bn": bn})


def _run(r, monkeypatch, p, b, env, pkeys=("k",), bkeys=("bk",),
         ranges=((0, KEY_RANGE),), thresh=50):
    """One build + fused probe under `env`: (frame or None, mode, bytes,
    launches of the generated kernel)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pc = {c: _upload(r, p[c]) for c in ["rid", "f", "x", "nv", *pkeys]}
    bc = {c: _upload(r, b[c]) for c in ["bv", "bn", *bkeys]}
    prog = r.make_prog([(OP_COL, 0, 0), (OP_LIT_I64, 0, thresh),
                        (OP_LT_I64, 0, 0)])
    bcodes, space = r.keypack(
        [bc[k] for k in bkeys],
        [(i, mn, rg, False) for i, (mn, rg) in enumerate(ranges)], len(b))
    bvalid = bc[bkeys[0]].validity if len(bkeys) == 1 else None
    table = r.hash_build(bcodes, bvalid, code_max=space - 1, key_filter=True)
    try:
        mode, nbytes = r.hash_table_filter(table)
        before = r.fprobe_jit_launches()
        res = r.filter_probe_cols(
            table, prog, [pc["f"]] + [pc[k] for k in pkeys],
            [(1 + i, mn, rg, False) for i, (mn, rg) in enumerate(ranges)],
            len(p), [pc["rid"], pc["x"], pc["nv"]], [bc["bv"], bc["bn"]])
        jit = r.fprobe_jit_launches() - before
    finally:
        r.hash_table_free(table)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if res is None:
        return None, mode, nbytes, jit
    got = _download(res[0], NAMES)
    assert res[1] == len(got)
    return got, mode, nbytes, jit


def _check(r, monkeypatch, p, b, interp, want_mode, env=None, **kw):
    """Filter on against the oracle and against filter off; returns the
    expected frame."""
    env = dict(env or {})
    if interp:
        env["DSX_DISABLE_JIT_FPROBE"] = "1"
    got, mode, nbytes, jit = _run(r, monkeypatch, p, b, env, **kw)
    off, off_mode, off_bytes, _ = _run(
        r, monkeypatch, p, b, dict(env, DSX_DISABLE_JOINFILTER="1"), **kw)
    assert mode == want_mode and (nbytes > 0) == (want_mode != NONE)
    assert (off_mode, off_bytes) == (NONE, 0)
    assert jit == (0 if interp or len(p) == 0 else 1)
    pk, bk = list(kw.get("pkeys", ("k",))), list(kw.get("bkeys", ("bk",)))
    exp = _oracle(p, b, _mask(p, kw.get("thresh", 50)), pk, bk, NAMES)
    assert (np.diff(got["rid"].to_numpy()) > 0).all()  # probe order kept
    assert_frame_close(got, _norm(exp), sort_by=["rid"])
    assert_frame_close(got, off, sort_by=["rid"])
    return exp


@KERNELS
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_probe_sizes_exact(runtime, monkeypatch, interp, n):
    rng = np.random.default_rng(n)
    p, b = _probe_frame(n, rng, null_keys=False), _build(rng)
    if n == 1:
        p["f"] = pd.array([0], dtype="Int64")  # the one row passes
        p["k"] = pd.array([int(b["bk"][5])], dtype="Int64")
    exp = _check(runtime, monkeypatch, p, b, interp, EXACT)
    assert len(exp) == 1 if n == 1 else 0 < len(exp) < n


@KERNELS
def test_nulls_and_range_ends(runtime, monkeypatch, interp):
    """NULL probe keys, NULL predicate values, NULL build keys; probe keys at
    the minimum and the maximum of the range, both of them build keys."""
    rng = np.random.default_rng(21)
    n = 4097
    p, b = _probe_frame(n, rng), _build(rng)
    p.loc[[0, 64, n - 1], "k"] = 0
    p.loc[[1, 63, n - 2], "k"] = KEY_RANGE - 1
    p.loc[[0, 1, 63, 64, n - 2, n - 1], "f"] = 0
    assert p["k"].isna().sum() > 0 and p["f"].isna().sum() > 0
    bk = pd.array(b["bk"], dtype="Int64")
    bk[10:60] = pd.NA  # 50 NULL build keys: never inserted, never matched
    b["bk"] = bk
    exp = _check(runtime, monkeypatch, p, b, interp, EXACT)
    assert {0, 1, 63, 64, n - 2, n - 1} <= set(exp["rid"])  # the range ends


@KERNELS
@pytest.mark.parametrize("density", ["none", "all"])
def test_match_density(runtime, monkeypatch, interp, density):
    rng = np.random.default_rng(22)
    n = 4097
    p, b = _probe_frame(n, rng, null_keys=False), _build(rng)
    absent = np.setdiff1d(np.arange(KEY_RANGE), b["bk"].to_numpy())
    pool = absent if density == "none" else b["bk"].to_numpy()
    p["k"] = pd.array(rng.choice(pool, n), dtype="Int64")
    p["f"] = pd.array(rng.integers(0, 100, n), dtype="Int64")  # no NULL
    exp = _check(runtime, monkeypatch, p, b, interp, EXACT, thresh=1000)
    assert len(exp) == (0 if density == "none" else n)


@KERNELS
def test_empty_build(runtime, monkeypatch, interp):
    rng = np.random.default_rng(23)
    p, b = _probe_frame(4097, rng), _build(rng, n=0)
    exp = _check(runtime, monkeypatch, p, b, interp, EXACT)
    assert len(exp) == 0


@KERNELS
def test_two_key_composite(runtime, monkeypatch, interp):
    rng = np.random.default_rng(24)
    n = 4097
    p = _probe_frame(n, rng)
    p["k"] = pd.array(rng.integers(0, 50, n), dtype="Int64")
    p.loc[rng.random(n) < 0.05, "k"] = pd.NA
    p["k2"] = rng.integers(0, 30, n).astype(np.int64)
    pairs = rng.permutation(50 * 30)[:N_BUILD]
    b = _build(rng)
    b["bk"] = (pairs // 30).astype(np.int64)
    b["bk2"] = (pairs % 30).astype(np.int64)
    exp = _check(runtime, monkeypatch, p, b, interp, EXACT,
                 pkeys=("k", "k2"), bkeys=("bk", "bk2"),
                 ranges=((0, 50), (0, 30)))
    assert 0 < len(exp) < n


@KERNELS
def test_hashed_packed_saturated(runtime, monkeypatch, interp):
    """64 bytes for 1 000 keys: the filter passes nearly everything."""
    rng = np.random.default_rng(25)
    p, b = _probe_frame(4097, rng), _build(rng)
    env = {"DSX_JOIN_FILTER_MAX_BYTES": "64", "DSX_JOIN_FILTER_MIN_BITS": "0"}
    exp = _check(runtime, monkeypatch, p, b, interp, HASHED, env=env)
    assert 0 < len(exp) < len(p)


@KERNELS
def test_hashed_unpacked(runtime, monkeypatch, interp):
    """Key range above 2^32: unpacked table, no exact bitmap possible."""
    rng = np.random.default_rng(26)
    n, big = 4097, 1 << 33
    p, b = _probe_frame(n, rng), _build(rng)
    far = rng.random(n) < 0.1
    p["k"] = pd.array(np.where(far, big, rng.integers(0, KEY_RANGE, n)),
                      dtype="Int64")
    p.loc[rng.random(n) < 0.05, "k"] = pd.NA
    b.loc[7, "bk"] = big
    exp = _check(runtime, monkeypatch, p, b, interp, HASHED,
                 ranges=((0, big + 1),))
    assert (exp["bv"] == b.loc[7, "bv"]).sum() > 0
    assert 0 < len(exp) < n


@KERNELS
def test_filter_dropped_under_a_small_cap(runtime, monkeypatch, interp):
    rng = np.random.default_rng(27)
    p, b = _probe_frame(4097, rng), _build(rng)
    exp = _check(runtime, monkeypatch, p, b, interp, NONE,
                 env={"DSX_JOIN_FILTER_MAX_BYTES": "64"})
    assert 0 < len(exp)


# ---------------------------------------------------------------------------
# SQL level
# ---------------------------------------------------------------------------
SQL = ("SELECT p.rid, p.k, p.x, p.nv, b.bk, b.bv, b.bn FROM p JOIN b "
       "ON p.k = b.bk WHERE p.f < 50")
SEL = ["rid", "k", "x", "nv", "bk", "bv", "bn"]


def _sql_on_off(monkeypatch, p, b, interp):
    """(filter on frame, prof, builds per mode, filter off frame)."""
    from dask_sql_amd.context import Context
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if interp:
        monkeypatch.setenv("DSX_DISABLE_JIT_FPROBE", "1")
    c = Context()
    c.create_table("p", p)
    c.create_table("b", b)
    r = c._get_runtime()
    r.prof_enable(True)
    r.prof_reset()
    before = r.join_filter_builds()
    got = c.sql(SQL).compute()
    prof = r.prof_get()
    builds = tuple(a - z for a, z in zip(r.join_filter_builds(), before))
    r.prof_enable(False)
    monkeypatch.setenv("DSX_DISABLE_JOINFILTER", "1")
    off = c.sql(SQL).compute()
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return got, prof, builds, off


@KERNELS
def test_sql_takes_the_fused_path_with_an_exact_filter(runtime, monkeypatch,
                                                       interp):
    rng = np.random.default_rng(28)
    p, b = _probe_frame(5000, rng), _build(rng)
    got, prof, builds, off = _sql_on_off(monkeypatch, p, b, interp)
    assert prof.get("k_fprobe_mask", {}).get("launches", 0) == 1
    assert prof.get("k_fprobe_emit", {}).get("launches", 0) == 1
    assert builds == (0, 1, 0)  # one filtered build, exact
    exp = _oracle(p, b, _mask(p, 50), ["k"], ["bk"], SEL)
    assert 0 < len(exp) < len(p)
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid"])


def test_other_joins_build_no_filter(runtime, monkeypatch):
    """Only a table that goes to the fused filter-probe asks for a filter: a
    join with no WHERE on its probe side, and hash_build's default, do not."""
    from dask_sql_amd.context import Context
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(30)
    p, b = _probe_frame(5000, rng), _build(rng)
    c = Context()
    c.create_table("p", p)
    c.create_table("b", b)
    r = c._get_runtime()
    before = r.join_filter_builds()
    for sql in ("SELECT p.rid, b.bv FROM p JOIN b ON p.k = b.bk",
                "SELECT p.rid, b.bv FROM p JOIN b ON p.k = b.bk "
                "WHERE b.bv >= 0",
                "SELECT p.rid, b.bv FROM p LEFT JOIN b ON p.k = b.bk "
                "WHERE p.f < 50"):
        assert len(c.sql(sql).compute()) > 0
    assert r.join_filter_builds() == before
    bcol = _upload(r, b["bk"])
    codes, space = r.keypack([bcol], [(0, 0, KEY_RANGE, False)], len(b))
    table = r.hash_build(codes, None, code_max=space - 1)
    try:
        assert r.hash_table_filter(table) == (NONE, 0)
    finally:
        r.hash_table_free(table)


@KERNELS
def test_duplicate_build_keys_fall_back(runtime, monkeypatch, interp):
    rng = np.random.default_rng(29)
    p, b = _probe_frame(5000, rng), _build(rng)
    b.loc[1, "bk"] = b.loc[0, "bk"]
    # entry level: not applicable, with the filter and without it
    for env in ({}, {"DSX_DISABLE_JOINFILTER": "1"}):
        if interp:
            env = dict(env, DSX_DISABLE_JIT_FPROBE="1")
        assert _run(runtime, monkeypatch, p, b, env)[0] is None
    # SQL level: the two-pass probe of the same table gives the same rows
    got, prof, builds, off = _sql_on_off(monkeypatch, p, b, interp)
    assert builds == (0, 1, 0)
    assert prof.get("k_fprobe_emit", {}).get("launches", 0) == 0
    assert prof.get("k_hash_probe_count", {}).get("launches", 0) == 1
    exp = _oracle(p, b, _mask(p, 50), ["k"], ["bk"], SEL)
    assert_frame_close(_norm(got), _norm(exp), sort_by=["rid", "bv"])
    assert_frame_close(_norm(got), _norm(off), sort_by=["rid", "bv"])
