"""The per-shape generated mask kernel of dsx_filter_probe_cols against the
interpreter kernel it replaces (-m gpu).

Every case runs runtime.filter_probe_cols twice in one process — generated
kernel, then DSX_DISABLE_JIT_FPROBE=1 — and asserts through
runtime.fprobe_jit_launches() that each run used the intended variant. Both
fill the same match mask, so the two outputs must be equal exactly, row order
included; the generated kernel's output is also compared with the pandas
oracle join over the filtered probe rows."""
import numpy as np
import pandas as pd
import pytest

from dask_sql_amd import runtime as rt
from tests.conftest import assert_frame_close
from tests.test_gpu_filter_probe import (_build_frame, _download, _launches,
                                         _mask, _norm, _oracle, _probe_frame)

pytestmark = pytest.mark.gpu

KNOB = "DSX_DISABLE_JIT_FPROBE"
W = 64 * rt.FPROBE_JIT_WORDS  # rows per wave iteration of the generated kernel
OP_COL, OP_LIT_I64, OP_LT_I64 = 1, 3, 30
_NP = {rt.I8: np.int8, rt.I32: np.int32, rt.I64: np.int64}


@pytest.fixture(scope="module")
def r():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dask_sql_amd.context import Context
    return Context()._get_runtime()


def _dev(r, s, dtype=None):
    """Upload a series; a nullable one gets a validity buffer. `dtype`
    narrows an integer column to I8/I32."""
    if pd.api.types.is_extension_array_dtype(s.dtype):
        d = rt.I64 if dtype is None else dtype
        valid = (~s.isna()).to_numpy().astype(np.uint8)
        return r.upload_column(s.fillna(0).to_numpy(dtype=_NP[d]),
                               valid if len(s) else None, d)
    arr = np.ascontiguousarray(s.to_numpy())
    if dtype is not None:
        arr = arr.astype(_NP[dtype])
    return r.upload_column(arr)


def _lt(col, lit):
    return rt.Runtime.make_prog([(OP_COL, col, 0), (OP_LIT_I64, 0, lit),
                                 (OP_LT_I64, 0, 0)])


def _both(r, monkeypatch, table, prog, cols, specs, n, pcols, bcols, names):
    """[generated-kernel frame, interpreter frame] (None: not applicable)."""
    out = []
    r.prof_enable(True)
    try:
        for jit in (True, False):
            if jit:
                monkeypatch.delenv(KNOB, raising=False)
            else:
                monkeypatch.setenv(KNOB, "1")
            before = r.fprobe_jit_launches()
            r.prof_reset()
            res = r.filter_probe_cols(table, prog, cols, specs, n, pcols,
                                      bcols)
            used = r.fprobe_jit_launches() - before
            assert used == (1 if jit and n > 0 else 0), (jit, used)
            assert _launches(r.prof_get(), "k_fprobe_mask") == (
                1 if n > 0 else 0)
            if res is None:
                out.append(None)
                continue
            frame = _download(res[0], names)
            assert res[1] == len(frame)
            out.append(frame)
    finally:
        monkeypatch.delenv(KNOB, raising=False)
        r.prof_enable(False)
    return out


def _table(r, bcols_dev, specs, n_build):
    codes, space = r.keypack(bcols_dev, specs, n_build)
    return r.hash_build(codes, None, code_max=space - 1)


def _check(got, off, exp):
    pd.testing.assert_frame_equal(got, off, check_exact=True)
    assert (np.diff(got["rid"].to_numpy()) > 0).all()  # probe row order
    assert_frame_close(got, _norm(exp), sort_by=["rid"])


# ---------------------------------------------------------------------------
# word and tail handling: nullable predicate column, nullable i64 key with
# NULLs, packed table
# ---------------------------------------------------------------------------
def _sizes(w):
    """Row counts around one wave iteration (w rows) and one block iteration
    (4 waves), without repeats."""
    return list(dict.fromkeys(
        [0, 1, 63, 64, 65, w - 1, w, w + 1, 4 * w - 1, 4 * w + 1]))


@pytest.mark.parametrize("n", _sizes(W) + [
    100_003,
    524_353,  # 8 193 words over the 2 048-block cap, 5 per block: the
              # trailing blocks are idle and take the round-up path
])
def test_row_counts(r, monkeypatch, n):
    _row_count_case(r, monkeypatch, n)


@pytest.mark.parametrize("words,n", [
    (w, n) for w in (2, 4, 8) if w != rt.FPROBE_JIT_WORDS
    for n in _sizes(64 * w)[5:] + [20_011]])
def test_row_counts_other_unroll_factors(r, monkeypatch, words, n):
    """The generator's R is a parameter (DSX_FPROBE_R re-measures it): the
    factors that do not ship fill the same mask."""
    monkeypatch.setenv("DSX_FPROBE_R", str(words))
    _row_count_case(r, monkeypatch, n)


def _row_count_case(r, monkeypatch, n):
    rng = np.random.default_rng(300 + n)
    p = _probe_frame(n, rng)[["rid", "k", "f", "x", "nv"]]
    b = _build_frame(rng)[["bk", "bv", "bn"]]
    pc = {c: _dev(r, p[c]) for c in p.columns}
    bc = {c: _dev(r, b[c]) for c in b.columns}
    table = _table(r, [bc["bk"]], [(0, 0, 1500, False)], len(b))
    names = ["rid", "x", "nv", "bv", "bn"]
    try:
        got, off = _both(r, monkeypatch, table, _lt(0, 50),
                         [pc["f"], pc["k"]], [(1, 0, 1500, False)], n,
                         [pc["rid"], pc["x"], pc["nv"]],
                         [bc["bv"], bc["bn"]], names)
    finally:
        r.hash_table_free(table)
    exp = _oracle(p, b, _mask(p, 50), ["k"], ["bk"], names)
    if n >= 1000:
        assert 0 < len(exp) < n
    _check(got, off, exp)


# ---------------------------------------------------------------------------
# shapes, at a size of several blocks with a ragged tail
# ---------------------------------------------------------------------------
N = 20_011


def _plain_probe(rng, n, key_lo, key_hi, key_np=np.int64):
    """No validity anywhere: d32 is the predicate column."""
    return pd.DataFrame({
        "rid": np.arange(n, dtype=np.int64),
        "k": rng.integers(key_lo, key_hi, n).astype(key_np),
        "d32": rng.integers(0, 10_000, n).astype(np.int32),
        "x": rng.random(n),
    })


def _plain_build(rng, keys):
    return pd.DataFrame({
        "bk": np.asarray(keys, dtype=np.int64),
        "bv": rng.integers(0, 1 << 40, len(keys)).astype(np.int64),
    })


def _run_plain(r, monkeypatch, p, b, thresh, key_dtype, mn, rng_):
    pc = {"rid": _dev(r, p["rid"]), "x": _dev(r, p["x"]),
          "d32": _dev(r, p["d32"]), "k": _dev(r, p["k"], key_dtype)}
    bc = {c: _dev(r, b[c]) for c in b.columns}
    table = _table(r, [bc["bk"]], [(0, mn, rng_, False)], len(b))
    names = ["rid", "x", "bk", "bv"]
    try:
        got, off = _both(r, monkeypatch, table, _lt(0, thresh),
                         [pc["d32"], pc["k"]], [(1, mn, rng_, False)], len(p),
                         [pc["rid"], pc["x"]], [bc["bk"], bc["bv"]], names)
    finally:
        r.hash_table_free(table)
    p64 = p.assign(k=p["k"].astype(np.int64))
    exp = _oracle(p64, b, (p["d32"] < thresh).to_numpy(), ["k"], ["bk"],
                  names)
    _check(got, off, exp)
    return exp


@pytest.mark.parametrize("key_dtype,lo,hi", [
    (rt.I8, -128, 128), (rt.I32, -70_000, 70_000), (rt.I64, 0, 1500)])
def test_key_dtypes_without_validity(r, monkeypatch, key_dtype, lo, hi):
    rng = np.random.default_rng(400 + key_dtype)
    p = _plain_probe(rng, N, lo, hi, _NP[key_dtype])
    keys = lo + rng.permutation(hi - lo)[:min(1000, (hi - lo) // 2)]
    exp = _run_plain(r, monkeypatch, p, _plain_build(rng, keys), 5000,
                     key_dtype, lo, hi - lo)
    assert 0 < len(exp) < N


@pytest.mark.parametrize("thresh,n_exp", [(-1, "none"), (10_001, "all")])
def test_predicate_passes_none_or_all(r, monkeypatch, thresh, n_exp):
    rng = np.random.default_rng(410)
    p = _plain_probe(rng, N, 0, 1500)
    exp = _run_plain(r, monkeypatch, p,
                     _plain_build(rng, rng.permutation(1500)[:1000]), thresh,
                     rt.I64, 0, 1500)
    assert (len(exp) == 0) if n_exp == "none" else (len(exp) > N // 2)


@pytest.mark.parametrize("present", [True, False])
def test_every_or_no_probe_key_present(r, monkeypatch, present):
    rng = np.random.default_rng(420)
    p = _plain_probe(rng, N, 0, 1000)
    keys = np.arange(1000) if present else np.arange(1000, 2000)
    exp = _run_plain(r, monkeypatch, p, _plain_build(rng, keys), 5000,
                     rt.I64, 0, 2000)
    assert len(exp) == (int((p["d32"] < 5000).sum()) if present else 0)


def test_longest_chains_build_of_2_15_keys(r, monkeypatch):
    """2^15 unique build keys → 65 536 slots at load factor exactly 0.5."""
    rng = np.random.default_rng(430)
    p = _plain_probe(rng, 50_021, 0, 1 << 16)
    keys = rng.permutation(1 << 16)[:1 << 15]
    exp = _run_plain(r, monkeypatch, p, _plain_build(rng, keys), 5000,
                     rt.I64, 0, 1 << 16)
    assert 0 < len(exp) < len(p)


def test_unpacked_layout(r, monkeypatch):
    """code_max ≥ 2^32: (code, row id) no longer share one table word."""
    rng = np.random.default_rng(440)
    big = 1 << 33
    p = _probe_frame(N, rng)[["rid", "k", "f", "x"]]
    far = rng.random(N) < 0.1
    p["k"] = pd.array(np.where(far, big, rng.integers(0, 1500, N)),
                      dtype="Int64")
    p.loc[rng.random(N) < 0.05, "k"] = pd.NA
    b = _build_frame(rng)[["bk", "bv"]]
    b.loc[0, "bk"] = big  # replaces one key, still unique
    pc = {c: _dev(r, p[c]) for c in p.columns}
    bc = {c: _dev(r, b[c]) for c in b.columns}
    spec = (0, big + 1, False)
    table = _table(r, [bc["bk"]], [(0,) + spec], len(b))
    names = ["rid", "x", "bk", "bv"]
    try:
        got, off = _both(r, monkeypatch, table, _lt(0, 50),
                         [pc["f"], pc["k"]], [(1,) + spec], N,
                         [pc["rid"], pc["x"]], [bc["bk"], bc["bv"]], names)
    finally:
        r.hash_table_free(table)
    exp = _oracle(p, b, _mask(p, 50), ["k"], ["bk"], names)
    assert (exp["bk"] == big).sum() > 0
    _check(got, off, exp)


def test_composite_key_with_nullable_i32(r, monkeypatch):
    rng = np.random.default_rng(450)
    p = _probe_frame(N, rng)[["rid", "f", "x"]]
    p["k"] = pd.array(rng.integers(0, 50, N), dtype="Int64")
    p.loc[rng.random(N) < 0.05, "k"] = pd.NA
    p["k2"] = rng.integers(0, 40, N).astype(np.int64)
    pairs = rng.permutation(50 * 40)[:1000]
    b = pd.DataFrame({"bk": (pairs // 40).astype(np.int64),
                      "bk2": (pairs % 40).astype(np.int64),
                      "bv": rng.integers(0, 1 << 40, 1000).astype(np.int64)})
    pc = {"rid": _dev(r, p["rid"]), "f": _dev(r, p["f"]),
          "x": _dev(r, p["x"]), "k": _dev(r, p["k"], rt.I32),
          "k2": _dev(r, p["k2"])}
    bc = {c: _dev(r, b[c]) for c in b.columns}
    table = _table(r, [bc["bk"], bc["bk2"]],
                   [(0, 0, 50, False), (1, 0, 40, False)], len(b))
    names = ["rid", "x", "bk", "bk2", "bv"]
    try:
        got, off = _both(r, monkeypatch, table, _lt(0, 50),
                         [pc["f"], pc["k"], pc["k2"]],
                         [(1, 0, 50, False), (2, 0, 40, False)], N,
                         [pc["rid"], pc["x"]],
                         [bc["bk"], bc["bk2"], bc["bv"]], names)
    finally:
        r.hash_table_free(table)
    exp = _oracle(p, b, _mask(p, 50), ["k", "k2"], ["bk", "bk2"], names)
    assert 0 < len(exp) < N
    _check(got, off, exp)


def test_duplicate_build_keys_not_applicable(r, monkeypatch):
    rng = np.random.default_rng(460)
    p = _plain_probe(rng, N, 0, 1500)
    keys = rng.permutation(1500)[:1000]
    keys[1] = keys[0]
    b = _plain_build(rng, keys)
    pc = {c: _dev(r, p[c]) for c in p.columns}
    bc = {c: _dev(r, b[c]) for c in b.columns}
    table = _table(r, [bc["bk"]], [(0, 0, 1500, False)], len(b))
    try:
        got, off = _both(r, monkeypatch, table, _lt(0, 5000),
                         [pc["d32"], pc["k"]], [(1, 0, 1500, False)], N,
                         [pc["rid"]], [bc["bv"]], ["rid", "bv"])
    finally:
        r.hash_table_free(table)
    assert got is None and off is None


# ---------------------------------------------------------------------------
# SQL level
# ---------------------------------------------------------------------------
def test_q3_mini_runs_generated_kernel(r, monkeypatch):
    from dask_sql_amd.context import Context
    from datagen import Q3_SQL, gen_q3, register_q3_tables
    from oracle.tpch import oracle_q3
    cust, orders, li = gen_q3(sf_rows=(1_500, 15_000, 60_000))
    c = Context()
    register_q3_tables(c, cust, orders, li)
    rq = c._get_runtime()
    monkeypatch.delenv(KNOB, raising=False)
    monkeypatch.delenv("DSX_DISABLE_FILTERPROBE", raising=False)
    before = rq.fprobe_jit_launches()
    out = c.sql(Q3_SQL).compute()
    assert rq.fprobe_jit_launches() - before == 2  # orders and lineitem
    monkeypatch.setenv(KNOB, "1")
    off = c.sql(Q3_SQL).compute()
    assert rq.fprobe_jit_launches() - before == 2
    exp = oracle_q3(cust, orders, li)
    assert len(out) == len(exp) == len(off)
    for got in (out, off):
        assert (got["l_orderkey"].to_numpy().astype(np.int64)
                == exp["l_orderkey"].to_numpy()).all()
        days = got["o_orderdate"].to_numpy().astype("datetime64[D]").astype(
            np.int64)
        assert (days == exp["o_orderdate"].to_numpy()).all()
    assert np.allclose(out["revenue"], exp["revenue"], rtol=1e-9)
