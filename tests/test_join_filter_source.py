"""The generated filter-probe mask kernel with a key-membership filter
(dsx_jit_fprobe_source_mode — emission only, no HIP calls) on CPU: all three
filter modes emit source that hipRTC compiles for gfx950, for the packed
single-key shape and for the two-key shape; the text depends on the shape and
the mode alone (the entry never sees a pointer, a size or the byte cap); and
mode 0 is dsx_jit_fprobe_source's text, character for character."""
import ctypes as ct

import pytest

from dask_sql_amd import runtime as rt

OP_COL, OP_LIT_I64, OP_GT_I64 = 1, 3, 32
NONE, EXACT, HASHED = 0, 1, 2
MALFORMED = -3

DATE_GT = [(OP_COL, 0, 0), (OP_LIT_I64, 0, 9204), (OP_GT_I64, 0, 0)]
SHAPES = {
    "one_key_packed": dict(
        keys=[(1, 1, 60_000_000, False)], dtypes=[rt.I32, rt.I64],
        has_validity=[0, 0], packed=True),
    "two_keys": dict(
        keys=[(1, 0, 50_000, False), (2, -7, 1000, True)],
        dtypes=[rt.I32, rt.I64, rt.I32], has_validity=[0, 0, 1],
        packed=True),
    "two_keys_unpacked": dict(
        keys=[(1, 0, 1 << 33, False), (2, -7, 1000, True)],
        dtypes=[rt.I32, rt.I64, rt.I32], has_validity=[0, 1, 1],
        packed=False),
}


@pytest.fixture(scope="module")
def lib():
    lib = rt._load_lib()
    head = [ct.POINTER(rt._Instr), ct.c_int, ct.POINTER(rt._KeySpec),
            ct.c_int, ct.POINTER(ct.c_int32), ct.POINTER(ct.c_uint8),
            ct.c_int, ct.c_int, ct.c_int]
    lib.dsx_jit_fprobe_source_mode.argtypes = head + [
        ct.c_int, ct.c_char_p, ct.c_int64]
    lib.dsx_jit_fprobe_source_mode.restype = ct.c_int
    lib.dsx_jit_fprobe_source.argtypes = head + [ct.c_char_p, ct.c_int64]
    lib.dsx_jit_fprobe_source.restype = ct.c_int
    lib.dsx_jit_compile_check.argtypes = [ct.c_char_p]
    lib.dsx_jit_compile_check.restype = ct.c_int
    return lib


def _source(lib, keys, dtypes, has_validity, packed, mode, words=0):
    """(rc, text); mode None calls the entry without a mode."""
    arr = (rt._Instr * len(DATE_GT))()
    for i, (op, a0, imm) in enumerate(DATE_GT):
        arr[i].op, arr[i].arg0, arr[i].imm = op, a0, imm
    ks = (rt._KeySpec * len(keys))()
    for i, (ci, mn, rng, nullable) in enumerate(keys):
        ks[i].col, ks[i].min, ks[i].range = ci, mn, rng
        ks[i].nullable, ks[i].mode = (1 if nullable else 0), 0
    dt = (ct.c_int32 * len(dtypes))(*dtypes)
    hv = (ct.c_uint8 * len(dtypes))(*has_validity)
    cap = 1 << 17
    buf = ct.create_string_buffer(cap)
    head = (arr, len(DATE_GT), ks, len(keys), dt, hv, len(dtypes),
            1 if packed else 0, words)
    if mode is None:
        rc = lib.dsx_jit_fprobe_source(*head, buf, cap)
    else:
        rc = lib.dsx_jit_fprobe_source_mode(*head, mode, buf, cap)
    return rc, (buf.value.decode() if rc == 0 else None)


@pytest.mark.parametrize("mode", [NONE, EXACT, HASHED])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_mode_emits_and_compiles(lib, name, mode):
    rc, src = _source(lib, mode=mode, **SHAPES[name])
    assert rc == 0
    assert "j_fprobe_mask(" in src
    sig = src[src.index("j_fprobe_mask("):]
    sig = sig[:sig.index("{")]
    body = src[src.index("j_fprobe_mask("):]
    assert ("jf_arg" in sig) == (mode != NONE)
    if mode == EXACT:  # no table in the mask pass at all
        assert "tkeys[" not in body and "dsx_jf_exact_word" in body
    if mode == HASHED:  # the filter word comes before the first slot
        assert body.index("jf[fw[j]]") < body.index("tkeys[s[j]]")
        assert "dsx_jf_hashed_bits" in body
    if mode == NONE:
        assert "dsx_jf_" not in src
    assert lib.dsx_jit_compile_check(src.encode()) == 0


@pytest.mark.parametrize("mode", [EXACT, HASHED])
def test_wider_unroll_compiles(lib, mode):
    rc, src = _source(lib, mode=mode, words=4, **SHAPES["two_keys"])
    assert rc == 0 and "#define R 4\n" in src
    assert lib.dsx_jit_compile_check(src.encode()) == 0


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mode_0_is_the_unfiltered_text(lib, name):
    assert _source(lib, mode=NONE, **SHAPES[name]) == \
        _source(lib, mode=None, **SHAPES[name])


def test_text_depends_on_shape_and_mode_only(lib, monkeypatch):
    shape = SHAPES["one_key_packed"]
    texts = {m: _source(lib, mode=m, **shape)[1] for m in (NONE, EXACT, HASHED)}
    assert len(set(texts.values())) == 3
    # the cap decides which mode a table gets, never the text of a mode
    monkeypatch.setenv("DSX_JOIN_FILTER_MAX_BYTES", "64")
    monkeypatch.setenv("DSX_DISABLE_JOINFILTER", "1")
    for m, text in texts.items():
        assert _source(lib, mode=m, **shape)[1] == text
    # the filter's pointer and its code_max / word mask are kernel arguments
    for m in (EXACT, HASHED):
        sig = texts[m][texts[m].index("j_fprobe_mask("):]
        sig = sig[:sig.index("{")]
        assert "const u32* __restrict__ jf" in sig and "u64 jf_arg" in sig


def test_unknown_mode_is_malformed(lib):
    assert _source(lib, mode=3, **SHAPES["one_key_packed"])[0] == MALFORMED
    assert _source(lib, mode=-1, **SHAPES["one_key_packed"])[0] == MALFORMED
