"""The generated filter-probe mask kernel's source (dsx_jit_fprobe_source —
emission only, no HIP calls) on CPU: every supported shape emits source that
hipRTC compiles for gfx950 (dsx_jit_compile_check, no GPU needed), a rejected
predicate reports -1 instead of crashing, and the text — the compile-cache
key — depends on the shape alone (the entry never sees pointers or n)."""
import ctypes as ct

import pytest

from dask_sql_amd import runtime as rt

# VM opcodes (include/dsxhip.h DsxOp)
OP_COL, OP_LIT_I64 = 1, 3
OP_LT_I64, OP_GT_I64, OP_AND, OP_OR = 30, 32, 40, 41

REJECTED, TOO_SMALL, MALFORMED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    lib = rt._load_lib()
    lib.dsx_jit_fprobe_source.argtypes = [
        ct.POINTER(rt._Instr), ct.c_int, ct.POINTER(rt._KeySpec), ct.c_int,
        ct.POINTER(ct.c_int32), ct.POINTER(ct.c_uint8), ct.c_int, ct.c_int,
        ct.c_int, ct.c_char_p, ct.c_int64]
    lib.dsx_jit_fprobe_source.restype = ct.c_int
    lib.dsx_jit_compile_check.argtypes = [ct.c_char_p]
    lib.dsx_jit_compile_check.restype = ct.c_int
    return lib


def _source(lib, prog, keys, dtypes, has_validity, packed, words=0,
            cap=1 << 17):
    """(rc, source text or None); keys = [(col, min, range, nullable)]."""
    n = len(prog)
    arr = (rt._Instr * max(n, 1))()
    for i, (op, a0, imm) in enumerate(prog):
        arr[i].op, arr[i].arg0, arr[i].imm = op, a0, imm
    ks = (rt._KeySpec * len(keys))()
    for i, (ci, mn, rng, nullable) in enumerate(keys):
        ks[i].col, ks[i].min, ks[i].range = ci, mn, rng
        ks[i].nullable, ks[i].mode = (1 if nullable else 0), 0
    dt = (ct.c_int32 * len(dtypes))(*dtypes)
    hv = (ct.c_uint8 * len(dtypes))(*[1 if v else 0 for v in has_validity])
    buf = ct.create_string_buffer(cap)
    rc = lib.dsx_jit_fprobe_source(arr, n, ks, len(keys), dt, hv, len(dtypes),
                                   1 if packed else 0, words, buf, cap)
    return rc, (buf.value.decode() if rc == 0 else None)


DATE_GT = [(OP_COL, 0, 0), (OP_LIT_I64, 0, 9204), (OP_GT_I64, 0, 0)]
# (f < 50 AND g > 3) OR f < 2 over nullable f, g: Kleene AND/OR forms
KLEENE = [(OP_COL, 0, 0), (OP_LIT_I64, 0, 50), (OP_LT_I64, 0, 0),
          (OP_COL, 1, 0), (OP_LIT_I64, 0, 3), (OP_GT_I64, 0, 0),
          (OP_AND, 0, 0),
          (OP_COL, 0, 0), (OP_LIT_I64, 0, 2), (OP_LT_I64, 0, 0),
          (OP_OR, 0, 0)]

SHAPES = {
    # Q3 lineitem: i32 date > constant, one i64 key, packed table
    "one_key_i64_packed": dict(
        prog=DATE_GT, keys=[(1, 1, 60_000_000, False)],
        dtypes=[rt.I32, rt.I64], has_validity=[0, 0], packed=True),
    "composite_nullable_i32": dict(
        prog=DATE_GT, keys=[(1, 0, 50_000, False), (2, -7, 1000, True)],
        dtypes=[rt.I32, rt.I64, rt.I32], has_validity=[0, 0, 1],
        packed=True),
    "unpacked": dict(
        prog=DATE_GT, keys=[(1, 0, (1 << 33) + 1, True)],
        dtypes=[rt.I32, rt.I64], has_validity=[0, 1], packed=False),
    "kleene_nullable_predicate": dict(
        prog=KLEENE, keys=[(2, 0, 1500, False)],
        dtypes=[rt.I64, rt.I64, rt.I8], has_validity=[1, 1, 0], packed=True),
    "empty_predicate": dict(
        prog=[], keys=[(0, 0, 1500, False)],
        dtypes=[rt.I64], has_validity=[0], packed=True),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_emits_and_compiles(lib, name):
    rc, src = _source(lib, **SHAPES[name])
    assert rc == 0
    assert 'extern "C" __global__' in src and "j_fprobe_mask(" in src
    assert f"#define R {rt.FPROBE_JIT_WORDS}\n" in src  # the shipped unroll
    if name == "kleene_nullable_predicate":
        assert "C.validity[0][r]" in src and "C.validity[1][r]" in src
    if name == "composite_nullable_i32":
        assert "jit_key_valid" in src and "C.validity[2][r] != 0" in src
    assert ("(k[j] >> 32) == code[j]" in src) == SHAPES[name]["packed"]
    assert lib.dsx_jit_compile_check(src.encode()) == 0


@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_every_unroll_compiles(lib, words):
    rc, src = _source(lib, words=words, **SHAPES["composite_nullable_i32"])
    assert rc == 0 and f"#define R {words}\n" in src
    assert lib.dsx_jit_compile_check(src.encode()) == 0


def test_selftest(lib):
    lib.dsx_jit_fprobe_selftest.restype = ct.c_int
    assert lib.dsx_jit_fprobe_selftest() == 0


def test_rejected_predicate_reports_error(lib):
    shape = dict(SHAPES["one_key_i64_packed"])
    shape["prog"] = [(OP_COL, 0, 0), (9999, 0, 0)]  # no such opcode
    assert _source(lib, **shape) == (REJECTED, None)
    # a Kleene chain over nullable columns grows ~2.6x per level; past the
    # generator's size limit it is left to the interpreter kernel
    prog = [(OP_COL, 0, 0), (OP_LIT_I64, 0, 50), (OP_LT_I64, 0, 0)]
    for i in range(16):
        prog += [(OP_COL, i % 2, 0), (OP_LIT_I64, 0, i), (OP_GT_I64, 0, 0),
                 (OP_AND if i % 2 else OP_OR, 0, 0)]
    shape = dict(SHAPES["kleene_nullable_predicate"])
    shape["prog"] = prog
    assert _source(lib, **shape) == (REJECTED, None)


def test_malformed_spec_and_small_buffer(lib):
    shape = dict(SHAPES["one_key_i64_packed"])
    assert _source(lib, cap=64, **shape)[0] == TOO_SMALL
    shape["keys"] = [(5, 0, 10, False)]  # key column out of range
    assert _source(lib, **shape)[0] == MALFORMED
    shape = dict(SHAPES["one_key_i64_packed"])
    assert _source(lib, words=9, **shape)[0] == MALFORMED


def test_source_is_a_function_of_the_shape_only(lib):
    """Pointers, n and the table mask are kernel arguments: the entry takes
    only dtypes and validity PRESENCE, so two calls for one shape give one
    text (one compile-cache entry), and the text names no address."""
    a = _source(lib, **SHAPES["composite_nullable_i32"])[1]
    b = _source(lib, **SHAPES["composite_nullable_i32"])[1]
    assert a == b
    sig = a[a.index("j_fprobe_mask("):]
    sig = sig[:sig.index("{")]
    for arg in ("ColsArg C", "i64 n", "tkeys", "i64 tmask", "dup", "mask",
                "block_counts", "extra"):
        assert arg in sig
    # what does belong to the shape changes the text
    other = dict(SHAPES["composite_nullable_i32"], has_validity=[0, 0, 0])
    assert _source(lib, **other)[1] != a
    assert _source(lib, **dict(SHAPES["composite_nullable_i32"],
                               packed=False))[1] != a
