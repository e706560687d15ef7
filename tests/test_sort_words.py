"""CPU tests of the radix sort chain's host-side halves:

- plan_sort_words (dask_sql_amd/physical/sort_words.py): how an ORDER BY
  collation is cut into 64-bit words for dsx_sort_word;
- the float order code (csrc/sort_code.h), g++-compiled behind a tiny main
  and compared index for index with pandas' stable sort in all four
  DESC × NULLS combinations.
"""
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "dask_sql_amd" / "csrc" / "sort_code.h"

DESC, NULLS_LAST, FLOAT = 2, 4, 8


# ---------------------------------------------------------------------------
# plan_sort_words
# ---------------------------------------------------------------------------
def _ikey(col, rng=10, nullable=False, mode=0, mn=0):
    return (col, False, mn, rng, nullable, mode)


def _fkey(col, nullable=False, mode=0):
    return (col, True, 0, 0, nullable, mode)


def test_float_keys_get_their_own_words():
    from dask_sql_amd.physical.sort_words import plan_sort_words
    keys = [_ikey(0), _fkey(1, mode=DESC), _ikey(2), _ikey(3), _fkey(4)]
    words = plan_sort_words(keys)
    # least significant first: [f4] [i2,i3] [f1] [i0]
    assert [w.cols for w in words] == [(4,), (3, 2), (1,), (0,)]
    assert words[0].specs == ((0, 0, 0, False, FLOAT),)
    assert words[2].specs == ((0, 0, 0, False, DESC | FLOAT),)
    for w in words:
        floats = [s for s in w.specs if s[4] & FLOAT]
        assert not floats or len(w.specs) == 1


def test_five_integer_keys_split_4_plus_1():
    from dask_sql_amd.physical.sort_words import plan_sort_words
    keys = [_ikey(i, rng=10 + i) for i in range(5)]
    words = plan_sort_words(keys)
    assert [len(w.specs) for w in words] == [1, 4]
    # least significant word first: the 5th key alone, then keys 0..3
    assert words[0].cols == (4,)
    assert words[0].specs == ((0, 0, 14, False, 0),)
    # inside a word: reversed significance (key 3 on stride 1 ... key 0 top)
    assert words[1].cols == (3, 2, 1, 0)
    assert [s[2] for s in words[1].specs] == [13, 12, 11, 10]
    assert [s[0] for s in words[1].specs] == [0, 1, 2, 3]


def test_key_space_bound_splits_words():
    from dask_sql_amd.physical.sort_words import plan_sort_words
    r = 1 << 30
    words = plan_sort_words([_ikey(0, rng=r), _ikey(1, rng=r),
                             _ikey(2, rng=r)])
    # 2^30 * 2^30 = 2^60 fits, * 2^30 = 2^90 does not
    assert [w.cols for w in words] == [(2,), (1, 0)]
    # exactly 2^62 still fits one word ...
    words = plan_sort_words([_ikey(0, rng=1 << 31), _ikey(1, rng=1 << 31)])
    assert [len(w.specs) for w in words] == [2]
    # ... one more slot (a nullable key) does not
    words = plan_sort_words([_ikey(0, rng=1 << 31),
                             _ikey(1, rng=1 << 31, nullable=True)])
    assert [len(w.specs) for w in words] == [1, 1]
    for w in plan_sort_words([_ikey(i, rng=r, nullable=True)
                              for i in range(7)]):
        space = 1
        for _, _, rng, nullable, _ in w.specs:
            space *= rng + (1 if nullable else 0)
        assert space <= 1 << 62 and len(w.specs) <= 4


def test_column_indices_remap_on_a_wide_table():
    from dask_sql_amd.physical.sort_words import plan_sort_words
    # key on column 40 of a 50-column table, plus a second key on column 7
    words = plan_sort_words([_ikey(40, rng=100, nullable=True,
                                   mode=DESC | NULLS_LAST, mn=-5),
                             _ikey(7)])
    assert len(words) == 1
    (w,) = words
    assert w.cols == (7, 40)
    assert w.specs == ((0, 0, 10, False, 0),
                       (1, -5, 100, True, DESC | NULLS_LAST))
    assert all(0 <= s[0] < len(w.cols) for s in w.specs)
    # the same column twice is carried once
    (w,) = plan_sort_words([_ikey(40), _ikey(40, mode=DESC)])
    assert w.cols == (40,) and [s[0] for s in w.specs] == [0, 0]


def test_empty_collation_plans_nothing():
    from dask_sql_amd.physical.sort_words import plan_sort_words
    assert plan_sort_words([]) == []


def test_chain_of_words_equals_pandas_on_host():
    """Simulate the chain with numpy stable sorts on the words' codes: the
    plan's order and in-word key order reproduce pandas' key-by-key
    mergesort."""
    from dask_sql_amd.physical.sort_words import plan_sort_words
    rng = np.random.default_rng(5)
    n = 3000
    data = {i: rng.integers(0, 6, n) for i in range(6)}
    asc = [True, False, True, True, False, True]
    keys = [_ikey(i, rng=6, mode=0 if asc[i] else DESC) for i in range(6)]
    perm = np.arange(n)
    for w in plan_sort_words(keys):
        code = np.zeros(n, dtype=np.int64)
        stride = 1
        for local, mn, rg, _, mode in w.specs:
            v = data[w.cols[local]] - mn
            if mode & DESC:
                v = (rg - 1) - v
            code += v * stride
            stride *= rg
        perm = perm[np.argsort(code[perm], kind="stable")]
    df = pd.DataFrame({f"k{i}": data[i] for i in range(6)})
    exp = df
    for i in reversed(range(6)):
        exp = exp.sort_values(f"k{i}", ascending=asc[i], kind="mergesort")
    assert perm.tolist() == exp.index.tolist()


# ---------------------------------------------------------------------------
# float order code
# ---------------------------------------------------------------------------
MAIN = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "sort_code.h"
int main(int argc, char** argv) {
  int n = atoi(argv[1]), mode = atoi(argv[2]);
  FILE* f = fopen(argv[3], "rb");
  double* x = (double*)malloc(8 * (size_t)n);
  unsigned char* v = (unsigned char*)malloc((size_t)n);
  if (fread(x, 8, n, f) != (size_t)n) return 2;
  if (fread(v, 1, n, f) != (size_t)n) return 2;
  fclose(f);
  for (int i = 0; i < n; i++)
    printf("%llu\n", (unsigned long long)dsx_f64_order_code(x[i], v[i], mode));
  return 0;
}
"""


def _bits(u):
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


@pytest.fixture(scope="module")
def float_codes():
    assert HEADER.exists(), f"{HEADER} missing"
    td = Path(tempfile.mkdtemp(prefix="dsx_sortcode_"))
    (td / "main.cc").write_text(MAIN)
    exe = td / "sortcode"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                        f"-I{HEADER.parent}", str(td / "main.cc"), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]

    rng = np.random.default_rng(2024)
    dmax = np.finfo(np.float64).max
    edge = np.array([
        0.0, -0.0, np.inf, -np.inf,
        _bits(0x7FF8000000000000), _bits(0xFFF8000000000000),  # ±quiet NaN
        _bits(0x7FF0000000000001), _bits(0xFFF0000000000001),  # signalling
        _bits(0x7FFFFFFFFFFFFFFF), _bits(0xFFFFFFFFFFFFFFFF),  # full payload
        5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308,
        dmax, -dmax, 1.0, -1.0, 0.0, -0.0, 1.0, -1.0,
    ], dtype=np.float64)
    rand = np.concatenate([
        rng.standard_normal(4000) * 1e3,
        rng.integers(0, 2 ** 63, 4000, dtype=np.uint64).view(np.float64),
        -rng.random(1000), rng.random(1000) * 1e-310,
    ])
    x = np.concatenate([edge, rand])
    assert len(rand) == 10_000
    rng.shuffle(x)
    valid = (rng.random(len(x)) > 0.1).astype(np.uint8)
    data = td / "x.bin"
    with open(data, "wb") as f:
        f.write(x.astype("<f8").tobytes())
        f.write(valid.tobytes())

    def codes(mode):
        out = subprocess.run([str(exe), str(len(x)), str(mode), str(data)],
                             capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        return np.array([int(t) for t in out.stdout.split()],
                        dtype=np.uint64)

    return x, valid, codes


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("nulls_last", [False, True])
def test_float_code_order_equals_pandas(float_codes, desc, nulls_last):
    x, valid, codes = float_codes
    mode = FLOAT | (DESC if desc else 0) | (NULLS_LAST if nulls_last else 0)
    code = codes(mode)
    got = np.lexsort((np.arange(len(x)), code))  # by (code, index)
    col = pd.Series(np.where(valid.astype(bool), x, np.nan))
    exp = col.sort_values(kind="mergesort", ascending=not desc,
                          na_position="last" if nulls_last else "first")
    assert got.tolist() == exp.index.tolist()


@pytest.mark.parametrize("mode", [8, 10, 12, 14])
def test_float_code_zero_signs_tie_and_null_slot(float_codes, mode):
    x, valid, codes = float_codes
    code = codes(mode)
    ok = valid.astype(bool)
    zeros = ok & (x == 0.0)
    assert np.signbit(x[zeros]).any() and (~np.signbit(x[zeros])).any()
    assert len(set(code[zeros].tolist())) == 1
    slot = np.uint64(0xFFFFFFFFFFFFFFFF) if mode & NULLS_LAST else np.uint64(0)
    null = ~ok | np.isnan(x)
    assert (code[null] == slot).all()
    assert (code[~null] != slot).all()
    # real values never reach either end of the code space
    assert (code[~null] != np.uint64(0)).all()
    assert (code[~null] != np.uint64(0xFFFFFFFFFFFFFFFF)).all()
