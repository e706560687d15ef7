"""CPU test of the group-by finish arithmetic (csrc/gb_finish.h), g++-compiled
behind a tiny main: key unpacking against Python integer arithmetic, and the
aggregate finalizers (NULL on count 0, MIN/MAX decodings, AVG against
Python's correctly rounded division)."""
import struct
import subprocess
import tempfile
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "dask_sql_amd" / "csrc"

MAIN = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "gb_finish.h"
// keys: argv = "keys" file nkeys {space min nullable mode}*nkeys
//       file = u64 codes; prints "valid bits" per code per key
// fin:  argv = "fin" file; file = u64 triples (kind, raw, count);
//       prints "valid bits" per triple
static uint64_t* slurp(const char* path, size_t* n) {
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint64_t* v = (uint64_t*)malloc(sz + 8);
  if (fread(v, 1, sz, f) != (size_t)sz) exit(2);
  fclose(f);
  *n = sz / 8;
  return v;
}
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  size_t n;
  uint64_t* v = slurp(argv[2], &n);
  if (argv[1][0] == 'k') {
    int nkeys = atoi(argv[3]);
    if (argc != 4 + 4 * nkeys || nkeys > 4) return 2;
    DsxGbKeyPlan plan[4];
    uint64_t stride = 1;  // as dsx_hash_groupby lays the keys out
    for (int j = 0; j < nkeys; j++) {
      uint64_t space = strtoull(argv[4 + 4 * j], 0, 10);
      int64_t mn = strtoll(argv[5 + 4 * j], 0, 10);
      int nullable = atoi(argv[6 + 4 * j]), mode = atoi(argv[7 + 4 * j]);
      plan[j] = dsx_gbf_key_plan(stride, space, mn, nullable, mode);
      if (mode == 0) stride *= space;
    }
    for (size_t i = 0; i < n; i++)
      for (int j = 0; j < nkeys; j++) {
        uint64_t bits;
        int valid = dsx_gbf_key_value(v[i], plan[j], &bits);
        printf("%d %llu\n", valid, (unsigned long long)bits);
      }
  } else {
    for (size_t i = 0; i + 3 <= n; i += 3) {
      uint64_t bits;
      int valid = dsx_gbf_finalize((int)v[i], v[i + 1], v[i + 2], &bits);
      printf("%d %llu\n", valid, (unsigned long long)bits);
    }
  }
  return 0;
}
"""

COUNT, SUM_I, SUM_F, MIN_I, MAX_I, MIN_F, MAX_F, AVG = range(8)
NAN_BITS = 0x7FF8000000000000
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def tool():
    with tempfile.TemporaryDirectory() as d:
        src = Path(d) / "gbf_main.cc"
        src.write_text(MAIN)
        exe = Path(d) / "gbf_main"
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                        f"-I{CSRC}", str(src), "-o", str(exe)], check=True)

        def run(mode, words, *args):
            data = Path(d) / "in.bin"
            np.asarray(words, dtype=np.uint64).tofile(data)
            out = subprocess.run(
                [str(exe), mode, str(data), *map(str, args)],
                check=True, capture_output=True, text=True).stdout.split()
            return [(int(out[i]), int(out[i + 1]))
                    for i in range(0, len(out), 2)]
        yield run


def _pack(keys, values):
    """pack_key's code of one row; values[j] None = NULL."""
    code, stride = 0, 1
    for (space, mn, nullable, _), v in zip(keys, values):
        if nullable:
            part = 0 if v is None else v - mn + 1
        else:
            part = v - mn
        assert 0 <= part < space
        code += part * stride
        stride *= space
    return code


def _check_keys(tool, keys, rows):
    codes = [_pack(keys, r) for r in rows]
    assert max(codes) < 1 << 62
    args = [len(keys)]
    for k in keys:
        args += list(k)
    out = tool("keys", codes, *args)
    it = iter(out)
    for r in rows:
        for (space, mn, nullable, _), v in zip(keys, r):
            valid, bits = next(it)
            if v is None:
                assert (valid, bits) == (0, 0)
            else:
                assert valid == 1
                assert bits == v & M64, (keys, r)


def _rows_for(keys, rng, n=200):
    """Random rows plus every corner (first, last, NULL) of every key."""
    def pick(k, how):
        space, mn, nullable, _ = k
        rng_ = space - (1 if nullable else 0)
        if how == "lo":
            return mn
        if how == "hi":
            return mn + rng_ - 1
        if how == "null" and nullable:
            return None
        if nullable and rng.random() < 0.2:
            return None
        return mn + int(rng.integers(0, rng_))
    rows = [[pick(k, how) for k in keys] for how in ("lo", "hi", "null")]
    for j in range(len(keys)):  # one key at a corner, the others random
        for how in ("lo", "hi", "null"):
            rows.append([pick(k, how if i == j else "rand")
                         for i, k in enumerate(keys)])
    rows += [[pick(k, "rand") for k in keys] for _ in range(n)]
    return rows


# (space, min, nullable, mode): space = range + nullable
KEYSETS = [
    [(1, 7, 0, 0)],                                   # space 1 alone
    [(1000, -499, 0, 0)],                             # odd-ish, negative min
    [(1024, 0, 0, 0)],                                # power of two
    [(5, -2, 1, 0)],                                  # nullable, NULL slot 0
    [(6_000_000, 1, 0, 0), (2406, 8035, 0, 0), (1, 0, 0, 0)],   # Q3's shape
    [(1, 0, 0, 0), (7, -3, 0, 0)],                    # space 1 first
    [(256, -128, 0, 0), (4096, 0, 1, 0)],             # pow2 stride and space
    [(3, 0, 1, 0), (17, -(1 << 40), 1, 0), (64, 5, 0, 0)],  # two nullable
    [(2, 0, 1, 0), (2, 0, 1, 0), (2, 0, 1, 0), (2, 0, 1, 0)],  # range-1 x4
    [(97, -1, 0, 0), (1 << 20, 0, 0, 0), (1, 3, 0, 0), (33, -16, 1, 0)],
    # products of space just under 2^62
    [((1 << 31) - 1, -(1 << 30), 0, 0), ((1 << 31) - 1, 0, 1, 0)],
    [(1 << 31, -5, 0, 0), (1 << 31, -(1 << 62), 0, 0)],
    [(2097143, 0, 0, 0), (2097143, -7, 1, 0), (1048573, 9, 0, 0)],
    [((1 << 62) - 1, -(1 << 61), 1, 0)],
    [(32749, 0, 0, 0), (32749, 0, 0, 0), (32749, -9, 1, 0), (131071, 1, 0, 0)],
]


@pytest.mark.parametrize("keys", KEYSETS,
                         ids=[f"k{i}" for i in range(len(KEYSETS))])
def test_key_unpack_matches_python_integers(tool, keys):
    prod = 1
    for k in keys:
        prod *= k[0]
    assert prod <= 1 << 62
    rng = np.random.default_rng(len(keys) * 1000 + keys[0][0] % 997)
    _check_keys(tool, keys, _rows_for(keys, rng))


def _f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_f64_bits_key(tool):
    vals = [0.0, 1.5, -1.5, 1e308, -5e-324, float("inf"), float("-inf")]
    codes = [0] + [_f64_bits(v) + 1 for v in vals]
    out = tool("keys", codes, 1, 1, 0, 1, 1)
    assert out[0] == (0, NAN_BITS)          # NaN / NULL share code 0
    assert out[1] == (1, 0)                 # the +0.0 code (−0.0 packs to it)
    for v, (valid, bits) in zip(vals, out[1:]):
        assert valid == 1 and bits == _f64_bits(v)


def _f64_ordered(x):
    b = _f64_bits(x)
    return (~b & M64) if b >> 63 else (b | (1 << 63))


def _fin(tool, triples):
    return tool("fin", [w & M64 for t in triples for w in t])


def test_count_zero_is_null_for_all_but_count(tool):
    out = _fin(tool, [(k, 12345, 0) for k in range(8)])
    assert out[COUNT] == (1, 0)
    for k in (SUM_I, MIN_I, MAX_I):
        assert out[k] == (0, 0)
    for k in (SUM_F, MIN_F, MAX_F, AVG):
        assert out[k] == (0, NAN_BITS)      # invalid f64 cells hold NaN


def test_count_one_and_decodings_at_negative_values(tool):
    ivals = [-(1 << 63), -7, -1, 0, 1, (1 << 63) - 1]
    fvals = [-1e300, -2.5, -0.0, 0.0, 5e-324, 3.25, float("-inf")]
    triples, exp = [], []
    for cnt in (1, 3):
        triples.append((COUNT, 999, cnt))
        exp.append((1, cnt))
        for v in ivals:
            triples.append((SUM_I, v, cnt))
            exp.append((1, v & M64))
            for k in (MIN_I, MAX_I):        # accumulators hold v ^ sign bit
                triples.append((k, (v & M64) ^ (1 << 63), cnt))
                exp.append((1, v & M64))
        for v in fvals:
            triples.append((SUM_F, _f64_bits(v), cnt))
            exp.append((1, _f64_bits(v)))
            for k in (MIN_F, MAX_F):        # accumulators hold f64_ordered
                triples.append((k, _f64_ordered(v), cnt))
                exp.append((1, _f64_bits(v)))
    assert _fin(tool, triples) == exp


def test_avg_is_correctly_rounded_division(tool):
    rng = np.random.default_rng(7)
    sums = np.concatenate([
        rng.integers(-(1 << 52), 1 << 52, 300).astype(np.float64),
        rng.standard_normal(300) * 1e6, [0.0, -0.0, 1.0, -1.0, 1e308]])
    counts = np.concatenate([rng.integers(1, 1 << 40, 300),
                             rng.integers(1, 10, 300), [1, 3, 3, 7, 3]])
    out = _fin(tool, [(AVG, _f64_bits(float(s)), int(c))
                      for s, c in zip(sums, counts)])
    for s, c, (valid, bits) in zip(sums, counts, out):
        assert valid == 1
        got = struct.unpack("<d", struct.pack("<Q", bits))[0]
        # Fraction → float rounds to nearest even: the correctly rounded
        # quotient of the two exact operands
        want = float(Fraction(float(s)) / int(c))
        assert got == want and (got != 0 or
                                _f64_bits(got) == _f64_bits(float(s) / int(c)))
