"""CPU test of the join key-membership filter's bit arithmetic
(csrc/join_filter.h), g++-compiled behind a tiny main that builds a filter
from a file of member codes and answers a file of queries.

Exact mode: a set bit is a member and nothing else. Hashed mode (blocked
two-bit Bloom filter: one 32-bit word per key, two distinct bits in it): no
false negative, and a false-positive rate under 1.5 x the analytic two-bit
value (1 - e^(-2n/B))^2 — a blocked layout sits a little above it, because
the keys of one word share 32 bits instead of the whole array.

Measured with this header (seeds below, 200 000 non-members):
  10.49 bits/key (n = 100 000, B = 2^20): 0.0340 against 0.0302 analytic
   5.24 bits/key (n = 200 000, B = 2^20): 0.1063 against 0.1006 analytic"""
import math
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "dask_sql_amd" / "csrc"

MAIN = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "join_filter.h"
// argv: mode arg n_members n_queries file(u64 members, then u64 queries)
// prints: the filter's words (exact mode only), then one 0/1 per query
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  int mode = atoi(argv[1]);
  uint64_t arg = strtoull(argv[2], 0, 10);
  size_t nm = strtoull(argv[3], 0, 10), nq = strtoull(argv[4], 0, 10);
  uint64_t* v = (uint64_t*)malloc(8 * (nm + nq + 1));
  FILE* f = fopen(argv[5], "rb");
  if (!f || fread(v, 8, nm + nq, f) != nm + nq) return 2;
  fclose(f);
  size_t words = mode == DSX_JF_EXACT ? dsx_jf_exact_words(arg) : arg + 1;
  uint32_t* w = (uint32_t*)calloc(words, 4);
  for (size_t i = 0; i < nm; i++) {
    if (mode == DSX_JF_EXACT) {
      w[dsx_jf_exact_word(v[i])] |= dsx_jf_exact_bit(v[i]);
    } else {
      uint64_t h = dsx_jf_mix64(v[i]);
      w[dsx_jf_hashed_word(h, arg)] |= dsx_jf_hashed_bits(h);
    }
  }
  if (mode == DSX_JF_EXACT) {
    printf("%zu\n", words);
    for (size_t i = 0; i < words; i++) printf("%u\n", w[i]);
  }
  for (size_t i = nm; i < nm + nq; i++) {
    int hit;
    if (mode == DSX_JF_EXACT) {
      hit = v[i] <= arg &&
            (w[dsx_jf_exact_word(v[i])] & dsx_jf_exact_bit(v[i])) != 0;
    } else {
      uint64_t h = dsx_jf_mix64(v[i]);
      uint32_t b = dsx_jf_hashed_bits(h);
      if (__builtin_popcount(b) != 2) return 3;  // two DISTINCT bits
      hit = (w[dsx_jf_hashed_word(h, arg)] & b) == b;
    }
    printf("%d\n", hit);
  }
  return 0;
}
"""

EXACT, HASHED = 1, 2


@pytest.fixture(scope="module")
def tool():
    with tempfile.TemporaryDirectory() as d:
        src = Path(d) / "jf_main.cc"
        src.write_text(MAIN)
        exe = Path(d) / "jf_main"
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                        f"-I{CSRC}", str(src), "-o", str(exe)], check=True)

        def run(mode, arg, members, queries):
            data = Path(d) / "in.bin"
            np.concatenate([np.asarray(members, dtype=np.uint64),
                            np.asarray(queries, dtype=np.uint64)]).tofile(data)
            out = subprocess.run(
                [str(exe), str(mode), str(arg), str(len(members)),
                 str(len(queries)), str(data)],
                check=True, capture_output=True, text=True).stdout.split()
            return np.array(out, dtype=np.int64)
        yield run


def test_exact_bits_are_the_members_and_nothing_else(tool):
    code_max = 1498  # 1499 codes: not a multiple of 32
    rng = np.random.default_rng(1)
    members = np.unique(np.concatenate(
        [[0, code_max], rng.integers(0, code_max + 1, 400)]))
    queries = np.arange(0, code_max + 40)  # past code_max: a miss, no read
    out = tool(EXACT, code_max, members, queries)
    words = int(out[0])
    assert words == (code_max + 1 + 31) // 32 == 47  # whole 32-bit words
    w = out[1:1 + words].astype(np.uint32)
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    exp = np.zeros(words * 32, dtype=np.uint8)
    exp[members] = 1
    assert (bits == exp).all()
    hit = out[1 + words:]
    assert (hit == np.isin(queries, members)).all()


@pytest.mark.parametrize("n_members", [
    100_000,   # 2^20 bits: 10.49 bits/key
    200_000,   # 2^20 bits:  5.24 bits/key
])
def test_hashed_no_false_negative_and_fp_rate(tool, n_members):
    nbits = 1 << 20
    rng = np.random.default_rng(n_members)
    # members and non-members from disjoint halves of a sparse code space
    members = np.unique(rng.integers(0, 1 << 40, n_members)) * 2
    non = np.unique(rng.integers(0, 1 << 40, 200_000)) * 2 + 1
    probe_members = members[:100_000]
    out = tool(HASHED, nbits // 32 - 1, members,
               np.concatenate([probe_members, non]))
    assert (out[:len(probe_members)] == 1).all()  # no false negative
    fp = out[len(probe_members):].mean()
    analytic = (1.0 - math.exp(-2.0 * len(members) / nbits)) ** 2
    print(f"bits/key {nbits / len(members):.2f}: fp {fp:.4f}, "
          f"analytic {analytic:.4f}")
    assert fp < 1.5 * analytic
    assert fp > 0.5 * analytic  # a filter that rejects everything is broken


def test_dense_codes_hash_as_well_as_random_ones(tool):
    """Join codes are key - min: consecutive integers, not random ones."""
    nbits = 1 << 17
    members = np.arange(0, 2 * 12_500, 2)  # 10.49 bits/key
    non = np.arange(1, 2 * 100_000, 2)
    out = tool(HASHED, nbits // 32 - 1, members,
               np.concatenate([members, non]))
    assert (out[:len(members)] == 1).all()
    analytic = (1.0 - math.exp(-2.0 * len(members) / nbits)) ** 2
    assert out[len(members):].mean() < 1.5 * analytic
