"""CPU tests of csrc/topk_select.h, the host/device arithmetic of
dsx_topk_rows: the order code of the primary ORDER BY key and the digit pick
of the MSB-first radix select. The header is g++-compiled behind a tiny main
(-Wall -Werror) and compared with numpy.
"""
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

HEADER = (Path(__file__).resolve().parent.parent / "dask_sql_amd" / "csrc"
          / "topk_select.h")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "topk_select.h"

// codes <kind> <desc> <n> <file>: one line per value, the code or "na"
static int run_codes(const char* kind, int desc, long n, const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  for (long i = 0; i < n; i++) {
    uint64_t code = 0;
    int ok = 1;
    if (!strcmp(kind, "f64")) {
      double x;
      if (fread(&x, 8, 1, f) != 1) return 3;
      ok = dsx_topk_code_f64(x, desc, &code);
    } else if (!strcmp(kind, "i64")) {
      int64_t x;
      if (fread(&x, 8, 1, f) != 1) return 3;
      code = dsx_topk_code_i64(x, desc);
    } else if (!strcmp(kind, "i32")) {
      int32_t x;
      if (fread(&x, 4, 1, f) != 1) return 3;
      code = dsx_topk_code_i64(x, desc);
    } else {
      int8_t x;
      if (fread(&x, 1, 1, f) != 1) return 3;
      code = dsx_topk_code_i64(x, desc);
    }
    if (ok) printf("%llu\n", (unsigned long long)code);
    else printf("na\n");
  }
  fclose(f);
  return 0;
}

// chain <file>: cases of (n, k, cap, codes[n]) as u64 words. Runs the select
// the way dsx_topk_rows does: per pass the histogram of the rows inside the
// prefix, dsx_topk_pick, stop at "done"; then the emit predicate and the
// trim. Prints: status(1 selected / 2 not applicable) end_pass emitted kept
// sum(idx+1) sum((idx+1)^2) over the kept rows.
static int run_chain(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  uint64_t hdr[3];
  while (fread(hdr, 8, 3, f) == 3) {
    long n = (long)hdr[0];
    uint32_t k = (uint32_t)hdr[1], cap = (uint32_t)hdr[2];
    std::vector<uint64_t> codes(n);
    if (fread(codes.data(), 8, n, f) != (size_t)n) return 3;
    uint64_t prefix = 0;
    uint32_t want = k, taken = 0;
    int status = 2, end_pass = -1;
    for (int p = 0; p < DSX_TOPK_PASSES; p++) {
      std::vector<uint32_t> hist(DSX_TOPK_BINS, 0);
      for (long i = 0; i < n; i++)
        if (dsx_topk_in_prefix(codes[i], prefix, p))
          hist[dsx_topk_digit(codes[i], p)]++;
      uint32_t before;
      int done;
      int b = dsx_topk_pick(hist.data(), DSX_TOPK_BINS, want, taken, cap,
                            &before, &done);
      prefix |= (uint64_t)b << dsx_topk_shift(p);
      want -= before;
      taken += before;
      end_pass = p;
      if (done) {
        status = 1;
        break;
      }
    }
    unsigned long long emitted = 0, kept = 0, s1 = 0, s2 = 0;
    if (status == 1) {
      std::vector<uint64_t> cand;
      std::vector<long> idx;
      for (long i = 0; i < n; i++)
        if (dsx_topk_at_or_before(codes[i], prefix, end_pass)) {
          cand.push_back(codes[i]);
          idx.push_back(i);
        }
      emitted = cand.size();
      std::vector<uint8_t> keep(cand.size());
      kept = dsx_topk_trim(cand.data(), (int64_t)cand.size(), k, keep.data());
      for (size_t j = 0; j < cand.size(); j++)
        if (keep[j]) {
          unsigned long long v = (unsigned long long)idx[j] + 1;
          s1 += v;
          s2 += v * v;
        }
    }
    printf("%d %d %llu %llu %llu %llu\n", status, end_pass, emitted, kept, s1,
           s2);
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "codes"))
    return run_codes(argv[2], atoi(argv[3]), atol(argv[4]), argv[5]);
  if (argc == 3 && !strcmp(argv[1], "chain")) return run_chain(argv[2]);
  return 1;
}
"""


@pytest.fixture(scope="module")
def exe():
    assert HEADER.exists(), f"{HEADER} missing"
    td = Path(tempfile.mkdtemp(prefix="dsx_topk_"))
    (td / "main.cc").write_text(MAIN)
    out = td / "topk"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                        f"-I{HEADER.parent}", str(td / "main.cc"), "-o",
                        str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]
    return out


def _codes(exe, kind, desc, arr):
    path = exe.parent / f"vals_{kind}_{int(desc)}.bin"
    path.write_bytes(np.ascontiguousarray(arr).tobytes())
    out = subprocess.run([str(exe), "codes", kind, str(int(desc)),
                          str(len(arr)), str(path)], capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    toks = out.stdout.split()
    assert len(toks) == len(arr)
    return toks


def _check_order(vals, codes, desc):
    """code order == value order: for every pair, code_a < code_b exactly
    when a sorts strictly before b, and equal codes exactly on equal values."""
    codes = np.array([int(t) for t in codes], dtype=np.uint64)
    order = np.argsort(codes, kind="stable")
    v, c = vals[order], codes[order]
    before = (v[:-1] > v[1:]) if desc else (v[:-1] < v[1:])
    assert ((c[:-1] < c[1:]) == before).all()
    assert ((c[:-1] == c[1:]) == (v[:-1] == v[1:])).all()


@pytest.mark.parametrize("desc", [False, True])
def test_f64_code_order(exe, desc):
    rng = np.random.default_rng(7)
    tiny = np.finfo(np.float64).tiny
    special = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, tiny / 4,
                        -tiny / 4, 5e-324, -5e-324, 1.0, -1.0, 1e308, -1e308,
                        np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0)])
    x = np.concatenate([special, rng.standard_normal(3000) * 1e6,
                        -np.abs(rng.standard_normal(500)) * 1e-300,
                        rng.integers(-5, 5, 500).astype(np.float64)])
    toks = _codes(exe, "f64", desc, x)
    assert "na" not in toks
    _check_order(x, toks, desc)
    # the two zeros tie
    assert toks[0] == toks[1]


def test_f64_nan_is_reported_not_coded(exe):
    x = np.array([1.0, np.nan, -np.nan, 2.0])
    for desc in (False, True):
        toks = _codes(exe, "f64", desc, x)
        assert [t == "na" for t in toks] == [False, True, True, False]


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("kind", ["i64", "i32", "i8"])
def test_int_code_order(exe, kind, desc):
    rng = np.random.default_rng(11)
    dt = {"i64": np.int64, "i32": np.int32, "i8": np.int8}[kind]
    info = np.iinfo(dt)
    x = np.concatenate([
        np.array([info.min, info.max, info.min + 1, info.max - 1, 0, -1, 1],
                 dtype=dt),
        rng.integers(info.min, info.max, 3000, dtype=dt, endpoint=True),
        rng.integers(-3, 3, 200).astype(dt)])
    toks = _codes(exe, kind, desc, x)
    assert "na" not in toks
    _check_order(x, toks, desc)


SHIFTS = [53, 42, 31, 20, 9, 0]


def _gen_cases(ncases=2000, seed=2024):
    rng = np.random.default_rng(seed)
    cases = []
    for ci in range(ncases):
        n = int(rng.integers(1, 5001))
        k = int(rng.integers(1, n + 1))
        kind = ci % 5
        if kind == 0:    # all distinct (random 64-bit codes)
            codes = rng.integers(0, 2**64, n, dtype=np.uint64)
        elif kind == 1:  # all equal
            codes = np.full(n, rng.integers(0, 2**64, dtype=np.uint64),
                            dtype=np.uint64)
        elif kind == 2:  # few values, spread over all digits
            vals = rng.integers(0, 2**64, int(rng.integers(2, 9)),
                                dtype=np.uint64)
            codes = vals[rng.integers(0, len(vals), n)]
        elif kind == 3:  # differ only in the lowest 8 bits: every pass runs
            base = rng.integers(0, 2**64, dtype=np.uint64) & ~np.uint64(0xFF)
            codes = base | rng.integers(0, 256, n).astype(np.uint64)
        else:            # few values that differ in one middle digit
            base = rng.integers(0, 2**64, dtype=np.uint64)
            sh = np.uint64(SHIFTS[int(rng.integers(0, 6))])
            codes = base ^ (rng.integers(0, 4, n).astype(np.uint64) << sh)
        s = np.sort(codes)
        exact = int((codes <= s[k - 1]).sum())
        pick = int(rng.integers(0, 5))
        cap = [exact, max(1, exact - 1), exact + int(rng.integers(1, 50)),
               int(rng.integers(1, n + 1)), 4 * k][pick]
        cases.append((n, k, cap, codes))
    return cases


def test_digit_pick_chain(exe):
    cases = _gen_cases()
    path = exe.parent / "cases.bin"
    with open(path, "wb") as f:
        for n, k, cap, codes in cases:
            f.write(np.array([n, k, cap], dtype=np.uint64).tobytes())
            f.write(codes.tobytes())
    out = subprocess.run([str(exe), "chain", str(path)], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    n_sel = n_na = n_early = 0
    for (n, k, cap, codes), line in zip(cases, lines):
        status, end_pass, emitted, kept, s1, s2 = (int(t) for t in
                                                   line.split())
        kth = np.sort(codes)[k - 1]
        exact = codes <= kth
        # rows at or before the k-th row's bucket after each pass: bucket +
        # taken. The select stops at the first pass where they fit the cap.
        sizes = [int(((codes >> np.uint64(s)) <= (kth >> np.uint64(s))).sum())
                 for s in SHIFTS]
        fits = [p for p, sz in enumerate(sizes) if sz <= cap]
        assert sizes[-1] == int(exact.sum())
        if int(exact.sum()) > cap:
            assert not fits
            assert status == 2, (n, k, cap)
            n_na += 1
            continue
        assert status == 1, (n, k, cap)
        assert end_pass == fits[0], (n, k, cap, end_pass, fits)
        assert emitted == sizes[end_pass]
        idx = np.nonzero(exact)[0].astype(object) + 1
        assert kept == len(idx)
        assert s1 == int(sum(idx)) % 2**64
        assert s2 == int(sum(i * i for i in idx)) % 2**64
        n_sel += 1
        n_early += end_pass < len(SHIFTS) - 1
    # the generator reaches all three ends
    assert n_sel > 200 and n_na > 200 and n_early > 100
    assert n_sel - n_early > 100
