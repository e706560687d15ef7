"""CPU tests of csrc/win_range.h, the host/device arithmetic of
dsx_window_range: the saturating key + offset add, the two binary searches
over a sorted order key, and the split of a frame into loose rows and
sparse-table entries. The header is g++-compiled behind a tiny main (-Wall
-Werror) and compared with numpy.
"""
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

HEADER = (Path(__file__).resolve().parent.parent / "dask_sql_amd" / "csrc"
          / "win_range.h")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "win_range.h"

// search <kind> <desc> <nkeys> <ntargets> <file>: keys then targets in the
// file; per target "lower upper" over the whole key array
template <class K>
static int run_search(int desc, long nk, long nt, FILE* f) {
  std::vector<K> key(nk), t(nt);
  if (nk && fread(key.data(), sizeof(K), nk, f) != (size_t)nk) return 3;
  if (nt && fread(t.data(), sizeof(K), nt, f) != (size_t)nt) return 3;
  for (long i = 0; i < nt; i++)
    printf("%lld %lld\n",
           (long long)dsx_win_lower<K>(key.data(), 0, nk, t[i], desc),
           (long long)dsx_win_upper<K>(key.data(), 0, nk, t[i], desc));
  return 0;
}

// sat <n> <file>: pairs (k, off) → k + off saturated
static int run_sat(long n, FILE* f) {
  for (long i = 0; i < n; i++) {
    int64_t kv[2];
    if (fread(kv, 8, 2, f) != 2) return 3;
    int ovf;
    int64_t r = dsx_win_sat_add_ovf(kv[0], kv[1], &ovf);
    if (r != dsx_win_sat_add(kv[0], kv[1])) return 4;
    // value, overflow side, and the four "bound admits no row" answers
    printf("%lld %d %d %d %d %d\n", (long long)r, ovf,
           dsx_win_low_none(ovf, 0), dsx_win_low_none(ovf, 1),
           dsx_win_high_none(ovf, 0), dsx_win_high_none(ovf, 1));
  }
  return 0;
}

// split <limit>: every 0 <= s <= e < limit
static int run_split(long limit) {
  for (long s = 0; s < limit; s++)
    for (long e = s; e < limit; e++) {
      DsxWinRmqSplit r = dsx_win_rmq_split(s, e);
      printf("%ld %ld %lld %lld %lld %lld %d %lld %lld\n", s, e,
             (long long)r.head_end, (long long)r.tail_begin, (long long)r.b0,
             (long long)r.b1, r.level, (long long)r.left, (long long)r.right);
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 7 && !strcmp(argv[1], "search")) {
    FILE* f = fopen(argv[6], "rb");
    if (!f) return 2;
    int desc = atoi(argv[3]);
    long nk = atol(argv[4]), nt = atol(argv[5]);
    int rc = !strcmp(argv[2], "f64") ? run_search<double>(desc, nk, nt, f)
                                     : run_search<int64_t>(desc, nk, nt, f);
    fclose(f);
    return rc;
  }
  if (argc == 4 && !strcmp(argv[1], "sat")) {
    FILE* f = fopen(argv[3], "rb");
    if (!f) return 2;
    int rc = run_sat(atol(argv[2]), f);
    fclose(f);
    return rc;
  }
  if (argc == 3 && !strcmp(argv[1], "split")) return run_split(atol(argv[2]));
  if (argc == 3 && !strcmp(argv[1], "levels")) {
    printf("%d\n", dsx_win_rmq_levels(atol(argv[2])));
    return 0;
  }
  return 1;
}
"""

I64_MAX = np.iinfo(np.int64).max
I64_MIN = np.iinfo(np.int64).min


@pytest.fixture(scope="module")
def exe():
    assert HEADER.exists(), f"{HEADER} missing"
    td = Path(tempfile.mkdtemp(prefix="dsx_winrange_"))
    (td / "main.cc").write_text(MAIN)
    out = td / "win_range"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                        f"-I{HEADER.parent}", str(td / "main.cc"), "-o",
                        str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]
    return out


def _run(exe, *args):
    out = subprocess.run([str(exe), *map(str, args)], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    return out.stdout


def _search(exe, kind, desc, keys, targets):
    path = exe.parent / "search.bin"
    path.write_bytes(np.ascontiguousarray(keys).tobytes()
                     + np.ascontiguousarray(targets).tobytes())
    rows = np.array(_run(exe, "search", kind, int(desc), len(keys),
                         len(targets), path).split(), dtype=np.int64)
    return rows.reshape(-1, 2)


def _expect(keys, targets, desc):
    """numpy.searchsorted over the ascending view."""
    n = len(keys)
    if not desc:
        return np.stack([np.searchsorted(keys, targets, "left"),
                         np.searchsorted(keys, targets, "right")], axis=1)
    asc = keys[::-1]
    return np.stack([n - np.searchsorted(asc, targets, "right"),
                     n - np.searchsorted(asc, targets, "left")], axis=1)


def _key_sets_i64():
    rng = np.random.default_rng(1)
    yield np.sort(rng.integers(-50, 50, 300)).astype(np.int64)   # duplicates
    yield np.full(37, 12, dtype=np.int64)                        # all equal
    yield np.array([5], dtype=np.int64)                          # one row
    yield np.zeros(0, dtype=np.int64)                            # no row
    yield np.arange(-64, 64, dtype=np.int64)                     # unique
    yield np.array([I64_MIN, I64_MIN, -1, 0, I64_MAX - 1, I64_MAX],
                   dtype=np.int64)


@pytest.mark.parametrize("desc", [False, True])
def test_int_searches_match_searchsorted(exe, desc):
    for keys in _key_sets_i64():
        lo = int(keys.min()) if len(keys) else 0
        hi = int(keys.max()) if len(keys) else 0
        targets = np.unique(np.concatenate([
            keys, keys[keys < I64_MAX] + 1, keys[keys > I64_MIN] - 1,
            # below and above every key
            np.array([max(lo, I64_MIN + 7) - 7, min(hi, I64_MAX - 7) + 7,
                      I64_MIN, I64_MAX], dtype=np.int64)]))
        k = keys[::-1].copy() if desc else keys
        got = _search(exe, "i64", desc, k, targets)
        assert (got == _expect(k, targets, desc)).all(), (keys[:8], desc)


@pytest.mark.parametrize("desc", [False, True])
def test_float_searches_match_searchsorted(exe, desc):
    rng = np.random.default_rng(2)
    sets = [np.sort(rng.integers(-40, 40, 200) / 4.0),
            np.array([-np.inf, -1.5, -0.0, 0.0, 0.0, 2.25, np.inf]),
            np.full(9, 0.5), np.array([1e300])]
    for keys in sets:
        targets = np.unique(np.concatenate([
            keys, keys + 0.25, keys - 0.25,
            np.array([-np.inf, np.inf, -1e308, 1e308, -0.0, 0.0])]))
        k = keys[::-1].copy() if desc else keys
        got = _search(exe, "f64", desc, k, targets)
        assert (got == _expect(k, targets, desc)).all(), (keys[:8], desc)


def test_saturating_add(exe):
    ks = [I64_MAX, I64_MAX - 1, I64_MAX - 100, 1, 0, -1, I64_MIN + 100,
          I64_MIN + 1, I64_MIN]
    offs = [0, 1, -1, 100, -100, I64_MAX, -I64_MAX, I64_MAX - 1]
    pairs = np.array([(k, o) for k in ks for o in offs], dtype=np.int64)
    path = exe.parent / "sat.bin"
    path.write_bytes(pairs.tobytes())
    rows = np.array(_run(exe, "sat", len(pairs), path).split(),
                    dtype=object).reshape(-1, 6)
    got = [int(t) for t in rows[:, 0]]
    exact = [int(k) + int(o) for k, o in pairs]
    want = [min(max(x, I64_MIN), I64_MAX) for x in exact]
    assert got == want
    # which limit the exact sum lies beyond, and when a bound is left
    # without any row: the low bound (keys at or after the target) when the
    # target lies beyond the far end of the sort direction, the high bound
    # (keys at or before it) when it lies before the near end
    ovf = [(x > I64_MAX) - (x < I64_MIN) for x in exact]
    assert [int(t) for t in rows[:, 1]] == ovf
    assert [int(t) for t in rows[:, 2]] == [int(o == 1) for o in ovf]
    assert [int(t) for t in rows[:, 3]] == [int(o == -1) for o in ovf]
    assert [int(t) for t in rows[:, 4]] == [int(o == -1) for o in ovf]
    assert [int(t) for t in rows[:, 5]] == [int(o == 1) for o in ovf]
    assert 1 in ovf and -1 in ovf
    # both limits are reached from both kinds of operand
    assert I64_MAX in want and I64_MIN in want


def test_levels(exe):
    for blocks in (1, 2, 3, 4, 63, 64, 65, 79, 1 << 20, (1 << 20) + 1):
        assert int(_run(exe, "levels", blocks)) == blocks.bit_length()


def test_split_covers_every_frame_exactly(exe):
    """Brute force for every 0 <= s <= e < 400: the head rows, the two
    table entries and the tail rows cover every row of [s, e] and none
    outside; loose runs hold at most 63 rows once there is a whole block;
    a frame wider than the direct-loop limit always has one."""
    limit = 400
    rows = np.array(_run(exe, "split", limit).split(), dtype=np.int64) \
        .reshape(-1, 9)
    assert len(rows) == limit * (limit + 1) // 2
    s, e, head_end, tail_begin, b0, b1, level, left, right = rows.T
    pos = np.arange(limit + 64)[None, :]

    def span(a, b):            # rows a..b inclusive → boolean coverage
        return (pos >= a[:, None]) & (pos <= b[:, None])

    has = b1 >= b0
    width = np.int64(1) << level
    ent_l = span(left * 64, (left + width) * 64 - 1) & has[:, None]
    ent_r = span(right * 64, (right + width) * 64 - 1) & has[:, None]
    cover = span(s, head_end) | span(tail_begin, e) | ent_l | ent_r
    assert (cover == span(s, e)).all()
    # the entries are whole blocks inside the frame, the loose runs short
    assert (left[has] == b0[has]).all()
    assert (right[has] + width[has] - 1 == b1[has]).all()
    assert (right[has] >= left[has]).all()
    assert (right[has] <= left[has] + width[has]).all()      # no gap
    assert ((head_end - s + 1)[has] <= 63).all()
    assert ((e - tail_begin + 1)[has] <= 63).all()
    assert has[(e - s + 1) > 128].all()
