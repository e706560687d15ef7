"""RANGE window frames with value offsets: the bound model, the offset
units, the output-dtype rule and a numpy host model. Pure Python and numpy:
no GPU, no library load.

Semantics are the SQL standard's as sqlite implements them. Rows of a
partition are sorted by the ORDER BY keys (NULLs last in both directions
unless the query says NULLS FIRST). For a row with order key ``k`` and
direction sign ``d`` (+1 ASC, -1 DESC) a bound carries a signed offset
(``a PRECEDING`` is ``-a``, ``b FOLLOWING`` is ``+b``):

- offset bound, non-NULL ``k``: the frame holds the non-NULL-key rows ``j``
  of the partition with ``lo <= d * (key[j] - k) <= hi``; ``k + offset``
  saturates at the int64 limits, and where the exact sum lies beyond the
  limit on the side that no key can reach, the bound admits no row (a key
  AT the limit does not tie with the saturated target);
- offset bound, NULL ``k``: that side ends at the edge of the row's peer
  group (the NULL block);
- CURRENT ROW: the peer group's first row (low side) / last row (high side);
- UNBOUNDED: the partition edge;
- an empty frame is NULL for every function except COUNT, which is 0.

The device twin is dsx_window_range (csrc/window_range.inc); the plugin
falls back to ``range_frames_host`` for what the device declines.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Union

import numpy as np

# what the builder validated and resolved (planner/range_frame.py)
from dask_sql_amd.planner.range_frame import (  # noqa: F401
    INT64_MAX, INT64_MIN, RANGE_AGGS, RANGE_FUNCS, RANGE_POSITIONAL)

UNBOUNDED, CURRENT, OFFSET = 0, 1, 2


class RangeBound(NamedTuple):
    kind: int                       # UNBOUNDED | CURRENT | OFFSET
    value: Union[int, float] = 0    # signed offset in the key's unit


def frame_bounds(frame):
    """Resolved ``("range", lo, hi)`` → ``(RangeBound, RangeBound)`` with
    signed offsets (PRECEDING negative)."""
    _, lo, hi = frame

    def one(b):
        side, v = b
        if side.startswith("unbounded"):
            return RangeBound(UNBOUNDED, 0)
        if side == "current":
            return RangeBound(CURRENT, 0)
        return RangeBound(OFFSET, -v if side == "preceding" else v)

    return one(lo), one(hi)


def range_can_be_empty(lo: RangeBound, hi: RangeBound) -> bool:
    """True iff some row's frame can hold no row: it starts after the
    current row's key, ends before it, or is an inverted offset pair."""
    if lo.kind == OFFSET and lo.value > 0:
        return True
    if hi.kind == OFFSET and hi.value < 0:
        return True
    return lo.kind == OFFSET and hi.kind == OFFSET and lo.value > hi.value


def range_out_dtype(func, lo, hi, plan_is_bigint, value_nullable):
    """Static output type → ``(kind, with_validity)``, kind in ``"i64" |
    "f64" | "value"``. COUNT is int64 without validity (an empty frame
    counts 0). SUM/MIN/MAX are int64 without validity for a BIGINT plan
    type over a value column without a validity buffer when the frame
    cannot be empty; otherwise float64 with validity. FIRST/LAST keep the
    value column's dtype, with validity."""
    if func in RANGE_POSITIONAL:
        return "value", True
    if func not in RANGE_AGGS:
        raise ValueError(f"window function {func} with a RANGE frame")
    if func == "count":
        return "i64", False
    if func in ("sum", "min", "max") and plan_is_bigint \
            and not value_nullable and not range_can_be_empty(lo, hi):
        return "i64", False
    return "f64", True


def needs_rmq(func, lo: RangeBound, hi: RangeBound) -> bool:
    """MIN/MAX with both sides bounded is served by the sparse table; every
    other shape by the per-partition scans."""
    return func in ("min", "max") and lo.kind != UNBOUNDED \
        and hi.kind != UNBOUNDED


def rmq_table_bytes(n: int) -> int:
    """Pool bytes of the device sparse table over n sorted rows: one f64
    per 64-row block and level, floor(log2(blocks)) + 1 levels (level j
    entry i covers blocks [i, i + 2^j))."""
    blocks = max(1, (n + 63) // 64)
    levels = blocks.bit_length()
    return 8 * blocks * levels


def rmq_max_bytes() -> int:
    """DSX_WIN_RANGE_RMQ_MAX_BYTES as dsx_window_range reads it, per call:
    the largest table a frame may take from the pool (default 1 GiB)."""
    try:
        v = int(os.environ.get("DSX_WIN_RANGE_RMQ_MAX_BYTES", ""))
        if v >= 0:
            return v
    except ValueError:
        pass
    return 1 << 30


# ---- host model ---------------------------------------------------------------
def sat_add(k: np.ndarray, off: int) -> np.ndarray:
    """int64 ``k + off`` saturating at the int64 limits."""
    k = np.asarray(k, dtype=np.int64)
    off = max(min(int(off), INT64_MAX), -INT64_MAX)
    if off >= 0:
        room = np.int64(INT64_MAX - off)
        return np.where(k > room, np.int64(INT64_MAX),
                        np.minimum(k, room) + np.int64(off))
    room = np.int64(INT64_MIN - off)
    return np.where(k < room, np.int64(INT64_MIN),
                    np.maximum(k, room) + np.int64(off))


def sat_overflow(k: np.ndarray, off: int) -> np.ndarray:
    """Which limit the exact ``k + off`` lies beyond: +1 above INT64_MAX,
    -1 below INT64_MIN, 0 when it fits."""
    k = np.asarray(k, dtype=np.int64)
    off = max(min(int(off), INT64_MAX), -INT64_MAX)
    if off >= 0:
        return (k > np.int64(INT64_MAX - off)).astype(np.int64)
    return -(k < np.int64(INT64_MIN - off)).astype(np.int64)


def dense_ids(cols) -> np.ndarray:
    """Dense int64 ids of the rows of ``[(array, valid_or_None), ...]``:
    two rows share an id iff they are equal on every column, NULL equal to
    NULL (and NaN a NULL, -0.0 equal to +0.0)."""
    n = len(cols[0][0]) if cols else 0
    ids = np.zeros(n, dtype=np.int64)
    for arr, valid in cols:
        ids = _combine(ids, _codes(arr, valid)[0])
    return ids


def _codes(arr, valid):
    """Dense value ranks (0..m-1 in ascending value order) with NULLs at
    code m → ``(codes, m)``."""
    arr = np.asarray(arr)
    ok = np.ones(len(arr), dtype=bool) if valid is None \
        else np.asarray(valid, dtype=bool).copy()
    if arr.dtype.kind == "f":
        ok &= ~np.isnan(arr)
    uniq, inv = np.unique(arr[ok], return_inverse=True)
    codes = np.full(len(arr), len(uniq), dtype=np.int64)
    codes[ok] = inv.reshape(-1)
    return codes, len(uniq)


def _combine(a, b):
    if len(a) == 0:
        return a
    width = int(b.max()) + 1
    _, inv = np.unique(a * width + b, return_inverse=True)
    return inv.reshape(-1).astype(np.int64)


def _rmq(vals, s, e, op):
    """op-reduction of vals[s[i] .. e[i]] (inclusive, s <= e) by a sparse
    table built up to the widest frame."""
    out = np.empty(len(s), dtype=vals.dtype)
    if len(s) == 0:
        return out
    length = e - s + 1
    lvl = np.zeros(len(s), dtype=np.int64)
    nz = length > 1
    lvl[nz] = np.floor(np.log2(length[nz])).astype(np.int64)
    # log2 rounding near powers of two
    lvl[(np.int64(1) << lvl) > length] -= 1
    lvl[(np.int64(2) << lvl) <= length] += 1
    table = vals
    for j in range(int(lvl.max()) + 1):
        if j:
            half = 1 << (j - 1)
            table = op(table[:-half], table[half:])
        m = lvl == j
        if m.any():
            out[m] = op(table[s[m]], table[e[m] - (1 << j) + 1])
    return out


def range_frames_host(func, pid, order, value, value_valid, lo: RangeBound,
                      hi: RangeBound, out_kind: str):
    """RANGE frames over plain arrays → ``(out, validity_or_None)`` in
    original row order.

    ``pid``: int partition id per row. ``order``: one ``(key, valid_or_None,
    desc, nulls_first)`` per ORDER BY key (exactly one when a bound is an
    OFFSET; its value is in the key's unit, int for integer keys and float
    for float keys). ``value`` / ``value_valid``: the operand (None for
    COUNT(*)). ``out_kind``: ``"i64"``, ``"f64"`` or ``"value"`` as
    range_out_dtype answers; validity is returned for the latter two."""
    if func not in RANGE_FUNCS:
        raise ValueError(f"window function {func} with a RANGE frame")
    pid = np.asarray(pid, dtype=np.int64)
    n = len(pid)
    offset = lo.kind == OFFSET or hi.kind == OFFSET
    if offset and len(order) != 1:
        raise ValueError("a RANGE frame with an offset needs exactly one "
                         "ORDER BY key")
    if n == 0:
        dt = {"i64": np.int64, "f64": np.float64}.get(out_kind) or \
            np.asarray(value).dtype
        return np.zeros(0, dtype=dt), \
            (None if out_kind == "i64" else np.zeros(0, dtype=np.uint8))
    # ---- stable sort by (partition, order keys) ------------------------------
    sort_cols = []
    for key, valid, desc, nulls_first in order:
        codes, m = _codes(key, valid)
        isnull = codes == m
        c = -codes if desc else codes
        c = np.where(isnull, -(m + 1) if nulls_first else m + 1, c)
        sort_cols.append(c)
    perm = np.lexsort(tuple(reversed([pid] + sort_cols))) if n else \
        np.zeros(0, dtype=np.int64)
    ps = pid[perm]
    head = np.ones(n, dtype=bool)
    head[1:] = ps[1:] != ps[:-1]
    peer_head = head.copy()
    for c in sort_cols:
        cs = c[perm]
        peer_head[1:] |= cs[1:] != cs[:-1]
    p_starts = np.flatnonzero(head)
    p_ends = np.r_[p_starts[1:], n]
    f_starts = np.flatnonzero(peer_head)
    f_len = np.diff(np.r_[f_starts, n])
    f0 = np.repeat(f_starts, f_len)
    f1 = f0 + np.repeat(f_len, f_len)                 # exclusive
    p_len = p_ends - p_starts
    p0 = np.repeat(p_starts, p_len)
    p1 = np.repeat(p_ends, p_len)

    # ---- frame bounds (inclusive sorted positions) ---------------------------
    s = p0.copy() if lo.kind == UNBOUNDED else f0.copy()
    e = (p1 - 1) if hi.kind == UNBOUNDED else (f1 - 1)
    if offset and n:
        key, valid, desc, _nf = order[0]
        key = np.asarray(key)
        fkey = key.dtype.kind == "f"
        kvalid = np.ones(n, dtype=bool) if valid is None \
            else np.asarray(valid, dtype=bool).copy()
        if fkey:
            kvalid &= ~np.isnan(key)
            ks = key.astype(np.float64)[perm]
        else:
            ks = key.astype(np.int64)[perm]
        nn = kvalid[perm]
        for a0, b0 in zip(p_starts, p_ends):
            idx = a0 + np.flatnonzero(nn[a0:b0])      # contiguous block
            if idx.size == 0:
                continue
            a, b = idx[0], idx[-1] + 1
            x = ks[a:b]
            asc_x = x[::-1] if desc else x

            def target(off):
                """Search target and, for integer keys, which int64 limit
                the exact k + off lies beyond (+1, -1, 0)."""
                off = -off if desc else off
                if fkey:
                    return x + float(off), np.zeros(len(x), dtype=np.int64)
                return sat_add(x, off), sat_overflow(x, off)

            # a target beyond an int64 limit admits every key (the
            # saturated value says so) or none (said here: a key AT the
            # limit would tie with the saturated value)
            if lo.kind == OFFSET:
                t, ovf = target(lo.value)
                if desc:   # first j with x[j] <= t
                    at = a + (b - a) - np.searchsorted(asc_x, t, "right")
                else:      # first j with x[j] >= t
                    at = a + np.searchsorted(asc_x, t, "left")
                s[a:b] = np.where(ovf == (-1 if desc else 1), b, at)
            if hi.kind == OFFSET:
                t, ovf = target(hi.value)
                if desc:   # last j with x[j] >= t
                    at = a + (b - a) - np.searchsorted(asc_x, t, "left") - 1
                else:      # last j with x[j] <= t
                    at = a + np.searchsorted(asc_x, t, "right") - 1
                e[a:b] = np.where(ovf == (1 if desc else -1), a - 1, at)
    empty = s > e
    sc = np.where(empty, 0, s)
    ec = np.where(empty, 0, e)

    # ---- results in sorted space ----------------------------------------------
    if value is not None:
        value = np.asarray(value)
        vok = np.ones(n, dtype=bool) if value_valid is None \
            else np.asarray(value_valid, dtype=bool)
        vok_s = vok[perm]
    if func in RANGE_POSITIONAL:
        at = perm[sc] if func == "first_value" else perm[ec]
        res = value[at] if n else value[:0]
        ok = ~empty & vok[at] if n else np.zeros(0, dtype=bool)
    else:
        if value is None:                              # COUNT(*)
            vs = np.ones(n, dtype=np.float64)
            vok_s = np.ones(n, dtype=bool)
        else:
            vs = np.where(vok_s, value.astype(np.float64)[perm], 0.0)
        # per-partition prefixes, as the device scans run
        cnt = np.cumsum(vok_s.astype(np.int64))
        cnt0 = np.r_[0, cnt]
        c = np.where(empty, 0, cnt0[ec + 1] - cnt0[sc]) if n else cnt
        if func in ("sum", "avg", "count"):
            cum = np.zeros(n + 1, dtype=np.float64)
            for a0, b0 in zip(p_starts, p_ends):
                cum[a0 + 1:b0 + 1] = np.cumsum(vs[a0:b0])
            before = np.where(sc > p0, cum[sc], 0.0) if n else cum[:0]
            acc = (cum[ec + 1] - before) if n else cum[:0]
        else:
            np_op = np.minimum if func == "min" else np.maximum
            ident = np.inf if func == "min" else -np.inf
            acc = _rmq(np.where(vok_s, vs, ident), sc, ec, np_op)
        if func == "count":
            res = c.astype(np.float64)
            ok = np.ones(n, dtype=bool)
        else:
            ok = ~empty & (c > 0)
            if func == "avg":
                acc = acc / np.where(c > 0, c, 1)
            res = np.where(ok, acc, np.nan)

    # ---- back to original row order --------------------------------------------
    if out_kind == "value":
        out = np.zeros(n, dtype=value.dtype)
        out[perm] = np.where(ok, res, np.zeros(1, dtype=value.dtype))
    elif out_kind == "i64":
        out = np.zeros(n, dtype=np.int64)
        out[perm] = np.where(ok, res, 0.0).astype(np.int64)
    else:
        out = np.empty(n, dtype=np.float64)
        out[perm] = res
    if out_kind == "i64":
        return out, None
    okv = np.zeros(n, dtype=np.uint8)
    okv[perm] = ok
    return out, okv
