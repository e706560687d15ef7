"""Key resolution: how a column becomes a DsxKeySpec for the sort, window,
join and group-by kernels — its (min, range), its rank column when it is a
dictionary, its resolved key record — and how a planned sort_word chain is
run. The one owner of these decisions; the plugins only pick modes and
engines.

Plain Python over the Runtime interface (no library load at import), so it
runs on CPU against a fake runtime.
"""
from __future__ import annotations

import numpy as np

from dask_sql_amd import runtime as rt

INT_KINDS = (rt.I64, rt.I32, rt.I8, rt.BOOL8)
FLOAT_KINDS = (rt.F64, rt.F32)


def dicts_of(cols):
    return [getattr(c, "dictionary", None) for c in cols]


def codes_i32(runtime, col):
    """Dictionary codes as a 4-byte column, the width a gather reads its
    row ids in. Factorized table columns already are; 8-byte codes out of a
    groupby or 1-byte codes of a declared dictionary are converted through
    the host (the VM has no 4-byte output)."""
    if col.dtype == rt.I32:
        return col
    arr, valid = col.to_numpy()
    arr = np.array(arr, dtype=np.int32)
    if valid is not None:
        arr[~valid.astype(bool)] = 0  # NULL rows: any in-range code
    return runtime.upload_column(
        arr,
        None if valid is None else valid.astype(np.uint8), rt.I32)


def minmax_cached(runtime, col):
    """Column statistics memo (the reference caches table statistics too —
    datacontainer.py Statistics / statistics.py:21). Derived columns (gather
    outputs) chain to their source via _stats_src: a subset's range is
    bounded by its source's, so the PERSISTENT base column caches the range
    across query steps (a superset range only widens the key space, never
    changes results)."""
    hit = getattr(col, "_minmax", None)
    if hit is not None:
        return hit
    src = getattr(col, "_stats_src", None)
    if src is not None and col.len > 0:
        mn, mx, _ = minmax_cached(runtime, src)
        hit = (mn, mx, col.len)  # conservative: subset of source rows
        col._minmax = hit
        return hit
    hit = runtime.minmax_i64(col)
    col._minmax = hit
    return hit


def key_range(runtime, col):
    """(min, range) of an integer-kind key column; a column without a
    non-NULL row is (0, 1)."""
    mn, mx, nn = minmax_cached(runtime, col)
    if nn == 0:
        return 0, 1
    return mn, mx - mn + 1


def joint_range(runtime, lcol, rcol):
    """(min, range) of one join key over both sides, so that the two sides'
    codes are comparable; a side without a non-NULL row does not count."""
    lmn, lmx, lnn = minmax_cached(runtime, lcol)
    rmn, rmx, rnn = minmax_cached(runtime, rcol)
    if lnn == 0 and rnn == 0:
        return 0, 1
    if lnn == 0:
        return rmn, rmx - rmn + 1
    if rnn == 0:
        return lmn, lmx - lmn + 1
    mn = min(lmn, rmn)
    return mn, max(lmx, rmx) - mn + 1


def dictionary_rank(dictionary):
    """int64 rank[code] = alphabetic position of the code's string.
    Dictionary codes are in first-appearance order; None entries keep rank
    0 and never take part (their rows are NULL)."""
    order = sorted((i for i, s in enumerate(dictionary) if s is not None),
                   key=lambda i: dictionary[i])
    rank = np.zeros(len(dictionary), dtype=np.int64)
    rank[order] = np.arange(len(order), dtype=np.int64)
    return rank


def ranked_column(runtime, col, n):
    """The I64 rank column of dictionary column `col`: its rank LUT
    gathered through the codes, sharing the source's validity."""
    lut = runtime.upload_column(dictionary_rank(col.dictionary))
    g = runtime.gather(lut, col.data, n)
    return rt.DeviceColumn(runtime, g.data, col.validity, n, rt.I64,
                           owner=False, keep_alive=(g, col, lut))


def key_record(runtime, work, n, idx, mode, rank):
    """Key work[idx] (n rows) resolved as plan_sort_words and
    plan_window_words take it: (col_idx, is_float, min, range, nullable,
    mode), or None for a dtype the device does not sort. The bucket
    sort's spec is the record without is_float (bucket_spec). rank: a
    dictionary key sorts by its
    rank column, which is appended to `work` (an ORDER BY key; a PARTITION
    BY key only needs equal strings to have equal codes)."""
    col = work[idx]
    if rank and getattr(col, "dictionary", None) is not None:
        col = ranked_column(runtime, col, n)
        work.append(col)
        idx = len(work) - 1
    if col.dtype in FLOAT_KINDS:
        return (idx, True, 0, 0, bool(col.validity), mode)
    if col.dtype not in INT_KINDS:
        return None
    mn, rng = key_range(runtime, col)
    return (idx, False, mn, rng, bool(col.validity), mode)


def bucket_spec(rec):
    """The (col, min, range, nullable, mode) of an integer-kind key record
    that sort_perm takes."""
    return rec[:1] + rec[2:]


def run_words(runtime, words, work, n):
    """Runs a planned word chain (least significant word first, each word
    bringing only its own key columns): the stable sort_word passes add up
    to a sort by the whole key list. Returns the permutation, or None as
    soon as sort_word refuses a word."""
    perm = None
    for w in words:
        perm = runtime.sort_word([work[i] for i in w.cols], list(w.specs),
                                 n, perm)
        if perm is None:
            return None
    return perm
