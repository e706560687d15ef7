"""physical/keys.py (pure parts) and Runtime._keyspec_array — CPU only."""
import ctypes as ct
import types

import numpy as np
import pytest

from dask_sql_amd import runtime as rt
from dask_sql_amd.physical import keys


def _col(dtype=rt.I64, minmax=None, nullable=False, n=10, **kw):
    c = types.SimpleNamespace(dtype=dtype, len=n, data=1,
                              validity=2 if nullable else None, **kw)
    if minmax is not None:
        c._minmax = minmax
    return c


class _NoDevice:
    """Statistics are preset: any device call is a test failure."""
    def __getattr__(self, name):
        raise AssertionError(f"unexpected runtime call: {name}")


RT = _NoDevice()


def test_dictionary_rank():
    r = keys.dictionary_rank(["b", None, "a"])
    assert r.dtype == np.int64 and r.tolist() == [1, 0, 0]
    assert keys.dictionary_rank(["pear", "apple", None, "fig"]).tolist() \
        == [2, 0, 0, 1]
    e = keys.dictionary_rank([])
    assert e.dtype == np.int64 and e.tolist() == []
    assert keys.dictionary_rank([None, None]).tolist() == [0, 0]


def test_key_range():
    assert keys.key_range(RT, _col(minmax=(5, 14, 10))) == (5, 10)
    assert keys.key_range(RT, _col(minmax=(-3, -3, 1))) == (-3, 1)
    # no non-NULL row: whatever min/max hold is ignored
    assert keys.key_range(RT, _col(minmax=(77, -9, 0))) == (0, 1)


@pytest.mark.parametrize("l, r, exp", [
    ((5, 14, 10), (-2, 8, 4), (-2, 17)),   # both sides: the hull
    ((5, 14, 10), (99, -99, 0), (5, 10)),  # right empty: left's own
    ((99, -99, 0), (-2, 8, 4), (-2, 11)),  # left empty: right's own
    ((99, -99, 0), (42, 41, 0), (0, 1)),   # both empty
])
def test_joint_range(l, r, exp):
    assert keys.joint_range(RT, _col(minmax=l), _col(minmax=r)) == exp


def test_key_record():
    work = [_col(rt.I32, (5, 14, 10), nullable=True),
            _col(rt.F64, nullable=True), _col(rt.F32),
            _col(dtype=99, minmax=(0, 1, 10)),
            _col(rt.I64, (3, 1, 0))]
    assert keys.key_record(RT, work, 10, 0, 6, True) == \
        (0, False, 5, 10, True, 6)
    assert keys.key_record(RT, work, 10, 1, 2, True) == \
        (1, True, 0, 0, True, 2)
    assert keys.key_record(RT, work, 10, 2, 0, False) == \
        (2, True, 0, 0, False, 0)
    assert keys.key_record(RT, work, 10, 3, 0, True) is None
    assert keys.key_record(RT, work, 10, 4, 4, True) == \
        (4, False, 0, 1, False, 4)
    assert len(work) == 5  # nothing ranked
    assert keys.bucket_spec((0, False, 5, 10, True, 6)) == (0, 5, 10, True, 6)


def test_key_record_ranks_only_on_request():
    """A dictionary key: raw codes for PARTITION BY, its rank column
    (appended to work, sharing the validity) for ORDER BY."""
    calls = []

    class FakeRT:
        lib = None

        def upload_column(self, arr):
            calls.append(("upload", arr.tolist()))
            return _col(n=len(arr))

        def gather(self, col, sel, n):
            calls.append(("gather", sel, n))
            return _col(n=n)

        def minmax_i64(self, col):
            calls.append(("minmax",))
            return (0, 1, col.len)

    d = _col(rt.I32, (0, 2, 10), nullable=True, dictionary=["b", None, "a"])
    d.data = 1234
    work = [d]
    assert keys.key_record(FakeRT(), work, 10, 0, 0, False) == \
        (0, False, 0, 3, True, 0)
    assert calls == [] and len(work) == 1
    assert keys.key_record(FakeRT(), work, 10, 0, 4, True) == \
        (1, False, 0, 2, True, 4)
    assert calls == [("upload", [1, 0, 0]), ("gather", 1234, 10),
                     ("minmax",)]
    ranked = work[1]
    assert ranked.dtype == rt.I64 and ranked.validity == d.validity
    assert ranked._keep_alive[1] is d and not ranked._owner


def test_run_words_stops_at_a_refusal():
    from dask_sql_amd.physical.sort_words import plan_sort_words
    seen = []

    class FakeRT:
        def __init__(self, refuse_at):
            self.refuse_at = refuse_at

        def sort_word(self, cols, specs, n, perm):
            seen.append((cols, specs, perm))
            return None if len(seen) == self.refuse_at else f"p{len(seen)}"

    words = plan_sort_words([(0, True, 0, 0, False, 4),
                             (1, False, 5, 10, False, 4)])
    assert keys.run_words(FakeRT(0), words, ["f", "i"], 7) == "p2"
    assert seen == [(["i"], [(0, 5, 10, False, 4)], None),
                    (["f"], [(0, 0, 0, False, 12)], "p1")]
    del seen[:]
    assert keys.run_words(FakeRT(1), words, ["f", "i"], 7) is None
    assert len(seen) == 1


def _fields(k):
    return (k.col, k.min, k.range, k.nullable, k.mode)


def test_keyspec_array():
    fill = rt.Runtime._keyspec_array
    ks = fill([(3, -5, 11, True), (1, 1 << 40, (1 << 62) + 1, False)])
    assert len(ks) == 2 and isinstance(ks[0], rt._KeySpec)
    assert _fields(ks[0]) == (3, -5, 11, 1, 0)
    assert _fields(ks[1]) == (1, 1 << 40, (1 << 62) + 1, 0, 0)
    ks = fill([(0, 0, 0, True, 12), (2, 7, 3, 0, 6), (1, 0, 1, 1)])
    assert [_fields(k) for k in ks] == [(0, 0, 0, 1, 12), (2, 7, 3, 0, 6),
                                        (1, 0, 1, 1, 0)]
    empty = fill([])
    assert len(empty) == 1 and _fields(empty[0]) == (0, 0, 0, 0, 0)
    assert ct.sizeof(empty) == ct.sizeof(rt._KeySpec)


def test_aggspec_array_and_hist_cache_predicate():
    prog = rt.Runtime.make_prog([(1, 0, 0), (2, 0, 7)])
    aggs = rt.Runtime._aggspec_array([(rt.AGG_SUM_I64, prog),
                                      (rt.AGG_COUNT, prog)])
    assert len(aggs) == 2 and aggs[0].op == rt.AGG_SUM_I64
    assert aggs[1].op == rt.AGG_COUNT and aggs[1].prog_len == 2
    assert (aggs[1].prog[1].op, aggs[1].prog[1].imm) == (2, 7)
    assert len(rt.Runtime._aggspec_array([])) == 1

    owned = types.SimpleNamespace(_keep_alive=None, _owner=True)
    view = types.SimpleNamespace(_keep_alive=object(), _owner=False)
    kept = types.SimpleNamespace(_keep_alive=object(), _owner=True)
    unsafe = rt.Runtime._hist_cache_unsafe
    cols = [owned, view, kept]
    assert not unsafe(cols, [(0, 0, 1, False), (2, 0, 1, False)])
    assert unsafe(cols, [(0, 0, 1, False), (1, 0, 1, False, 1)])
    assert not unsafe(cols, [])
