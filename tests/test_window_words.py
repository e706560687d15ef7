"""CPU tests of plan_window_words (dask_sql_amd/physical/sort_words.py): how
a window's PARTITION BY / ORDER BY keys are cut into the 64-bit words that
dsx_sort_word sorts by and dsx_window_mark_word marks boundaries on."""
import numpy as np
import pandas as pd

from dask_sql_amd.physical.sort_words import (PARTITION_MODE,
                                              plan_window_words,
                                              window_order_mode)

DESC, NULLS_LAST, FLOAT = 2, 4, 8


def _ikey(col, rng=10, nullable=False, mode=NULLS_LAST, mn=0):
    return (col, False, mn, rng, nullable, mode)


def _fkey(col, nullable=False, mode=NULLS_LAST):
    return (col, True, 0, 0, nullable, mode)


def _sides(words):
    return [w.is_partition for w in words]


def test_order_words_come_before_partition_words_and_never_mix():
    part = [_ikey(0), _fkey(1), _ikey(2)]
    order = [_ikey(3), _fkey(4), _ikey(5), _ikey(0)]
    words = plan_window_words(part, order)
    sides = _sides(words)
    assert sides == sorted(sides)          # every False before every True
    assert sides.count(True) == 3 and sides.count(False) == 3
    pcols, ocols = {0, 1, 2}, {3, 4, 5, 0}
    for w in words:
        assert set(w.cols) <= (pcols if w.is_partition else ocols)
    # least significant first inside each side: order [i5,i0] [f4] [i3],
    # partition [i2] [f1] [i0]
    assert [w.cols for w in words] == [(0, 5), (4,), (3,),
                                       (2,), (1,), (0,)]
    # small integer keys next to each other across the PARTITION/ORDER
    # seam still do not share a word
    words = plan_window_words([_ikey(0)], [_ikey(1)])
    assert [(w.cols, w.is_partition) for w in words] == [((1,), False),
                                                         ((0,), True)]


def test_float_key_stands_alone_in_its_word():
    words = plan_window_words([_ikey(0), _fkey(1, nullable=True)],
                              [_fkey(2, mode=DESC | NULLS_LAST), _ikey(3)])
    for w in words:
        if any(s[4] & FLOAT for s in w.specs):
            assert len(w.specs) == 1 and len(w.cols) == 1
    by_col = {w.cols: w for w in words}
    assert by_col[(1,)].specs == ((0, 0, 0, True, PARTITION_MODE | FLOAT),)
    assert by_col[(1,)].is_partition
    assert by_col[(2,)].specs == ((0, 0, 0, False,
                                   DESC | NULLS_LAST | FLOAT),)
    assert not by_col[(2,)].is_partition


def test_two_partition_and_four_order_keys():
    part = [_ikey(0, rng=100), _ikey(1, rng=50, nullable=True)]
    order = [_ikey(2 + j, rng=10 + j) for j in range(4)]
    words = plan_window_words(part, order)
    assert _sides(words) == [False, True]
    # in-word key order is reversed significance (last key on stride 1)
    assert words[0].cols == (5, 4, 3, 2)
    assert [s[2] for s in words[0].specs] == [13, 12, 11, 10]
    assert words[1].cols == (1, 0)
    assert words[1].specs == ((0, 0, 50, True, PARTITION_MODE),
                              (1, 0, 100, False, PARTITION_MODE))
    # a fifth order key opens another order word, not a mixed one
    words = plan_window_words(part, order + [_ikey(6)])
    assert _sides(words) == [False, False, True]
    assert [len(w.specs) for w in words] == [1, 4, 2]


def test_two_keys_of_range_2_40_split_into_two_words():
    r = 1 << 40
    words = plan_window_words([_ikey(0, rng=r), _ikey(1, rng=r)], [])
    assert [(w.cols, w.is_partition) for w in words] == [((1,), True),
                                                         ((0,), True)]
    words = plan_window_words([], [_ikey(0, rng=r), _ikey(1, rng=r)])
    assert [(w.cols, w.is_partition) for w in words] == [((1,), False),
                                                         ((0,), False)]
    # 2^31 * 2^31 = 2^62 is the last space that fits one word
    words = plan_window_words([_ikey(0, rng=1 << 31), _ikey(1, rng=1 << 31)],
                              [])
    assert [len(w.specs) for w in words] == [2]


def test_explicit_nulls_first_clears_bit_4_on_that_key_only():
    assert window_order_mode(False, None) == NULLS_LAST
    assert window_order_mode(False, False) == NULLS_LAST
    assert window_order_mode(False, True) == 0
    assert window_order_mode(True, True) == DESC
    order = [_ikey(0, nullable=True, mode=window_order_mode(False, True)),
             _ikey(1, nullable=True, mode=window_order_mode(True, False)),
             _fkey(2, nullable=True, mode=window_order_mode(False, None))]
    words = plan_window_words([_ikey(3, nullable=True)], order)
    modes = {}
    for w in words:
        for s in w.specs:
            modes[w.cols[s[0]]] = s[4]
    assert modes == {0: 0, 1: DESC | NULLS_LAST, 2: NULLS_LAST | FLOAT,
                     3: PARTITION_MODE}


def test_desc_sets_bit_2():
    assert window_order_mode(True, None) == DESC | NULLS_LAST
    assert window_order_mode(True, None) & DESC
    assert not window_order_mode(False, None) & DESC
    (w,) = plan_window_words([], [_ikey(0, mode=window_order_mode(True,
                                                                  None))])
    assert w.specs[0][4] & DESC and not w.is_partition


def test_partition_keys_always_take_mode_4():
    words = plan_window_words([_ikey(0, mode=DESC), _fkey(1, mode=0)], [])
    assert [s[4] for w in words for s in w.specs] == \
        [PARTITION_MODE | FLOAT, PARTITION_MODE]
    assert PARTITION_MODE == NULLS_LAST


def test_no_partition_keys_no_partition_words():
    words = plan_window_words([], [_ikey(0), _fkey(1)])
    assert words and not any(w.is_partition for w in words)
    words = plan_window_words([_fkey(0)], [])
    assert _sides(words) == [True]
    assert plan_window_words([], []) == []


def test_chain_and_marks_equal_pandas_on_host():
    """Simulate the chain with numpy stable sorts on the words' codes, and
    the boundary marks with code != left-neighbour code per word: the
    permutation is the host path's (order keys, then partition keys, all
    mergesort), the OR of the partition words' marks starts the pandas
    groups, and the order words' marks on top start the peer groups."""
    rng = np.random.default_rng(11)
    n = 4000
    data = {i: rng.integers(0, 5, n) for i in range(7)}
    part = [_ikey(i, rng=5) for i in (0, 1)]
    desc = {2: False, 3: True, 4: False, 5: True, 6: False}
    order = [_ikey(i, rng=5, mode=window_order_mode(desc[i], None))
             for i in (2, 3, 4, 5, 6)]
    words = plan_window_words(part, order)
    assert _sides(words) == [False, False, True]

    def codes(w):
        code = np.zeros(n, dtype=np.int64)
        stride = 1
        for local, mn, rg, _, mode in w.specs:
            v = data[w.cols[local]] - mn
            if mode & DESC:
                v = (rg - 1) - v
            code += v * stride
            stride *= rg
        return code

    perm = np.arange(n)
    for w in words:
        perm = perm[np.argsort(codes(w)[perm], kind="stable")]
    df = pd.DataFrame({f"k{i}": data[i] for i in range(7)})
    exp = df.sort_values([f"k{i}" for i in (2, 3, 4, 5, 6)],
                         ascending=[not desc[i] for i in (2, 3, 4, 5, 6)],
                         kind="mergesort")
    exp = exp.sort_values(["k0", "k1"], kind="mergesort")
    assert perm.tolist() == exp.index.tolist()

    def marks(side):
        m = np.zeros(n, dtype=bool)
        for w in words:
            if w.is_partition == side:
                c = codes(w)[perm]
                m |= np.r_[True, c[1:] != c[:-1]]
        return m

    pm = marks(True)
    fm = pm | marks(False)
    pid = exp.groupby(["k0", "k1"], sort=False).ngroup().to_numpy()
    fid = exp.groupby([f"k{i}" for i in range(7)],
                      sort=False).ngroup().to_numpy()
    assert (np.cumsum(pm) - 1).tolist() == pid.tolist()
    assert (np.cumsum(fm) - 1).tolist() == fid.tolist()
