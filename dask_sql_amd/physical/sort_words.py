"""Word planning for the device radix sort chain (Runtime.sort_word /
dsx_sort_word, csrc/radix_sort.inc).

An ORDER BY collation is cut into 64-bit order "words". dsx_sort_word sorts
stably by one word, so running the words least significant first sorts by
the whole collation — the reference's own procedure, key by key from the
last to the first with a stable sort (physical/utils/sort.py:36-60), with
several keys per step where they fit one code.

A window's PARTITION BY / ORDER BY keys are cut the same way by
plan_window_words, partition and order keys in words of their own, so that
Runtime.window_mark_word can tell a partition boundary from a peer boundary.

Pure Python, no GPU: the plan is testable on its own.
"""
from __future__ import annotations

from typing import NamedTuple

MAX_KEYS = 4          # DSX_MAX_KEYS (include/dsxhip.h)
MAX_SPACE = 1 << 62   # packed key space bound of pack_key words
MODE_FLOAT = 8        # DsxKeySpec mode bit 3: float key, a word of its own


class SortWord(NamedTuple):
    """One dsx_sort_word call.

    cols:  indices into the CALLER's column list of the columns this word
           reads, each once — the word's own column array.
    specs: (col, min, range, nullable, mode) per key, `col` indexing
           `cols`, in the REVERSED significance order pack_key expects
           (the word's last ORDER BY key first, on stride 1)."""
    cols: tuple
    specs: tuple


class WindowWord(NamedTuple):
    """One word of a window's (partition, order) sort: a SortWord plus
    which side of the OVER clause its keys come from."""
    cols: tuple
    specs: tuple
    is_partition: bool


def _emit(group):
    """group: keys of one word in ORDER BY (most significant first) order."""
    cols = []
    specs = []
    for col_idx, is_float, mn, rng, nullable, mode in reversed(group):
        if col_idx not in cols:
            cols.append(col_idx)
        local = cols.index(col_idx)
        if is_float:
            specs.append((local, 0, 0, bool(nullable), int(mode) | MODE_FLOAT))
        else:
            specs.append((local, int(mn), int(rng), bool(nullable),
                          int(mode)))
    return SortWord(tuple(cols), tuple(specs))


def plan_sort_words(keys):
    """keys: the resolved collation in ORDER BY order, one
    (col_idx, is_float, min, range, nullable, mode) per key; mode carries
    bit 2 = DESC and bit 4 = NULLS LAST.

    Returns the SortWords LEAST significant first — the order to run them:

        perm = None
        for w in plan_sort_words(keys):
            perm = runtime.sort_word([cols[i] for i in w.cols], w.specs,
                                     n, perm)

    Each float key is a word of its own (its code fills all 64 bits).
    Consecutive integer-kind keys share a word greedily, from the most
    significant key on, while the word has at most MAX_KEYS keys and the
    product of (range + nullable) stays at most 2^62. A single key whose
    own range exceeds 2^62 still gets its word; dsx_sort_word then answers
    -4 and the caller sorts on the host."""
    words = []   # most significant first while building
    group = []
    space = 1
    for key in keys:
        col_idx, is_float, mn, rng, nullable, mode = key
        if is_float:
            if group:
                words.append(_emit(group))
                group, space = [], 1
            words.append(_emit([key]))
            continue
        width = int(rng) + (1 if nullable else 0)
        if width < 1:
            raise ValueError(f"sort key on column {col_idx}: empty range")
        if group and (len(group) >= MAX_KEYS or space * width > MAX_SPACE):
            words.append(_emit(group))
            group, space = [], 1
        group.append(key)
        space *= width
    if group:
        words.append(_emit(group))
    words.reverse()
    return words


PARTITION_MODE = 4    # ascending, NULLS LAST — how the host sorts partitions


def window_order_mode(desc, nulls_first):
    """DsxKeySpec mode of a window ORDER BY key: bit 2 = DESC; bit 4 =
    NULLS LAST unless the key is explicitly NULLS FIRST (nulls_first is
    True) — the host path places NULLs last for both directions when the
    query does not say."""
    return (2 if desc else 0) | (0 if nulls_first is True else 4)


def plan_window_words(part_keys, order_keys):
    """The sort_word chain of a window: rows sorted by the partition keys,
    then the order keys, with every word tagged by the side it belongs to.

    part_keys, order_keys: key lists in the plan_sort_words format, most
    significant first. Order keys carry window_order_mode(); partition keys
    are always taken with PARTITION_MODE, whatever mode they carry.

    Returns WindowWords LEAST significant first — plan_sort_words(order_keys)
    followed by plan_sort_words(part_keys). A word never mixes the two
    sides: the OR of the partition words' boundary marks (Runtime.
    window_mark_word) is then exactly the partition boundaries, and the
    order words' marks on top of them the peer boundaries."""
    part_keys = [(c, f, mn, rng, nullable, PARTITION_MODE)
                 for c, f, mn, rng, nullable, _mode in part_keys]
    return [WindowWord(w.cols, w.specs, False)
            for w in plan_sort_words(order_keys)] + \
           [WindowWord(w.cols, w.specs, True)
            for w in plan_sort_words(part_keys)]
