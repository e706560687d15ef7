"""Word planning for the device radix sort chain (Runtime.sort_word /
dsx_sort_word, csrc/radix_sort.inc).

An ORDER BY collation is cut into 64-bit order "words". dsx_sort_word sorts
stably by one word, so running the words least significant first sorts by
the whole collation — the reference's own procedure, key by key from the
last to the first with a stable sort (physical/utils/sort.py:36-60), with
several keys per step where they fit one code.

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
