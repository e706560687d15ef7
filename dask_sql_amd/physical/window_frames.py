"""Lowering of explicit ROWS window frames (reference
rel/logical/window.py:145-198) to the device frame model of
dsx_window_rows (include/dsxhip.h). Pure Python: no GPU, no library load.

A frame becomes ``(lo_off, hi_off)``: row offsets relative to the current
sorted position, ``None`` for an unbounded side. ``k PRECEDING`` is ``-k``,
``CURRENT ROW`` is ``0``, ``k FOLLOWING`` is ``+k``.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

# Mirror DSX_WIN_ROWS_DIRECT_MAXW / DSX_WIN_ROWS_TILE_MAXW in
# include/dsxhip.h (tests/test_window_frame_lowering.py compares them with
# dsx_window_rows_limits). Starting values, not tuned.
WIN_ROWS_DIRECT_MAXW = 64
WIN_ROWS_TILE_MAXW = 1024

FRAME_AGGS = ("sum", "count", "avg", "min", "max")
FRAME_POSITIONAL = ("first_value", "last_value")

# offsets past this act like "beyond any table" on the device and keep the
# C ABI's int64 arithmetic safe
_OFF_CLAMP = 1 << 40


class LoweredFrame(NamedTuple):
    lo_off: Optional[int]   # None = UNBOUNDED PRECEDING
    hi_off: Optional[int]   # None = UNBOUNDED FOLLOWING
    strategy: str           # "tile" | "prefix" | "host"


def frame_offsets(frame):
    """``("rows", lo, hi)`` as the parser emits it → ``(lo_off, hi_off)``,
    or None when the device model has no such frame (RANGE, UNBOUNDED
    FOLLOWING as the low bound, UNBOUNDED PRECEDING as the high bound)."""
    kind, lo, hi = frame
    if kind != "rows":
        return None

    def off(bound):
        side, k = bound
        if side == "current":
            return 0
        if k is None or int(k) < 0:
            raise ValueError(f"bad frame bound {bound}")
        k = min(int(k), _OFF_CLAMP)
        return -k if side == "preceding" else k

    if lo[0] == "unbounded_preceding":
        lo_off = None
    elif lo[0] in ("current", "preceding", "following"):
        lo_off = off(lo)
    else:
        return None
    if hi[0] == "unbounded_following":
        hi_off = None
    elif hi[0] in ("current", "preceding", "following"):
        hi_off = off(hi)
    else:
        return None
    return lo_off, hi_off


def frame_can_be_empty(lo_off, hi_off) -> bool:
    """True iff some row's frame can hold no row at all: the frame starts
    after the current row, ends before it, or is inverted. Then the first
    or last row of every partition has an empty frame, so any non-empty
    table yields at least one NULL."""
    if lo_off is not None and lo_off > 0:
        return True
    if hi_off is not None and hi_off < 0:
        return True
    return lo_off is not None and hi_off is not None and lo_off > hi_off


def frame_strategy(func, lo_off, hi_off) -> str:
    """Which dsx_window_rows path serves the frame: ``"tile"``
    (k_win_rows_tile), ``"prefix"`` (segmented scans + k_win_rows_prefix;
    also the positional FIRST/LAST copy) or ``"host"``."""
    if func in FRAME_POSITIONAL:
        return "prefix"
    if func not in FRAME_AGGS:
        return "host"
    if lo_off is None or hi_off is None:
        return "prefix"
    width = hi_off - lo_off + 1
    minmax = func in ("min", "max")
    if width <= (WIN_ROWS_TILE_MAXW if minmax else WIN_ROWS_DIRECT_MAXW):
        return "tile"
    # a bounded MIN/MAX has no prefix-difference form
    return "host" if minmax else "prefix"


def lower_rows_frame(func, frame) -> LoweredFrame:
    offs = frame_offsets(frame)
    if offs is None:
        return LoweredFrame(None, None, "host")
    lo_off, hi_off = offs
    return LoweredFrame(lo_off, hi_off, frame_strategy(func, lo_off, hi_off))


def frame_out_dtype(func, lo_off, hi_off, plan_is_bigint, value_nullable):
    """Static output type of a framed window column → ``(kind,
    with_validity)``, kind in ``"i64" | "f64" | "value"``. Matches what the
    host rolling path materializes: float64 with NULLs whenever an empty
    frame exists; otherwise COUNT is int64, SUM/MIN/MAX are int64 for a
    BIGINT plan type over a column without a validity buffer, and the rest
    is float64 with validity. FIRST/LAST keep the value column's dtype."""
    if func in FRAME_POSITIONAL:
        return "value", True
    if func not in FRAME_AGGS:
        raise ValueError(f"window function {func} with an explicit frame")
    if frame_can_be_empty(lo_off, hi_off):
        return "f64", True
    if func == "count":
        return "i64", False
    if func in ("sum", "min", "max") and plan_is_bigint \
            and not value_nullable:
        return "i64", False
    return "f64", True
