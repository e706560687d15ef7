"""Validation of RANGE window frames and resolution of their offsets to the
order key's unit — the builder's half of RANGE frames with value offsets.
Pure Python. The bound model, the dtype rule and the host model that consume
the resolved frame are in physical/window_range.py.

A parsed bound is ``(side, value)`` with side in ``unbounded_preceding |
preceding | current | following | unbounded_following`` and, for an offset,
a value that is an int, a float or ``("interval", n, unit)``.
"""
from __future__ import annotations

import math

RANGE_AGGS = ("sum", "count", "avg", "min", "max")
RANGE_POSITIONAL = ("first_value", "last_value")
RANGE_FUNCS = RANGE_AGGS + RANGE_POSITIONAL

INT64_MAX = (1 << 63) - 1
INT64_MIN = -(1 << 63)

_INT_TYPES = ("BIGINT", "INTEGER", "SMALLINT", "TINYINT")
_FLOAT_TYPES = ("DOUBLE", "FLOAT", "REAL")

_NS = {"DAY": 86_400_000_000_000, "WEEK": 7 * 86_400_000_000_000,
       "HOUR": 3_600_000_000_000, "MINUTE": 60_000_000_000,
       "SECOND": 1_000_000_000, "MILLISECOND": 1_000_000,
       "MICROSECOND": 1_000}
_CALENDAR = ("MONTH", "YEAR", "QUARTER")

# bound kinds in frame order: a low bound may not be of a later kind than
# the high bound
_SIDE_RANK = {"unbounded_preceding": 0, "preceding": 1, "current": 2,
              "following": 3, "unbounded_following": 4}


def resolve_offset(value, key_type: str):
    """A parsed offset (int, float or ``("interval", n, unit)``) in the unit
    of an order key of SQL type ``key_type``: int for integer, DATE (days)
    and TIMESTAMP (nanoseconds) keys, float for DOUBLE/FLOAT keys."""
    interval = isinstance(value, tuple)
    if interval:
        _, qty, unit = value
        unit = str(unit).upper()
        if qty < 0:
            raise ValueError("a RANGE frame offset must not be negative")
    elif value < 0:
        raise ValueError("a RANGE frame offset must not be negative")
    if key_type in _INT_TYPES:
        if interval:
            raise ValueError(
                f"INTERVAL offset on a {key_type} RANGE order key")
        return min(int(math.floor(value)), INT64_MAX)
    if key_type in _FLOAT_TYPES:
        if interval:
            raise ValueError(
                f"INTERVAL offset on a {key_type} RANGE order key")
        return float(value)
    if key_type == "DATE":
        if not interval:
            return min(int(math.floor(value)), INT64_MAX)
        if unit == "DAY":
            return min(int(qty), INT64_MAX)
        if unit == "WEEK":
            return min(7 * int(qty), INT64_MAX)
        raise NotImplementedError(
            f"RANGE offset INTERVAL {unit} on a DATE order key")
    if key_type == "TIMESTAMP":
        if not interval:
            raise NotImplementedError(
                "a bare number as RANGE offset on a TIMESTAMP order key "
                "(no unit): write an INTERVAL")
        if unit in _CALENDAR or unit not in _NS:
            raise NotImplementedError(
                f"RANGE offset INTERVAL {unit} on a TIMESTAMP order key")
        return min(int(qty) * _NS[unit], INT64_MAX)
    raise ValueError(f"RANGE offset on a {key_type} order key")


def resolve_range_frame(frame, order_types):
    """Validate a parsed ``("range", lo, hi)`` frame against the ORDER BY
    key types and resolve every offset to the key's unit. Returns the frame
    in the same shape, ``("range", (side, value), (side, value))``."""
    kind, lo, hi = frame
    if kind != "range":
        raise ValueError(f"not a RANGE frame: {frame}")
    for b in (lo, hi):
        if b[0] not in _SIDE_RANK:
            raise ValueError(f"bad frame bound {b}")
    if lo[0] == "unbounded_following":
        raise ValueError("UNBOUNDED FOLLOWING cannot start a frame")
    if hi[0] == "unbounded_preceding":
        raise ValueError("UNBOUNDED PRECEDING cannot end a frame")
    if _SIDE_RANK[lo[0]] > _SIDE_RANK[hi[0]]:
        raise ValueError(
            f"frame starts at {lo[0].upper()} but ends at {hi[0].upper()}")
    out = []
    for b in (lo, hi):
        if b[0] in ("preceding", "following"):
            if len(order_types) != 1:
                raise ValueError(
                    "a RANGE frame with an offset needs exactly one "
                    f"ORDER BY key, got {len(order_types)}")
            out.append((b[0], resolve_offset(b[1], order_types[0])))
        else:
            out.append((b[0], 0 if b[0] == "current" else None))
    return ("range", out[0], out[1])
