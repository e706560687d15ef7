"""Build-from-columns routing: does a fused equi join build its hash table
straight from the build side's columns (Runtime.hash_build_cols: WHERE, NULL-key
drop, key pack and insert in one sweep, no wait), and may a build side whose
WHERE is still pending stay pending for it?

The answer is a pure function of plan facts, so it is tested without a device.
Two kinds of build side take the entry:

  * a materialized one, with an empty predicate, for every join type of the
    fused path (it replaces keypack + hash_build and nothing else changes);
  * a pending DeferredFilter on an INNER join, with its predicate over the
    unfiltered base columns. The table is then sized by the base rows and its
    row ids index the base columns, so a selective WHERE pays a larger clear
    and a sparser table; DSX_FILTERBUILD_MAX_ROWS caps the base rows up to
    which that trade was measured not to lose (profiles/filter_build.json).
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

# largest measured base size at which a pending build side was not slower
# than filter-then-build at 20 % and at 1 % selectivity (1.5 M, 6 M and 15 M
# measured; at 15 M and 1 % it lost 0.001-0.003 ms of 0.95)
DEFAULT_MAX_ROWS = 6_000_000
# build rows (base rows of a pending side) from which the entry is taken;
# smaller builds keep keypack + hash_build and their launch profile. Smallest
# measured base at which the entry won by more than the repeats differ
# (profiles/filter_build.json, "small" bases)
DEFAULT_MIN_ROWS = 4096


class Verdict(NamedTuple):
    ok: bool
    reason: str
    side: Optional[str] = None   # the build side, "l" / "r"
    pending: bool = False        # ok: that side stays an unrun WHERE

    def __bool__(self):
        return self.ok


def disabled() -> bool:
    """DSX_DISABLE_FILTERBUILD=1 restores keypack + hash_build everywhere (a
    pending build side then runs its filter first); read per call."""
    v = os.environ.get("DSX_DISABLE_FILTERBUILD")
    return bool(v) and v != "0"


def max_rows() -> int:
    """DSX_FILTERBUILD_MAX_ROWS: base rows up to which a pending build side
    stays pending; read per call."""
    try:
        return int(os.environ.get("DSX_FILTERBUILD_MAX_ROWS",
                                  DEFAULT_MAX_ROWS))
    except ValueError:
        return DEFAULT_MAX_ROWS


def min_rows() -> int:
    """DSX_FILTERBUILD_MIN_ROWS: build rows (base rows of a pending side)
    below which the table is built from a packed code column as before; read
    per call."""
    try:
        return int(os.environ.get("DSX_FILTERBUILD_MIN_ROWS",
                                  DEFAULT_MIN_ROWS))
    except ValueError:
        return DEFAULT_MIN_ROWS


def build_side(join_type: str, probe_side: Optional[str], n_l: int,
               n_r: int) -> str:
    """The fused path's build side: opposite a filter-probe side; else the
    rhs, except RIGHT (probes with the rhs) and INNER (builds on the smaller
    side). A pending side counts with its base rows."""
    if probe_side in ("l", "r"):
        return "r" if probe_side == "l" else "l"
    swap = join_type == "right" or (join_type == "inner" and n_l < n_r)
    return "l" if swap else "r"


def verdict(*, join_type: str, fusable: bool, pend_l: bool, pend_r: bool,
            n_l: int, n_r: int, probe_side: Optional[str],
            radix_min_build: Optional[int], cap: int, knob_off: bool,
            min_rows: int = 0,
            keys_int: bool = True, key_rewritten: bool = False,
            n_cols: int = 0, max_cols: int = 16) -> Verdict:
    """join_type: the plugin's lower-case name ("inner", "left", "right",
      "leftanti").
    fusable: the join takes the fused-emit path at all (equi keys, no
      residual, no null-equal keys, at most 16 output columns, fusing on).
    pend_l / pend_r: that input is a WHERE over a base table that has not
      run; n_l / n_r then are its base rows, else the input's rows.
    probe_side: the filter-probe verdict ("l"/"r") or None.
    radix_min_build: the radix path's build-size gate, None with radix off.
    min_rows: build rows from which the entry is taken at all.
    The last four are known only once the sides are set up: whether every key
    is an integer kind, whether the string-key reconciliation replaced the
    build side's key column, and the program + key column count against the
    entry's column limit."""
    if knob_off:
        return Verdict(False, "DSX_DISABLE_FILTERBUILD")
    if not fusable:
        return Verdict(False, "not a fused equi join")
    side = build_side(join_type, probe_side, n_l, n_r)
    pending = pend_l if side == "l" else pend_r
    n_b = n_l if side == "l" else n_r
    if n_b < min_rows:
        return Verdict(False, "build side below DSX_FILTERBUILD_MIN_ROWS",
                       side)
    if not keys_int:
        return Verdict(False, "join key is not an integer kind", side)
    if key_rewritten:
        return Verdict(False, "build key rewritten into the other side's "
                              "dictionary", side)
    if n_cols > max_cols:
        return Verdict(False, "too many program + key columns", side)
    if pending:
        if join_type != "inner":
            return Verdict(False, f"{join_type} join with a pending build "
                                  "side", side)
        if radix_min_build is not None and min(n_l, n_r) >= radix_min_build:
            return Verdict(False, "radix gate takes the join", side)
        if n_b > cap:
            return Verdict(False, "pending build side above "
                                  "DSX_FILTERBUILD_MAX_ROWS", side)
    return Verdict(True, "build from columns", side, pending)
