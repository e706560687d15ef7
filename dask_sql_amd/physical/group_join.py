"""Group-join eligibility: may Aggregate(Projection(Join)) run as ONE sweep
that accumulates per build row (Runtime.filter_probe_groupby) instead of a
join followed by a group-by?

An inner PK-FK join grouped by the PK plus columns of the PK side has one
group per matched build row, so the join rows never need to exist (the
groupjoin of the literature; TPC-H Q3, Q10, Q18). The fused filter-probe path
already requires unique build keys and answers DSX_NOT_APPLICABLE otherwise;
what is left to decide from the plan is written here as a pure function of
plan facts, so it is tested without a device.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Sequence

# aggregate functions whose finish kind is one of Runtime.GB_FIN_KINDS (the
# stddev / variance family composes two accumulators on the host side)
FUNCS = frozenset({"sum", "count", "avg", "min", "max", "any_value",
                   "single_value", "every", "bool_and", "bool_or"})

DEFAULT_MIN_ROWS = 1 << 20


class AggFact(NamedTuple):
    func: str                      # lower-case SQL name
    arg_cols: Optional[frozenset]  # join-row columns the argument reads;
    #                                None for COUNT(*)
    distinct: bool = False
    filtered: bool = False         # carries a FILTER (WHERE ...) clause


class Verdict(NamedTuple):
    ok: bool
    reason: str
    # per output key: ("build", join-row column) gathered as it is, or
    # ("key", i): the build column of join key pair i stands in for its
    # probe-side twin
    key_sources: tuple = ()

    def __bool__(self):
        return self.ok


def disabled() -> bool:
    """DSX_DISABLE_GROUPJOIN=1 restores join-then-group-by; read per call."""
    v = os.environ.get("DSX_DISABLE_GROUPJOIN")
    return bool(v) and v != "0"


def min_rows() -> int:
    """DSX_GROUPJOIN_MIN_ROWS: probe base rows from which the path is taken;
    read per call. Below it a step is bound by its host waits on either
    path."""
    try:
        return int(os.environ.get("DSX_GROUPJOIN_MIN_ROWS", DEFAULT_MIN_ROWS))
    except ValueError:
        return DEFAULT_MIN_ROWS


def verdict(*, join_type: str, residual: bool, null_equal: bool,
            probe_side: Optional[str], n_lhs_cols: int,
            lhs_on: Sequence[int], rhs_on: Sequence[int],
            key_dtypes: Sequence[tuple], group_cols: Sequence[Optional[int]],
            aggs: Sequence[AggFact], max_aggs: int, max_keys: int) -> Verdict:
    """Columns are indices into the join's row: lhs columns first, then rhs
    (rhs_on and key positions of the rhs side are side-local, as the join
    plugin keeps them).

    probe_side: the join plugin's filter-probe verdict ("l"/"r": that side
      is a pending WHERE over a base table and the larger side), None when
      the join would not take the fused filter-probe path.
    key_dtypes: per join key pair (lhs dtype, rhs dtype), anything hashable.
    group_cols: per GROUP BY key its join-row column, None for a key that is
      not a plain column.
    """
    if join_type != "inner":
        return Verdict(False, f"{join_type} join")
    if not lhs_on or len(lhs_on) != len(rhs_on):
        return Verdict(False, "no equi keys")
    if residual:
        return Verdict(False, "residual condition")
    if null_equal:
        return Verdict(False, "null-equal keys")
    if probe_side not in ("l", "r"):
        return Verdict(False, "no pending WHERE on the probe side")
    if not aggs:
        return Verdict(False, "no aggregate")
    if len(aggs) > max_aggs:
        return Verdict(False, "too many aggregates")
    if not group_cols or len(group_cols) > max_keys:
        return Verdict(False, "too many or no group keys")

    def on_probe(col):
        return (col < n_lhs_cols) == (probe_side == "l")

    lhs_key = list(lhs_on)
    rhs_key = [n_lhs_cols + i for i in rhs_on]
    probe_key, build_key = (lhs_key, rhs_key) if probe_side == "l" \
        else (rhs_key, lhs_key)
    for i, (dl, dr) in enumerate(key_dtypes):
        if dl != dr:
            return Verdict(False, f"join key {i}: dtypes differ")
    sources = []
    covered = set()
    for g in group_cols:
        if g is None:
            return Verdict(False, "group key is not a column")
        if g in probe_key:
            i = probe_key.index(g)
            covered.add(i)
            sources.append(("key", i))
        elif on_probe(g):
            return Verdict(False, "group key from the probe side")
        else:
            if g in build_key:
                covered.add(build_key.index(g))
            sources.append(("build", g))
    if len(covered) != len(probe_key):
        return Verdict(False, "group keys miss a join key")
    for a in aggs:
        if a.distinct:
            return Verdict(False, "DISTINCT aggregate")
        if a.filtered:
            return Verdict(False, "FILTER aggregate")
        if a.func not in FUNCS:
            return Verdict(False, f"aggregate {a.func}")
        if a.arg_cols is not None and not all(on_probe(c)
                                              for c in a.arg_cols):
            return Verdict(False, "aggregate over a build column")
    return Verdict(True, "group-join", tuple(sources))
