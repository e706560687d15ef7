"""Join routing: which executor runs a join, which side probes and which
builds, which pending WHERE stays pending, and whether the hash table is built
straight from columns — decided in one place, from what the plan and the
inputs say before any device work. Pure functions of plan facts (no device
access, no library load at import), so they are tested without a device;
physical/join.py gathers the facts and runs what `route` says. Precedence:

  1. the filter-probe side (a pending WHERE on the larger side of a fused
     INNER join) is chosen first and stands down behind the radix build-size
     gate and behind the entry's column limit;
  2. filter_build.verdict says whether a pending build side stays pending;
  3. the radix path is tried only when neither holds;
  4. then the fused path;
  5. last the pair, anti-residual or cross path.

Every other pending side runs its WHERE first (`JoinRoute.materialize`). Which
of such sides builds, and the radix gate, go by their real rows: while a
`Side.mat_rows` is unknown, `route` answers with path None and the sides to
run, and is asked again with the count filled in. What stays pending is
decided from base rows alone, so it is the same in both answers.
"""
from __future__ import annotations

import os
from collections import namedtuple

from dask_sql_amd import runtime as rt
from dask_sql_amd.physical import filter_build as fb
from dask_sql_amd.physical.keys import INT_KINDS

FUSED_TYPES = ("inner", "left", "right", "leftanti")
MAX_OUT_COLS = 16  # columns one fused emit materializes

Knobs = namedtuple("Knobs", "disable_radix radix_min_build radix_min_probe "
                   "disable_joinfuse disable_filterprobe disable_filterbuild "
                   "filterbuild_max_rows filterbuild_min_rows")
# One input. deferred: a DeferredFilter, run or not; pending: its WHERE has
# not run. rows: its rows, the base table's while pending; mat_rows: a pending
# side's rows once its WHERE has run for this join. n_cols: the program + key
# columns it hands to dsx_filter_probe_cols / dsx_hash_build_cols while it
# stays pending, counted by column identity (a side whose WHERE has run hands
# over its few key columns alone, which never reach the limit)
Side = namedtuple("Side", "rows deferred pending mat_rows n_cols",
                  defaults=(False, False, None, 0))
# join_type: the plugin's lower-case name. keys: per equi key (lhs dtype, rhs
# dtype, whether the dictionary remap rewrites the rhs key: both dictionaries,
# not the same object, not equal lists). null_aware (NOT IN): its NULL check
# reads the rhs before routing. n_mat: columns the plan consumes
JoinFacts = namedtuple(
    "JoinFacts", "join_type keys lhs rhs residual null_eq null_aware n_mat",
    defaults=(False, False, False, 0))
# path: "radix" / "fused" / "pairs" / "anti_residual" / "cross", None while
# `materialize` (pending sides, in the order their WHERE runs) has to run
# first. swap: probe with the rhs, build on the lhs; ktype: the kernels' join
# type. fprobe / fbuild: the side whose WHERE runs inside the probe / build.
# build_from_cols: hash_build_cols, else keypack + hash_build. fallback: the
# path if radix_join declines
JoinRoute = namedtuple(
    "JoinRoute", "path swap ktype fprobe fbuild build_from_cols materialize "
    "fallback reason",
    defaults=(False, rt.JOIN_INNER, None, None, False, (), None, ""))


def filterprobe_disabled() -> bool:
    """DSX_DISABLE_FILTERPROBE=1: a WHERE over a base table runs at once (no
    DeferredFilter) and no join fuses one into its probe; read per call."""
    return bool(os.environ.get("DSX_DISABLE_FILTERPROBE"))


def knobs() -> Knobs:
    """Every join-routing environment variable, read now. The join's own
    DSX_DISABLE_* switches are on when set to anything but the empty string;
    a radix size that is not an integer is an error, as it always was."""
    env = os.environ.get
    return Knobs(bool(env("DSX_DISABLE_RADIX")),
                 int(env("DSX_RADIX_MIN_BUILD", 8_000_000)),
                 int(env("DSX_RADIX_MIN_PROBE", 4_000_000)),
                 bool(env("DSX_DISABLE_JOINFUSE")), filterprobe_disabled(),
                 fb.disabled(), fb.max_rows(), fb.min_rows())


def fusable(f, k) -> bool:
    """The fused-emit precondition: equi keys, no residual, no null-equal
    keys, at most 16 materialized columns, fusing on, a join type the probe
    kernels emit."""
    return bool(f.keys and not f.residual and not f.null_eq
                and f.n_mat <= MAX_OUT_COLS and not k.disable_joinfuse
                and f.join_type in FUSED_TYPES)


def sides(join_type, n_l, n_r, fprobe=None, fbuild=None):
    """(swap, ktype): the probe and build sides of every hash path. A
    filter-probe side probes and a filter-build side builds; else the rhs
    builds, except RIGHT (probes with the rhs) and INNER (builds on the
    smaller side). FULL OUTER runs as LEFT plus the unmatched build rows."""
    if fbuild and fprobe is None:
        fprobe = "r" if fbuild == "l" else "l"
    if fb.build_side(join_type, fprobe, n_l, n_r) == "l":
        return True, rt.JOIN_LEFT if join_type == "right" else rt.JOIN_INNER
    return False, {"inner": rt.JOIN_INNER, "left": rt.JOIN_LEFT,
                   "outer": rt.JOIN_LEFT,
                   "leftanti": rt.JOIN_LEFTANTI}[join_type]


def route(f, k, group_join=False) -> JoinRoute:
    """The one decision over JoinFacts f and Knobs k. group_join: the route of
    the aggregate's group-join attempt over this join — its accumulators are
    sized by the build rows, so the build side always runs its WHERE, and the
    caller checks the probe side's column count itself, with its argument
    columns added."""
    fus = fusable(f, k)
    keys_int = all(a in INT_KINDS and b in INT_KINDS for a, b, _ in f.keys)
    rewritten = any(w for _, _, w in f.keys)
    side = {"l": f.lhs, "r": f.rhs}
    gate = None if k.disable_radix else k.radix_min_build

    def verdict(pend_l, pend_r, n_l, n_r, probe, late_for=None):
        late = {}
        if late_for:  # what the entry would get of that build side
            late = dict(keys_int=keys_int,
                        key_rewritten=rewritten and late_for == "r",
                        n_cols=side[late_for].n_cols
                        if (pend_l, pend_r)[late_for == "r"] else 0)
        return fb.verdict(
            join_type=f.join_type, fusable=fus, pend_l=pend_l, pend_r=pend_r,
            n_l=n_l, n_r=n_r, probe_side=probe, radix_min_build=gate,
            cap=k.filterbuild_max_rows, knob_off=k.disable_filterbuild,
            min_rows=k.filterbuild_min_rows, max_cols=rt.MAX_COLS, **late)

    # 1, 2. which pending WHERE stays pending, from base rows alone
    pend_l, pend_r = f.lhs.pending, f.rhs.pending
    n_l, n_r = f.lhs.rows, f.rhs.rows
    fprobe = fbuild = wide = v = None
    dropped = []  # sides taken at first that run their WHERE after all, last
    reason = ""
    if pend_l or pend_r:
        if (f.join_type == "inner" and fus and not k.disable_filterprobe
                and not (gate is not None and min(n_l, n_r) >= gate)):
            larger = "r" if n_l < n_r else "l"
            fprobe = larger if side[larger].pending else None
        b = fb.build_side(f.join_type, fprobe, n_l, n_r)
        if side[b].pending and not group_join:
            v = verdict(pend_l, pend_r, n_l, n_r, fprobe, b)
            if v:
                fbuild = b
            else:
                reason = f"build side filters first ({v.reason}); "
                if ((not keys_int or side[b].n_cols > rt.MAX_COLS
                     or (rewritten and b == "r"))
                        and verdict(pend_l, pend_r, n_l, n_r, fprobe)):
                    dropped = [b]  # declined by what its columns are
        if not keys_int:  # pair path: nothing stays pending
            dropped = [s for s in "lr" if s in (fprobe, fbuild, *dropped)]
            fprobe = fbuild = None
        elif (fprobe and not group_join
              and side[fprobe].n_cols > rt.MAX_COLS):
            reason += "probe side filters first (program + key columns); "
            wide, fprobe = fprobe, None
            dropped.insert(0, wide)
    kept = (fprobe, fbuild)
    materialize = tuple(
        [s for s in "lr" if side[s].pending and s not in kept
         and s not in dropped] + dropped)
    if "l" in materialize:
        n_l = f.lhs.mat_rows
    if "r" in materialize:
        n_r = f.rhs.mat_rows
    if n_l is None or n_r is None:
        # the sides are known already where a kept side forces them
        swap, ktype = sides(f.join_type, 0, 0, fprobe, fbuild) \
            if fprobe or fbuild else (False, rt.JOIN_INNER)
        return JoinRoute(None, swap, ktype, fprobe, fbuild, False,
                         materialize, None, reason + "row counts pending")

    swap, ktype = sides(f.join_type if f.keys else "inner", n_l, n_r, fprobe,
                        fbuild)

    def done(path, from_cols=False, fallback=None):
        return JoinRoute(path, swap, ktype, fprobe, fbuild, from_cols,
                         materialize, fallback, reason + path)

    if not f.keys:
        return done("cross")
    # 3. radix: only when nothing stays pending, and by the real row counts
    n_b, n_p = (n_l, n_r) if swap else (n_r, n_l)
    radix = (not fprobe and not fbuild and keys_int and not f.residual
             and not f.null_eq and f.n_mat <= MAX_OUT_COLS
             and not k.disable_radix and f.join_type in FUSED_TYPES
             and n_b >= k.radix_min_build and n_p >= k.radix_min_probe)
    if not (fus and keys_int):
        if radix:
            return done("radix", False, "pairs")
        if f.residual and f.join_type == "leftanti":
            swap, ktype = sides("inner", n_l, n_r)
            return done("anti_residual")
        return done("pairs")
    # build from columns: a materialized side takes the entry with an empty
    # predicate. A WHERE that could not stay pending has run by now and its
    # table is built the old way, from the compacted columns — except a
    # probe side that fell back for its width, which is a plain table now
    build = "l" if swap else "r"
    if not (fbuild and not materialize):  # else: the same question as above
        v = verdict(fprobe == "l" or fbuild == "l",
                    fprobe == "r" or fbuild == "r", n_l, n_r,
                    fprobe or (fbuild and ("r" if fbuild == "l" else "l")),
                    build)
    late_declined = bool(dropped) and dropped[-1] != wide
    from_cols = bool(v) and not late_declined and (
        group_join or fbuild is not None or not side[build].deferred
        or build == wide)
    if radix:
        return done("radix", from_cols, "fused")
    return done("fused", from_cols)
