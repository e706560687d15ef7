#!/usr/bin/env python3
"""Host time of the join's routing in one TPC-H Q3 step: cProfile over one
warmed-up `Context.sql(Q3).compute()`, reporting the inclusive time of
DaskJoinPlugin.convert and DaskAggregatePlugin._try_group_join.

    python scripts/join_host_prof.py [--tree DIR] [--rows N] [--steps K]

--tree: the checkout to import dask_sql_amd from (default: this one), so two
trees are compared with one script. Prints one JSON line."""
import argparse
import cProfile
import json
import pstats
import sys
import time
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--rows", type=int, default=1_500_000, help="orders rows")
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()
sys.path.insert(0, str(Path(args.tree).resolve()))

from dask_sql_amd.context import Context  # noqa: E402
from datagen import Q3_SQL, gen_q3, register_q3_tables  # noqa: E402

n = args.rows
c = Context()
register_q3_tables(c, *gen_q3(sf_rows=(n // 10, n, 4 * n)))
for _ in range(5):
    c.sql(Q3_SQL).compute()
t0 = time.perf_counter()
for _ in range(args.steps):
    c.sql(Q3_SQL).compute()
wall = (time.perf_counter() - t0) / args.steps
prof = cProfile.Profile()
prof.enable()
for _ in range(args.steps):
    c.sql(Q3_SQL).compute()
prof.disable()
out = {"tree": args.tree, "orders_rows": n, "steps": args.steps,
       "ms_per_step_unprofiled": round(wall * 1e3, 4)}
from dask_sql_amd.physical.rel_plugins import (  # noqa: E402
    DaskAggregatePlugin, DaskJoinPlugin)

# by code object: other plugins have a `convert` in the same file
wanted = {}
for cls, names in ((DaskJoinPlugin, ("convert", "route", "settle")),
                   (DaskAggregatePlugin, ("_try_group_join",))):
    for name in names:
        code = getattr(getattr(cls, name, None), "__code__", None)
        if code is not None:
            wanted[(code.co_filename, code.co_firstlineno, name)] = \
                f"{cls.__name__}.{name}"
for key, (_, calls, _, cum, _) in pstats.Stats(prof).stats.items():
    if key in wanted:
        out[wanted[key]] = {"calls_per_step": calls / args.steps,
                            "cum_ms_per_step": round(cum / args.steps * 1e3,
                                                     4)}
print(json.dumps(out, sort_keys=True))
