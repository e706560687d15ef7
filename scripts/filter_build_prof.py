"""A pending build side built straight from its base columns against
filter-then-build, in one process (profiles/filter_build.json): the
measurement behind DSX_FILTERBUILD_MAX_ROWS (physical/filter_build.py).

A two-table inner join with a WHERE on both sides and a build-side value in
the SELECT, so that the fused probe's emit pass fetches the table:

    SELECT p.rid, b.bv FROM p JOIN b ON p.k = b.bk
    WHERE b.bsel < T AND p.f < 50

b has --bases rows (unique keys), p twice as many. T keeps 20 % or 1 % of b.
"on" lifts the cap and the row minimum (the table is sized by b's base rows,
its row ids index the base columns); "off" is DSX_DISABLE_FILTERBUILD=1 (filter, key pack, build over
the survivors). The radix gate is switched off for the whole run: at its
default it takes every join whose smaller base side has 8 M rows before
either path is asked.

Per configuration the results are compared first (same rows after sorting);
then 3 warm-ups, --reps timed steps (median and min wall ms) and one profiled
pass of 5 steps (HIP events: ms and launches per step per kernel family),
off, on, off, on so that drift shows between the repeats.

    python scripts/filter_build_prof.py [--reps R] [--bases N,N,N] [--out PATH]

The same run with small --bases (4096,16384,65536,262144) is the measurement
behind DSX_FILTERBUILD_MIN_ROWS (profiles/filter_build_small.json).
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from dask_sql_amd.context import Context  # noqa: E402

PROF_STEPS = 5
SQL = ("SELECT p.rid, b.bv FROM p JOIN b ON p.k = b.bk "
       "WHERE b.bsel < {t} AND p.f < 50")


def set_knob(off):
    os.environ.pop("DSX_DISABLE_FILTERBUILD", None)
    os.environ.pop("DSX_FILTERBUILD_MAX_ROWS", None)
    os.environ.pop("DSX_FILTERBUILD_MIN_ROWS", None)
    if off:
        os.environ["DSX_DISABLE_FILTERBUILD"] = "1"
    else:
        os.environ["DSX_FILTERBUILD_MAX_ROWS"] = str(1 << 40)
        os.environ["DSX_FILTERBUILD_MIN_ROWS"] = "0"


def measure(ctx, sql, off, warmup, reps):
    set_knob(off)
    r = ctx._get_runtime()
    for _ in range(warmup):
        ctx.sql(sql).compute()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.sql(sql).compute()
        wall.append(time.perf_counter() - t0)
    r.prof_enable(True)
    r.prof_reset()
    for _ in range(PROF_STEPS):
        ctx.sql(sql).compute()
    prof = r.prof_get()
    r.prof_enable(False)
    return {
        "step_ms_median": statistics.median(wall) * 1e3,
        "step_ms_min": min(wall) * 1e3,
        "kernel_ms_per_step": sum(v["ms"] for v in prof.values())
        / PROF_STEPS,
        "families": {k: {"ms_per_step": v["ms"] / PROF_STEPS,
                         "launches_per_step": v["launches"] / PROF_STEPS}
                     for k, v in sorted(prof.items())},
        "reps": reps, "warmup": warmup,
    }


def compare(ctx, sql):
    frames = []
    for off in (True, False):
        set_knob(off)
        f = ctx.sql(sql).compute()
        frames.append(f.sort_values("rid").reset_index(drop=True))
    assert len(frames[0]) == len(frames[1])
    for c in frames[0].columns:
        assert (frames[0][c].to_numpy() == frames[1][c].to_numpy()).all(), c
    return len(frames[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bases", default="1500000,6000000,15000000")
    ap.add_argument("--out", default=str(REPO / "profiles" /
                                         "filter_build.json"))
    args = ap.parse_args()
    os.environ["DSX_DISABLE_RADIX"] = "1"
    res = {"reps": args.reps, "sql": SQL, "radix": "off"}
    rng = np.random.default_rng(7)
    for nb in (int(x) for x in args.bases.split(",")):
        n_p = 2 * nb
        b = pd.DataFrame({
            "bk": rng.permutation(nb).astype(np.int64),
            "bsel": rng.integers(0, 100, nb).astype(np.int32),
            "bv": rng.integers(0, 1 << 40, nb).astype(np.int64)})
        p = pd.DataFrame({
            "rid": np.arange(n_p, dtype=np.int64),
            "k": rng.integers(0, nb, n_p).astype(np.int64),
            "f": rng.integers(0, 100, n_p).astype(np.int32)})
        c = Context()
        c.create_table("b", b, persist=True)
        c.create_table("p", p, persist=True)
        for label, t in (("sel_20pct", 20), ("sel_1pct", 1)):
            sql = SQL.format(t=t)
            entry = {"rows_out": compare(c, sql)}
            for tag, off in (("off", True), ("on", False), ("off_2", True),
                             ("on_2", False)):
                entry[tag] = measure(c, sql, off, args.warmup, args.reps)
                print(nb, label, tag, json.dumps(
                    {k: v for k, v in entry[tag].items() if k != "families"}),
                    flush=True)
            res[f"base_{nb}_{label}"] = entry
        del c, b, p
    set_knob(True)
    os.environ.pop("DSX_DISABLE_FILTERBUILD", None)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
