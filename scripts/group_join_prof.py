"""Group-join against join-then-group-by on Q3 SF10, in one process
(profiles/group_join.json).

Q3's lineitem ⋈ orders join grouped by (l_orderkey, o_orderdate,
o_shippriority) runs either as one sweep that accumulates per build row
(Runtime.filter_probe_groupby) or, under DSX_DISABLE_GROUPJOIN=1, as the
fused filter-probe join followed by the partition group-by. Both are measured
on bench.py's tables, then once more with o_orderkey and l_orderkey multiplied
by --spread: the exact key bitmap no longer fits its cap and the mask pass
takes the hashed filter (scripts/join_filter_prof.py's second case).

Per configuration the results are compared first (keys, dates, priorities
equal; revenue within 16·2⁻⁵³ relative); then 3 warm-ups, --reps timed steps
(median and min wall ms) and one profiled pass of 5 steps (HIP events: ms and
launches per step of every kernel family that differs).

    python scripts/group_join_prof.py [--reps R] [--spread S] [--out PATH]
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

from dask_sql_amd.context import Context  # noqa: E402
from datagen import Q3_SQL, gen_q3, register_q3_tables  # noqa: E402

KNOB = "DSX_DISABLE_GROUPJOIN"
PROF_STEPS = 5
REL = 16 * 2.0 ** -53


def set_knob(off):
    if off:
        os.environ[KNOB] = "1"
    else:
        os.environ.pop(KNOB, None)


def measure(ctx, off, warmup, reps):
    set_knob(off)
    r = ctx._get_runtime()
    for _ in range(warmup):
        ctx.sql(Q3_SQL).compute()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.sql(Q3_SQL).compute()
        wall.append(time.perf_counter() - t0)
    r.prof_enable(True)
    r.prof_reset()
    for _ in range(PROF_STEPS):
        ctx.sql(Q3_SQL).compute()
    prof = r.prof_get()
    r.prof_enable(False)
    set_knob(False)
    fams = {k: {"ms_per_step": v["ms"] / PROF_STEPS,
                "launches_per_step": v["launches"] / PROF_STEPS}
            for k, v in sorted(prof.items())}
    return {
        "step_ms_median": statistics.median(wall) * 1e3,
        "step_ms_min": min(wall) * 1e3,
        "kernel_ms_per_step": sum(v["ms"] for v in prof.values())
        / PROF_STEPS,
        "families": fams, "reps": reps, "warmup": warmup,
    }


def compare(ctx):
    set_knob(True)
    off = ctx.sql(Q3_SQL).compute()
    set_knob(False)
    on = ctx.sql(Q3_SQL).compute()
    assert list(on.columns) == list(off.columns)
    assert len(on) == len(off)
    for c in on.columns:
        a, b = on[c].to_numpy(), off[c].to_numpy()
        if c == "revenue":
            rel = np.abs(a - b) / np.abs(b)
            assert (rel <= REL).all(), (c, rel.max())
        else:
            assert (a == b).all(), c
    return float((np.abs(on["revenue"].to_numpy() - off["revenue"].to_numpy())
                  / np.abs(off["revenue"].to_numpy())).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spread", type=int, default=4)
    ap.add_argument("--out", default=str(REPO / "profiles" /
                                         "group_join.json"))
    args = ap.parse_args()
    res = {"reps": args.reps, "key_spread": args.spread}
    cust, orders, li = gen_q3()
    for label, spread in (("q3_sf10", 1),
                          (f"q3_sf10_keys_x{args.spread}", args.spread)):
        if spread != 1:
            orders["o_orderkey"] *= spread
            li["l_orderkey"] *= spread
        c = Context()
        register_q3_tables(c, cust, orders, li, persist=True)
        entry = {"revenue_max_rel_diff": compare(c)}
        # off, on, off, on: drift shows as a difference between the repeats
        for tag, off in (("join_then_groupby", True), ("group_join", False),
                         ("join_then_groupby_2", True),
                         ("group_join_2", False)):
            entry[tag] = measure(c, off, args.warmup, args.reps)
            print(label, tag, json.dumps(
                {k: v for k, v in entry[tag].items() if k != "families"}),
                flush=True)
        res[label] = entry
        del c
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
