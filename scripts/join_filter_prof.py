"""Times the join key-membership filter (csrc/join_filter.h) where bench.py
cannot: on SPARSE join keys. bench.py's Q3 keys are dense (0..15M), so the
lineitem join always gets the exact bitmap; real TPC-H order keys are spread
by 4, which at SF10 makes the code range 60M and the exact bitmap 7.5 MB —
above the default cap, so the hashed mode decides there.

    python scripts/join_filter_prof.py [--reps R] [--spread S] [--out PATH]

One process, one context: Q3 (datagen.Q3_SQL) over gen_q3 tables with
o_orderkey and l_orderkey multiplied by --spread, under

  off           DSX_DISABLE_JOINFILTER=1
  default       nothing set (cap DSX_JOIN_FILTER_MAX_BYTES of join_filter.h)
  exact_8MiB    DSX_JOIN_FILTER_MAX_BYTES=8388608 (the 7.5 MB bitmap fits)
  hashed_1MiB   DSX_JOIN_FILTER_MAX_BYTES=1048576
  hashed_4MiB   DSX_JOIN_FILTER_MAX_BYTES=4194304
  off_again     the first configuration once more (drift of the session)

The knobs are read per call. For each: warm-up, the median wall time of
Context.sql(Q3).compute() over --reps runs, then — in separate profiled runs —
the HIP-event time per step of k_fprobe_mask (both launches), k_hash_build
and k_fprobe_emit, and which filter modes the step's two tables got
(Runtime.join_filter_builds). The results of all configurations are compared
with the first before anything is reported. Needs a GPU; no fallback."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from dask_sql_amd.context import Context  # noqa: E402
from datagen import Q3_SQL, gen_q3, register_q3_tables  # noqa: E402

KNOBS = ("DSX_DISABLE_JOINFILTER", "DSX_JOIN_FILTER_MAX_BYTES",
         "DSX_JOIN_FILTER_MIN_BITS")
CONFIGS = [
    ("off", {"DSX_DISABLE_JOINFILTER": "1"}),
    ("default", {}),
    ("exact_8MiB", {"DSX_JOIN_FILTER_MAX_BYTES": str(8 << 20)}),
    ("hashed_1MiB", {"DSX_JOIN_FILTER_MAX_BYTES": str(1 << 20)}),
    ("hashed_4MiB", {"DSX_JOIN_FILTER_MAX_BYTES": str(4 << 20)}),
    ("off_again", {"DSX_DISABLE_JOINFILTER": "1"}),
]
FAMILIES = ("k_fprobe_mask", "k_hash_build", "k_fprobe_emit")


def measure(ctx, env, warmup, reps):
    rt = ctx._get_runtime()
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        for _ in range(warmup):
            ctx.sql(Q3_SQL).compute()
        ms, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = ctx.sql(Q3_SQL).compute()
            ms.append((time.perf_counter() - t0) * 1e3)
        before = rt.join_filter_builds()
        rt.prof_enable(True)
        rt.prof_reset()
        for _ in range(reps):
            ctx.sql(Q3_SQL).compute()
        rt.synchronize()
        prof = rt.prof_get()
        rt.prof_enable(False)
        rt.prof_reset()
        builds = [a - b for a, b in zip(rt.join_filter_builds(), before)]
    finally:
        for k in env:
            os.environ.pop(k, None)
    return out, {
        "env": env,
        "wall_ms": {"median": round(statistics.median(ms), 4),
                    "min": round(min(ms), 4), "max": round(max(ms), 4),
                    "runs": len(ms)},
        "kernel_ms_per_step": {
            k: round(prof[k]["ms"] / reps, 4) for k in FAMILIES if k in prof},
        "all_kernels_ms_per_step": round(
            sum(v["ms"] for v in prof.values()) / reps, 4),
        "filtered_builds_per_step": {
            name: n / reps for name, n in zip(("none", "exact", "hashed"),
                                              builds)},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--spread", type=int, default=4)
    ap.add_argument("--out", default=str(
        REPO / "profiles" / "join_filter.json"))
    args = ap.parse_args()

    cust, orders, li = gen_q3()
    orders["o_orderkey"] *= args.spread
    li["l_orderkey"] *= args.spread
    ctx = Context()
    register_q3_tables(ctx, cust, orders, li)
    span = int(orders["o_orderkey"].max()) + 1
    result = {
        "shape": {"customer": len(cust), "orders": len(orders),
                  "lineitem": len(li), "key_spread": args.spread,
                  "lineitem_join_code_range": span,
                  "exact_bitmap_bytes": (span + 31) // 32 * 4},
        "method": "median wall ms of Context.sql(Q3).compute(); kernel ms = "
                  "HIP events from prof_get() over separate profiled runs, "
                  "per step (k_fprobe_mask: orders + lineitem launch)",
        "configs": {},
    }
    del cust, orders, li
    first = None
    for name, env in CONFIGS:
        out, entry = measure(ctx, env, 3, args.reps)
        if first is None:
            first = out
        for col in first.columns:
            a, b = first[col].to_numpy(), out[col].to_numpy()
            if np.issubdtype(a.dtype, np.datetime64):
                a, b = a.astype(np.int64), b.astype(np.int64)
            a, b = a.astype(np.float64), b.astype(np.float64)
            assert a.shape == b.shape and np.allclose(a, b, rtol=1e-12), \
                (name, col)
        result["configs"][name] = entry
        print(name, json.dumps(entry["wall_ms"]),
              json.dumps(entry["kernel_ms_per_step"]),
              json.dumps(entry["filtered_builds_per_step"]), flush=True)
    result["results_equal_across_configs"] = True
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
