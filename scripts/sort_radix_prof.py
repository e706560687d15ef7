"""Times ORDER BY through the radix sort chain (dsx_sort_word) against the
paths it complements, at 5M rows on one GPU:

  float   SELECT f, p FROM t ORDER BY f      (f64, uniform random)
          chain  vs  DSX_DISABLE_RADIXSORT=1 — the host path every float
          key took before dsx_sort_word existed (download + pandas
          mergesort)
  int2    the two-key integer query of test_device_general_sort_at_scale
          bucket path (dsx_sort_perm, the default)  vs  DSX_SORT_RADIX=1

    python scripts/sort_radix_prof.py [--rows N] [--reps R] [--host-reps H]
        [--parent-json PATH] [--out PATH]

For each: warm-up runs, then the median wall time of Context.sql(...)
.compute() over repeated runs (compute() ends in a download, so the device
work is finished), and — from one extra profiled run, kept apart from the
timed ones — the per-family HIP-event times of prof_get(). Results of the
two paths are compared before anything is reported. --parent-json embeds the
output of the same script run on a checkout of the parent commit (where both
knobs are unknown and the float query sorts on the host). Needs a GPU; there
is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import pandas as pd

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from dask_sql_amd.context import Context  # noqa: E402

KNOBS = ("DSX_DISABLE_RADIXSORT", "DSX_SORT_RADIX")


def timed(ctx, sql, warmup, reps):
    for _ in range(warmup):
        ctx.sql(sql).compute()
    times, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = ctx.sql(sql).compute()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def measure(ctx, sql, env, warmup, reps):
    rt = ctx._get_runtime()
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        out, ms = timed(ctx, sql, warmup, reps)
        rt.prof_enable(True)
        rt.prof_reset()
        ctx.sql(sql).compute()
        prof = rt.prof_get()
        rt.prof_enable(False)
        rt.prof_reset()
    finally:
        for k in env:
            os.environ.pop(k, None)
    sort_k = {k: {"ms": round(v["ms"], 4), "launches": v["launches"]}
              for k, v in sorted(prof.items())
              if k.startswith(("k_sort_", "k_rsort_", "k_gather"))}
    return out, {
        "env": env,
        "wall_ms": {"median": statistics.median(ms), "min": min(ms),
                    "max": max(ms), "runs": len(ms)},
        "kernels_ms": sort_k,
        "sort_kernels_total_ms": round(sum(
            v["ms"] for k, v in sort_k.items()
            if k.startswith(("k_sort_", "k_rsort_"))), 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=str(
        REPO / "profiles" / "sort_radix.json"))
    args = ap.parse_args()

    n = args.rows
    rng = np.random.default_rng(41)
    # int2: exactly the frame of test_device_general_sort_at_scale
    k1 = rng.integers(0, 50_000, n).astype(np.int64)
    k2 = pd.array(rng.integers(0, 100, n), dtype="Int64")
    k2[rng.choice(n, n // 1000, replace=False)] = None
    p = np.arange(n, dtype=np.int64)
    ctx = Context()
    ctx.create_table("ts", pd.DataFrame({"k1": k1, "k2": k2, "p": p}))
    ctx.create_table("tf", pd.DataFrame({"f": rng.random(n), "p": p}))

    result = {
        "shape": {"rows": n, "float": "f64 uniform [0,1), i64 payload",
                  "int2": "i64 k1 in [0,50000), nullable Int64 k2 in "
                          "[0,100), i64 payload"},
        "method": "median wall ms of Context.sql().compute() (ends in a "
                  "device→host download of the sorted frame); kernel ms = "
                  "HIP events from prof_get() in one separate profiled run",
        "queries": {},
    }

    sql = "SELECT f, p FROM tf ORDER BY f"
    dev, e_dev = measure(ctx, sql, {}, 2, args.reps)
    host, e_host = measure(ctx, sql, {"DSX_DISABLE_RADIXSORT": "1"}, 1,
                           args.host_reps)
    assert dev["p"].astype(np.int64).tolist() == \
        host["p"].astype(np.int64).tolist()
    result["queries"]["float"] = {
        "sql": sql, "radix_chain": e_dev, "host_path": e_host,
        "speedup_median": e_host["wall_ms"]["median"]
        / e_dev["wall_ms"]["median"],
        "results_identical": True}
    print("float", json.dumps(e_dev["wall_ms"]),
          json.dumps(e_host["wall_ms"]), flush=True)

    sql = "SELECT k1, k2, p FROM ts ORDER BY k1, k2 DESC"
    bucket, e_b = measure(ctx, sql, {}, 2, args.reps)
    radix, e_r = measure(ctx, sql, {"DSX_SORT_RADIX": "1"}, 2, args.reps)
    assert bucket["p"].astype(np.int64).tolist() == \
        radix["p"].astype(np.int64).tolist()
    result["queries"]["int2"] = {
        "sql": sql, "bucket_path": e_b, "radix_chain": e_r,
        "results_identical": True}
    print("int2", json.dumps(e_b["wall_ms"]), json.dumps(e_r["wall_ms"]),
          e_b["sort_kernels_total_ms"], e_r["sort_kernels_total_ms"],
          flush=True)

    if args.parent_json:
        result["parent_commit"] = json.loads(
            Path(args.parent_json).read_text())["queries"]
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
