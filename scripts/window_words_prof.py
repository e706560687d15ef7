"""Times window functions whose keys take the word front half (the
dsx_sort_word chain + dsx_window_mark_word + dsx_window_seg_ids) against the
host path those shapes took before it existed, at 5M rows on one GPU:

  sum_part_float  SUM(v) OVER (PARTITION BY p ORDER BY f)   f DOUBLE
  rownum_float    ROW_NUMBER() OVER (ORDER BY f)

    python scripts/window_words_prof.py [--rows N] [--parts P] [--reps R]
        [--host-reps H] [--parent-json PATH] [--out PATH]

For each query: warm-up runs, then the median wall time of Context.sql(...)
.compute() over repeated runs (compute() ends in a download, so the device
work is finished) — once by default (the word front half), once with
DSX_DISABLE_WINWORDS=1 (the host path) — and, from one extra profiled run
kept apart from the timed ones, the per-kernel HIP-event times of
prof_get(). The two paths' results are compared before anything is
reported. --parent-json embeds the output of the same script run on a
checkout of the parent commit, where the knob is unknown and both runs take
the host path. Needs a GPU; there is no fallback."""
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

KNOBS = ("DSX_DISABLE_WINWORDS", "DSX_WIN_WORDS", "DSX_DISABLE_DEVWINDOW")
QUERIES = {
    "sum_part_float": "SELECT rid, SUM(v) OVER (PARTITION BY p ORDER BY f) "
                      "AS w FROM tw",
    "rownum_float": "SELECT rid, ROW_NUMBER() OVER (ORDER BY f) AS w FROM tw",
}


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
    kernels = {k: {"ms": round(v["ms"], 4), "launches": v["launches"]}
               for k, v in sorted(prof.items())
               if k.startswith(("k_win_", "k_rsort_", "k_sort_"))}
    return out, {
        "env": env,
        "wall_ms": {"median": statistics.median(ms), "min": min(ms),
                    "max": max(ms), "runs": len(ms)},
        "kernels_ms": kernels,
        "window_kernels_total_ms": round(
            sum(v["ms"] for v in kernels.values()), 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--parts", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=str(
        REPO / "profiles" / "window_words.json"))
    args = ap.parse_args()

    n = args.rows
    rng = np.random.default_rng(61)
    df = pd.DataFrame({
        "p": rng.integers(0, args.parts, n).astype(np.int64),
        "f": rng.random(n),
        "v": rng.random(n),
        "rid": np.arange(n, dtype=np.int64)})
    ctx = Context()
    ctx.create_table("tw", df)

    result = {
        "shape": {"rows": n, "partitions": args.parts,
                  "keys": "int64 p, float64 f uniform [0,1)",
                  "value": "float64"},
        "method": "median wall ms of Context.sql().compute() (ends in a "
                  "device→host download); kernel ms = HIP events from "
                  "prof_get() in one separate profiled run",
        "queries": {},
    }
    for name, sql in QUERIES.items():
        dev, e_dev = measure(ctx, sql, {}, 2, args.reps)
        host, e_host = measure(ctx, sql, {"DSX_DISABLE_WINWORDS": "1"}, 1,
                               args.host_reps)
        d = dev.sort_values("rid")["w"].to_numpy(dtype=np.float64)
        h = host.sort_values("rid")["w"].to_numpy(dtype=np.float64)
        assert (np.isnan(d) == np.isnan(h)).all(), name
        np.testing.assert_allclose(np.nan_to_num(d), np.nan_to_num(h),
                                   rtol=1e-9, atol=1e-12)
        result["queries"][name] = {
            "sql": sql, "word_front_half": e_dev, "host_path": e_host,
            "speedup_median": e_host["wall_ms"]["median"]
            / e_dev["wall_ms"]["median"],
            "results_match_rtol": 1e-9}
        print(name, json.dumps(e_dev["wall_ms"]),
              json.dumps(e_host["wall_ms"]),
              json.dumps(e_dev["kernels_ms"]), flush=True)

    if args.parent_json:
        result["parent_commit"] = json.loads(
            Path(args.parent_json).read_text())["queries"]
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
