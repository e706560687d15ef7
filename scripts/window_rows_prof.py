"""Times explicit ROWS window frames on the device path against the host
rolling path (DSX_DISABLE_DEVWINDOW=1 — the behaviour before
dsx_window_rows existed), at the shape of the at-scale window test: 2M
rows, 50k partitions.

    python scripts/window_rows_prof.py [--rows N] [--parts P]
        [--reps R] [--host-reps H] [--out PATH]

For each frame: warm-up runs, then the median wall time of Context.sql(...)
.compute() over repeated runs (compute() ends in a download, so the device
work is finished), and — from one extra profiled run, kept apart from the
timed ones — the per-kernel HIP-event times of prof_get(). The two paths'
results are compared before anything is reported. Needs a GPU; there is no
fallback."""
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
from dask_sql_amd.physical import window_frames as wf  # noqa: E402

FRAMES = {
    "sum_2_preceding_current":
        "ROWS BETWEEN 2 PRECEDING AND CURRENT ROW",
    "sum_unbounded_preceding_current":
        "ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW",
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--parts", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=str(
        REPO / "profiles" / "window_rows_frames.json"))
    args = ap.parse_args()

    rng = np.random.default_rng(51)
    n = args.rows
    df = pd.DataFrame({
        "p": rng.integers(0, args.parts, n).astype(np.int64),
        "o": rng.integers(0, 10_000, n).astype(np.int64),
        "v": rng.random(n),
        "rid": np.arange(n, dtype=np.int64)})
    ctx = Context()
    ctx.create_table("tw", df)
    rt = ctx._get_runtime()

    result = {
        "shape": {"rows": n, "partitions": args.parts,
                  "keys": "int64 p, int64 o (ties within partitions)",
                  "value": "float64"},
        "method": "median wall ms of Context.sql().compute() (ends in a "
                  "device→host download); kernel ms = HIP events from "
                  "prof_get() in one separate profiled run",
        "thresholds": {"WIN_ROWS_DIRECT_MAXW": wf.WIN_ROWS_DIRECT_MAXW,
                       "WIN_ROWS_TILE_MAXW": wf.WIN_ROWS_TILE_MAXW,
                       "tuned": False},
        "frames": {},
    }
    for name, frame in FRAMES.items():
        sql = (f"SELECT rid, SUM(v) OVER (PARTITION BY p ORDER BY o {frame})"
               " AS s FROM tw")
        os.environ.pop("DSX_DISABLE_DEVWINDOW", None)
        dev, dev_ms = timed(ctx, sql, 2, args.reps)
        rt.prof_enable(True)
        rt.prof_reset()
        ctx.sql(sql).compute()
        prof = rt.prof_get()
        rt.prof_enable(False)
        os.environ["DSX_DISABLE_DEVWINDOW"] = "1"
        try:
            host, host_ms = timed(ctx, sql, 1, args.host_reps)
        finally:
            os.environ.pop("DSX_DISABLE_DEVWINDOW", None)
        dev = dev.sort_values("rid")["s"].to_numpy(dtype=np.float64)
        host = host.sort_values("rid")["s"].to_numpy(dtype=np.float64)
        assert (np.isnan(dev) == np.isnan(host)).all(), name
        np.testing.assert_allclose(np.nan_to_num(dev), np.nan_to_num(host),
                                   rtol=1e-9, atol=1e-12)
        entry = {
            "sql": sql,
            "device_ms": {"median": statistics.median(dev_ms),
                          "min": min(dev_ms), "max": max(dev_ms),
                          "runs": len(dev_ms)},
            "host_ms": {"median": statistics.median(host_ms),
                        "min": min(host_ms), "max": max(host_ms),
                        "runs": len(host_ms)},
            "speedup_median": statistics.median(host_ms)
            / statistics.median(dev_ms),
            "results_match_rtol": 1e-9,
            "device_kernels_ms": {
                k: {"ms": round(v["ms"], 4), "launches": v["launches"]}
                for k, v in sorted(prof.items())},
        }
        for k in ("k_win_rows_tile", "k_win_rows_prefix"):
            entry.setdefault("new_kernel_launched", {})[k] = \
                prof.get(k, {}).get("launches", 0)
        result["frames"][name] = entry
        print(name, json.dumps(entry["device_ms"]),
              json.dumps(entry["host_ms"]),
              f"speedup {entry['speedup_median']:.1f}x", flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
