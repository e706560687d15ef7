"""Times RANGE window frames with value offsets on the device path
(dsx_window_range) three ways, at 10M rows in 1 000 partitions:

- on the device;
- on the numpy host model (DSX_DISABLE_DEVWINDOW=1 —
  window_range.range_frames_host), the fallback and A/B partner;
- for keys that are dense and unique inside each partition, where an offset
  is a row distance, against the device ROWS frame of the same width
  (dsx_window_rows): what a frame of that width cost before RANGE existed.

    python scripts/window_range_prof.py [--rows N] [--parts P]
        [--reps R] [--host-reps H] [--out PATH]

Per query: warm-up runs, then the median wall time of Context.sql(...)
.compute() over repeated runs (compute() ends in a download, so the device
work is finished), and — from one extra profiled run, kept apart from the
timed ones — the per-kernel HIP-event times of prof_get(). Results are
compared before anything is reported (integer values: exact). Needs a GPU;
there is no fallback."""
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
from dask_sql_amd.physical import window_range as wrg  # noqa: E402

FRAMES = {
    "100_preceding_current": "BETWEEN 100 PRECEDING AND CURRENT ROW",
    "unbounded_preceding_100_following":
        "BETWEEN UNBOUNDED PRECEDING AND 100 FOLLOWING",
}
FUNCS = ("SUM", "MIN")


def timed(ctx, sql, warmup, reps):
    for _ in range(warmup):
        ctx.sql(sql).compute()
    times, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = ctx.sql(sql).compute()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def profiled(ctx, rt, sql):
    rt.prof_enable(True)
    rt.prof_reset()
    ctx.sql(sql).compute()
    prof = rt.prof_get()
    rt.prof_enable(False)
    return {k: {"ms": round(v["ms"], 4), "launches": v["launches"]}
            for k, v in sorted(prof.items())}


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms),
            "runs": len(ms)}


def column(df):
    return df.sort_values("rid")["s"].to_numpy(dtype=np.float64)


def same(a, b, what):
    assert (np.isnan(a) == np.isnan(b)).all(), what
    assert (np.nan_to_num(a) == np.nan_to_num(b)).all(), what


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--parts", type=int, default=1_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=str(
        REPO / "profiles" / "window_range_frames.json"))
    args = ap.parse_args()

    rng = np.random.default_rng(61)
    n = args.rows
    p = rng.integers(0, args.parts, n).astype(np.int64)
    # dense unique keys per partition: the row's rank in a random order
    order = np.lexsort((rng.random(n), p))
    head = np.flatnonzero(np.r_[True, p[order][1:] != p[order][:-1]])
    first = np.repeat(head, np.diff(np.r_[head, n]))
    dense = np.empty(n, dtype=np.int64)
    dense[order] = np.arange(n) - first
    df = pd.DataFrame({
        "p": p,
        "o": rng.integers(0, 2 * n // args.parts, n).astype(np.int64),
        "d": dense,
        "v": rng.integers(-1000, 1000, n).astype(np.int64),
        "rid": np.arange(n, dtype=np.int64)})
    ctx = Context()
    ctx.create_table("tr", df)
    rt = ctx._get_runtime()

    result = {
        "shape": {"rows": n, "partitions": args.parts,
                  "keys": "int64 p; int64 o with ties (about 2 rows per "
                          "key value and partition); int64 d dense and "
                          "unique inside each partition",
                  "value": "int64 in [-1000, 1000)"},
        "method": "median wall ms of Context.sql().compute() (ends in a "
                  "device→host download) after 2 warm-up runs; kernel ms = "
                  "HIP events from prof_get() in one separate profiled run; "
                  "host model: one run, no warm-up (numpy only)",
        "rmq_table_bytes": wrg.rmq_table_bytes(n),
        "queries": {},
    }
    for fname, frame in FRAMES.items():
        for func in FUNCS:
            name = f"{func.lower()}_{fname}"

            def sql(kind, key):
                return (f"SELECT rid, {func}(v) OVER (PARTITION BY p ORDER "
                        f"BY {key} {kind} {frame}) AS s FROM tr")

            os.environ.pop("DSX_DISABLE_DEVWINDOW", None)
            entry = {}
            # RANGE on keys with ties: device against the host model
            dev, dev_ms = timed(ctx, sql("RANGE", "o"), 2, args.reps)
            entry["range_ties"] = {
                "sql": sql("RANGE", "o"), "device_ms": stats(dev_ms),
                "device_kernels_ms": profiled(ctx, rt, sql("RANGE", "o"))}
            os.environ["DSX_DISABLE_DEVWINDOW"] = "1"
            try:
                host, host_ms = timed(ctx, sql("RANGE", "o"), 0,
                                      args.host_reps)
            finally:
                os.environ.pop("DSX_DISABLE_DEVWINDOW", None)
            same(column(dev), column(host), name + " device vs host model")
            entry["range_ties"]["host_model_ms"] = stats(host_ms)
            # dense unique keys: RANGE against ROWS of the same width,
            # alternating
            rng_ms, rows_ms = [], []
            timed(ctx, sql("RANGE", "d"), 2, 0)
            timed(ctx, sql("ROWS", "d"), 2, 0)
            for _ in range(args.reps):
                a, t = timed(ctx, sql("RANGE", "d"), 0, 1)
                rng_ms += t
                b, t = timed(ctx, sql("ROWS", "d"), 0, 1)
                rows_ms += t
            same(column(a), column(b), name + " RANGE vs ROWS")
            entry["dense_unique"] = {
                "range_sql": sql("RANGE", "d"), "rows_sql": sql("ROWS", "d"),
                "range_device_ms": stats(rng_ms),
                "rows_device_ms": stats(rows_ms),
                "range_kernels_ms": profiled(ctx, rt, sql("RANGE", "d")),
                "rows_kernels_ms": profiled(ctx, rt, sql("ROWS", "d"))}
            result["queries"][name] = entry
            print(name, "range/ties", json.dumps(stats(dev_ms)), "host model",
                  json.dumps(stats(host_ms)), "dense range",
                  json.dumps(stats(rng_ms)), "dense rows",
                  json.dumps(stats(rows_ms)), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
