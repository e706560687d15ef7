#!/usr/bin/env python3
"""Benchmark harness (driver contract).

`python bench.py --gpus N --steps K --warmup W` runs the hot-path query on N
GPUs of one node (launched by torch.distributed.run for N>1, one rank per
GPU over RCCL). A "step" = one pass of the hot path over the rank's batch.

Default workload = **TPC-H Q3 SF10** — the configuration BASELINE.json's
metric is quoted on; it fits one GPU (~2.3 GB), so it is the N=1 headline
(VERDICT r1 #1). The query text is the REAL Q3 ('BUILDING',
DATE '1995-03-15'); tables are registered with their real types
(dictionary-encoded mktsegment, DATE columns).

A plain run does only what the headline figure needs: generate + upload,
warm up, time K steps, print ONE JSON line (rank 0) with the contract
fields (`metric`, `value`, `unit`, `higher_is_better`, `dtype`,
`ms_per_step`, ...). `--dump-outputs DIR` additionally writes the result of
the last timed step (the frame `Context.sql(...).compute()` returns) as
`DIR/<NN>_<column>.npy`, float64; inputs are seeded, so two builds can be
compared output for output.

`--full` adds everything else to the same JSON line: a separate profiled
pass (`roofline`, `kernels`), `cpu_baseline` (the oracle timed on host cores
on a bounded sample — reported baseline, not the target) and, at N=1 on the
default workload, the C2 scan workload (BASELINE configs[1]) under
"secondary".

Roofline accounting: `roofline.frac` = whole-op
algorithmic bytes ÷ whole-op kernel time — the summed HIP-event time of
EVERY kernel a step launches, not the per-launch time of one family.
The dominant family's own per-launch numbers are reported under
`roofline.dominant` for kernel-level comparison against rocprof.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))

from datagen import Q1_SQL, Q3_SQL  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md spec peak (≈6300 achievable)

WORKLOADS = {
    "c2_filter_groupby_100m": {
        "rows": 100_000_000, "n_groups": 1_000_000,
        "sql": "SELECT key, SUM(x) AS s, COUNT(*) AS c FROM t "
               "WHERE x < 0.5 GROUP BY key",
        # algorithmic bytes = 16 B/row in + ~24 B/group out.
        # dominant = the fused-groupby kernel family (partition path:
        # hist+scatter+aggregate+finalize; fallback: the CAS kernel)
        "dominant": ["k_gbpart_hist", "k_gbpart_scatter",
                     "k_gbpart_aggregate", "k_gbpart_finalize",
                     "k_groupby_global"],
        "algo_bytes": lambda n, g: 16 * n + 24 * g,
        "scaling": "weak",
    },
    "c2_filter_groupby_100m_1kgroups": {
        "rows": 100_000_000, "n_groups": 1_000,
        "sql": "SELECT key, SUM(x) AS s, COUNT(*) AS c FROM t "
               "WHERE x < 0.5 GROUP BY key",
        "dominant": ["k_groupby_direct"],
        "algo_bytes": lambda n, g: 16 * n + 24 * g,
        "scaling": "weak",
    },
    "c3_join_100m_10m": {
        "rows": 100_000_000, "build_rows": 10_000_000,
        "sql": "SELECT p.key, p.pv, b.bv FROM probe_t p JOIN build_t b "
               "ON p.key = b.key",
        # 16 B/probe-row + 16 B/build-row + 24 B/match
        "dominant": ["k_hash_probe_mat", "k_hash_probe_emit",
                     "k_hash_probe_count", "k_hash_build"],
        "algo_bytes": lambda n, g: 16 * n + 16 * g + 24 * n,
        "scaling": "weak",
    },
    "q1_sf10": {
        "rows": 59_986_052,
        "sql": Q1_SQL,
        # ~38 B/row scanned
        "dominant": ["k_groupby_direct"],
        "algo_bytes": lambda n, g: 38 * n,
        "scaling": "strong",
    },
    "q3_sf10": {
        "rows": 60_000_000,  # lineitem; customer 1.5M + orders 15M extra
        "sql": Q3_SQL,
        "dominant": ["k_hash_probe_mat", "k_hash_probe_emit",
                     "k_hash_probe_count"],
        # whole-query algorithmic bytes, normalized per lineitem row:
        # lineitem 28 B/row (key 8 + extprice 8 + discount 8 + shipdate 4),
        # orders 24 B/row at n/4 rows, customer 9 B/row at n/40 rows
        "algo_bytes": lambda n, g: 28 * n + 24 * (n // 4) + 9 * (n // 40),
        "scaling": "strong",
    },
}


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(msg, file=sys.stderr, flush=True)


def make_context(workload, rank, world, device_id):
    import pandas as pd

    from dask_sql_amd.context import Context
    from datagen import (SEED, gen_c2, gen_c3, gen_lineitem_q1, gen_q3,
                         register_q1_table, register_q3_tables)

    c = Context(device_id=device_id)
    w = WORKLOADS[workload]
    seed = SEED + rank
    if workload.startswith("c2"):
        key, val = gen_c2(n=w["rows"], n_groups=w["n_groups"], seed=seed)
        c.create_table("t", pd.DataFrame({"key": key, "x": val}),
                       persist=True)
        total_rows = w["rows"]
    elif workload.startswith("c3"):
        bk, bv, pk, pv = gen_c3(n_build=w["build_rows"], n_probe=w["rows"],
                                seed=seed)
        c.create_table("probe_t", pd.DataFrame({"key": pk, "pv": pv}),
                       persist=True)
        c.create_table("build_t", pd.DataFrame({"key": bk, "bv": bv}),
                       persist=True)
        total_rows = w["rows"]
    elif workload == "q1_sf10":
        n = w["rows"] // world
        li = gen_lineitem_q1(n=n, seed=seed)
        register_q1_table(c, li, persist=True)
        total_rows = n
    elif workload == "q3_sf10":
        # strong scaling: each rank holds a row slice of the SF10 tables
        cust, orders, li = gen_q3(seed=SEED)
        if world > 1:
            cust = cust.iloc[rank::world].reset_index(drop=True)
            orders = orders.iloc[rank::world].reset_index(drop=True)
            li = li.iloc[rank::world].reset_index(drop=True)
        register_q3_tables(c, cust, orders, li, persist=True)
        total_rows = w["rows"] // world
    else:
        raise KeyError(workload)
    return c, total_rows


def run_step(c, workload, world, pg):
    """One pass of the hot path. Returns the result holder (device)."""
    w = WORKLOADS[workload]
    if workload == "q3_sf10" and world > 1:
        # distributed Q3: mid-pipeline RCCL repartition
        from dask_sql_amd.distributed import q3_distributed
        out = q3_distributed(c, pg)
        c._get_runtime().synchronize()
        return out
    res = c.sql(w["sql"])
    if world > 1 and workload.startswith(("c2", "q1")):
        # distributed partial-merge over RCCL: exchange partial
        # group rows by key hash, re-aggregate locally
        from dask_sql_amd.distributed import merge_groupby_partials
        dc = res.dc
        cc = dc.column_container
        cols = [dc.table.col(cc.get_backend_by_frontend_name(n))
                for n in cc.columns]
        runtime = c._get_runtime()
        if workload.startswith("c2"):
            key, vals, ops = cols[0], [cols[1], cols[2]], ["sum_f", "sum_i"]
        else:
            # Q1: composite dict keys, G ≤ 6 → host gather + weighted merge
            # (distributed.q1_merge_partials recombines AVG correctly)
            return _q1_allgather_merge(c, res, pg)
        mkey, mvals = merge_groupby_partials(runtime, key, vals, ops, pg)
        runtime.synchronize()
        return (mkey, mvals)
    runtime = c._get_runtime()
    runtime.synchronize()
    return res


def _q1_allgather_merge(c, res, pg):
    """Q1 partials are ≤ 12 rows — a host gather is the cheap correct merge
    (Q1 needs only a trivially small reduce). AVG columns
    recombine count-weighted (distributed.q1_merge_partials)."""
    import torch.distributed as dist

    from dask_sql_amd.distributed import q1_merge_partials
    pdf = res.compute()
    gathered = [None] * dist.get_world_size(pg)
    dist.all_gather_object(gathered, pdf, group=pg)
    return q1_merge_partials(gathered)


def cpu_baseline_leg(workload):
    """The oracle (CPU restatement, 'port') timed on host cores on a bounded
    sample — reported baseline only."""
    import multiprocessing as mp

    from datagen import gen_c2, gen_c3, gen_lineitem_q1

    cores = min(os.cpu_count() or 1, 16)
    if workload.startswith("c2"):
        w = WORKLOADS[workload]
        sample = 20_000_000
        key, val = gen_c2(n=sample, n_groups=w["n_groups"])
        chunks = np.array_split(np.arange(sample), cores)
        args = [(key[ix], val[ix]) for ix in chunks]
        t0 = time.perf_counter()
        with mp.Pool(cores) as pool:
            partials = pool.starmap(_oracle_c2_chunk, args)
        import pandas as pd
        allp = pd.concat(partials)
        allp.groupby("key", dropna=False).agg(
            s=("s", "sum"), c=("c", "sum"))
        dt = time.perf_counter() - t0
        return {"value": sample / dt, "unit": "rows/s", "cores": cores,
                "kind": "port",
                "sample": f"{sample} rows of the same distribution, "
                          f"{cores}-way chunked pandas (dask-equivalent "
                          f"chunk/agg tree)"}
    if workload.startswith("c3"):
        sample = 10_000_000
        bk, bv, pk, pv = gen_c3(n_build=1_000_000, n_probe=sample)
        from oracle.tpch import oracle_c3_join
        t0 = time.perf_counter()
        oracle_c3_join(bk, pk, bv, pv)
        dt = time.perf_counter() - t0
        return {"value": sample / dt, "unit": "rows/s", "cores": 1,
                "kind": "port", "sample": f"{sample} probe rows ⋈ 1M build"}
    if workload.startswith("q1"):
        sample = 10_000_000
        li = gen_lineitem_q1(n=sample)
        from oracle.tpch import oracle_q1
        t0 = time.perf_counter()
        oracle_q1(li)
        dt = time.perf_counter() - t0
        return {"value": sample / dt, "unit": "rows/s", "cores": 1,
                "kind": "port", "sample": f"{sample} lineitem rows"}
    if workload.startswith("q3"):
        from datagen import gen_q3
        cust, orders, li = gen_q3(sf_rows=(150_000, 1_500_000, 6_000_000))
        from oracle.tpch import oracle_q3
        t0 = time.perf_counter()
        oracle_q3(cust, orders, li)
        dt = time.perf_counter() - t0
        return {"value": 6_000_000 / dt, "unit": "rows/s (lineitem)",
                "cores": 1, "kind": "port", "sample": "SF1 synthetic Q3"}
    return None


def _oracle_c2_chunk(key, val):
    from oracle.tpch import oracle_c1_c2_groupby
    return oracle_c1_c2_groupby(key, val, predicate=True)


DUMP_BUDGET_BYTES = 64 * 1000 * 1000  # --dump-outputs writes at most this
DUMP_SAMPLE_SEED = 1234


def _as_float64(series):
    """One result column as float64: numbers as they are, dates/timestamps
    as ns since the epoch, strings as their rank among the column's sorted
    distinct values; NULL → NaN."""
    import pandas as pd

    arr = series.to_numpy()
    if np.issubdtype(arr.dtype, np.datetime64):
        ns = arr.astype("datetime64[ns]")
        out = ns.astype(np.int64).astype(np.float64)
        out[np.isnat(ns)] = np.nan
        return out
    if arr.dtype == object:
        null = pd.isna(series).to_numpy()
        out = np.full(len(arr), np.nan)
        if (~null).any():
            _, inv = np.unique(arr[~null].astype(str), return_inverse=True)
            out[~null] = inv
        return out
    return pd.to_numeric(series, errors="coerce").to_numpy(
        dtype=np.float64, na_value=np.nan)


def dump_outputs(result, workload, out_dir):
    """Write what the last timed step handed back — the frame a caller of
    the timed path receives — one float64 `<NN>_<column>.npy` per column.
    Queries without ORDER BY return rows in no fixed order, so their rows
    are sorted by all columns first; a result above the size budget is cut
    to a fixed seeded row sample (same rows for every build)."""
    import re

    import pandas as pd

    if hasattr(result, "compute"):
        pdf = result.compute()
    elif isinstance(result, pd.DataFrame):
        pdf = result
    else:  # (key, [values]) device columns of the distributed merge
        mkey, mvals = result
        pdf = pd.DataFrame({"key": mkey.to_numpy()[0]})
        for i, v in enumerate(mvals):
            pdf[f"val{i}"] = v.to_numpy()[0]
    cols = {f"{i:02d}_" + re.sub(r"[^A-Za-z0-9_.-]", "_", str(name)):
            _as_float64(pdf.iloc[:, i]) for i, name in enumerate(pdf.columns)}
    n = len(pdf)
    names = list(cols)
    if n and "ORDER BY" not in WORKLOADS[workload]["sql"].upper():
        order = np.lexsort([cols[k] for k in reversed(names)])
        cols = {k: v[order] for k, v in cols.items()}
    cap = DUMP_BUDGET_BYTES // (8 * max(1, len(names)))
    if n > cap:
        keep = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(
            n, size=cap, replace=False))
        cols = {k: v[keep] for k, v in cols.items()}
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    for k, v in cols.items():
        np.save(out_dir / f"{k}.npy", np.ascontiguousarray(v))
    log(f"[bench] wrote {len(names)} output columns "
        f"({min(n, cap)} of {n} rows) under {out_dir}")


def run_workload(workload, args, world, rank, local_rank, pg,
                 with_cpu_baseline, full, dump_dir=None):
    """Generate + upload, warm up, time K steps; return the metrics dict
    (rank 0) or None. `full` adds the profiled pass (roofline + per-kernel
    figures) and, with `with_cpu_baseline`, the CPU baseline leg."""
    import torch

    w = WORKLOADS[workload]
    log(f"[bench] generating + uploading {workload} (rank {rank}/{world})")
    c, rows_per_rank = make_context(workload, rank, world, local_rank)
    runtime = c._get_runtime()

    # warmup (also primes stat caches and the planner)
    for _ in range(args.warmup):
        run_step(c, workload, world, pg)
    runtime.synchronize()
    if torch.cuda.is_available():
        torch.cuda.synchronize(local_rank)

    # timed region runs WITHOUT per-kernel profiling (HIP event
    # create/record cost ~0.2 ms/step at Q3's ~44 launches); a separate
    # profiled pass afterwards provides the kernel breakdown
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    last = None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = None  # release the previous step's result before the next
        last = run_step(c, workload, world, pg)
    runtime.synchronize()
    if torch.cuda.is_available():
        torch.cuda.synchronize(local_rank)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=f"cuda:{local_rank}")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if dump_dir is not None and rank == 0:
        dump_outputs(last, workload, dump_dir)
    last = None

    ms_per_step = elapsed * 1000.0 / args.steps
    total_rows = rows_per_rank * world
    value = total_rows * args.steps / elapsed
    result = {
        "metric": "rows/s",
        "value": round(value, 1),
        "unit": "rows/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True,
        "scaling": w["scaling"],
        "vs_baseline": None,  # reference publishes no numbers
        "dtype": "f64",
        "data": "synthetic",
        "config": {
            "workload": workload,
            "rows_per_gpu": rows_per_rank,
            "n_groups": w.get("n_groups"),
            "sql": " ".join(w["sql"].split())[:160],
            "parallelism": f"dp{world}" if world > 1 else "single",
        },
    }
    if not full:
        return result if rank == 0 else None

    # profiled pass (same step count → same per-step kernel accounting)
    runtime.prof_enable(True)
    runtime.prof_reset()
    for _ in range(args.steps):
        run_step(c, workload, world, pg)
    runtime.synchronize()
    if torch.cuda.is_available():
        torch.cuda.synchronize(local_rank)
    prof = runtime.prof_get()
    runtime.prof_enable(False)

    if rank != 0:
        return None

    # Whole-op roofline: algorithmic bytes of one step ÷ the summed
    # HIP-event time of EVERY kernel that step launched (VERDICT r1 weak#4:
    # per-launch time of one family understates whole-query cost).
    g = w.get("n_groups", w.get("build_rows", 16))
    algo_bytes = float(w["algo_bytes"](rows_per_rank, g))
    kernel_ms_total = sum(v["ms"] for v in prof.values())
    kernel_ms_per_step = kernel_ms_total / args.steps if args.steps else 0.0
    roofline = None
    if kernel_ms_per_step > 0:
        achieved = algo_bytes / (kernel_ms_per_step / 1000.0) / 1e9  # GB/s
        traffic = None
        tf = REPO / "profiles" / f"traffic_{workload}.json"
        if tf.exists():
            traffic = json.loads(tf.read_text()).get("bytes_per_launch")
        dom = w["dominant"]
        present = [d for d in dom if d in prof and prof[d]["launches"] > 0]
        dominant = None
        if present:
            dom_ms_step = sum(prof[d]["ms"] for d in present) / args.steps
            dom_launch_ms = sum(prof[d]["ms"] / prof[d]["launches"]
                                for d in present)
            dominant = {
                "kernels": present,
                "ms_per_step": round(dom_ms_step, 4),
                "ms_per_launch": round(dom_launch_ms, 4),
                "achieved": round(
                    algo_bytes / (dom_ms_step / 1000.0) / 1e9, 1)
                if dom_ms_step else None,
            }
        roofline = {"bound": "hbm", "achieved": round(achieved, 1),
                    "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBPS, 4),
                    "traffic": traffic,
                    "kernel_ms_per_step": round(kernel_ms_per_step, 4),
                    "algo_bytes_per_step": algo_bytes,
                    "dominant": dominant}
    cpu_baseline = None
    if with_cpu_baseline:
        log("[bench] timing CPU baseline (oracle restatement)")
        cpu_baseline = cpu_baseline_leg(workload)

    result.update({
        "roofline": roofline,
        "cpu_baseline": cpu_baseline,
        "kernels": {k: {"ms_per_launch": round(v["ms"] / v["launches"], 4),
                        "launches": v["launches"]}
                    for k, v in sorted(prof.items())},
    })
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="q3_sf10",
                    help="headline default: TPC-H Q3 SF10 (BASELINE metric)")
    ap.add_argument("--full", action="store_true",
                    help="also run the profiled pass (roofline + per-kernel "
                         "figures), the CPU baseline and, at N=1 on the "
                         "default workload, the C2 secondary workload")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's result "
                         "columns as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the C2 secondary line at N=1")
    args = ap.parse_args()

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    if args.gpus > 1 and world == 1:
        print("launch N>1 via torch.distributed.run (driver contract)",
              file=sys.stderr)
        sys.exit(2)
    pg = None
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend="nccl")
        pg = dist.group.WORLD

    with_cpu = args.full and world == 1 and not args.no_cpu_baseline
    out = run_workload(args.workload, args, world, rank, local_rank, pg,
                       with_cpu, args.full, args.dump_outputs)

    # At N=1 a --full run of the default workload also measures the C2 scan
    # workload (BASELINE configs[1] — the single-GPU north-star kernel) and
    # attaches it to the same JSON line (driver contract: ONE line on stdout).
    if (args.full and world == 1 and args.workload == "q3_sf10"
            and not args.no_secondary):
        sec = run_workload("c2_filter_groupby_100m", args, world, rank,
                           local_rank, pg, with_cpu, True)
        if out is not None and sec is not None:
            out["secondary"] = {
                "workload": "c2_filter_groupby_100m",
                "value": sec["value"], "unit": sec["unit"],
                "ms_per_step": sec["ms_per_step"],
                "roofline": sec["roofline"],
                "cpu_baseline": sec["cpu_baseline"],
                "kernels": sec["kernels"],
            }

    if rank == 0 and out is not None:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
