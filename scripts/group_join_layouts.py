"""Group-join per accumulator record layout (profiles/group_join_layouts.json):
Q3 SF10 with its SUM (liveness sum), with MIN(l_extendedprice) (live byte)
and with AVG(l_extendedprice), COUNT(*) (row count in word 0), each with
DSX_DISABLE_GROUPJOIN=1 and without, and with DSX_DISABLE_JIT_FPROBE=1
(interpreter mask and accumulate kernels). 3 warm-ups, 20 timed steps (median
wall ms), 5 profiled steps (k_fprobe_agg and all kernels, ms per step).

    python scripts/group_join_layouts.py [OUT.json]
"""
import json, os, statistics, sys, time
from pathlib import Path
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from dask_sql_amd.context import Context
from datagen import gen_q3, register_q3_tables
T = """SELECT l_orderkey, {a}, o_orderdate, o_shippriority
 FROM customer, orders, lineitem
 WHERE c_mktsegment = 'BUILDING' AND c_custkey = o_custkey
 AND l_orderkey = o_orderkey AND o_orderdate < DATE '1995-03-15'
 AND l_shipdate > DATE '1995-03-15'
 GROUP BY l_orderkey, o_orderdate, o_shippriority
 ORDER BY v DESC, o_orderdate LIMIT 10"""
SHAPES = {"live_sum": "SUM(l_extendedprice*(1-l_discount)) AS v",
          "live_byte_min": "MIN(l_extendedprice) AS v",
          "row_count_avg": "AVG(l_extendedprice) AS v, COUNT(*) AS c"}
c = Context(); register_q3_tables(c, *gen_q3(), persist=True)
r = c._get_runtime(); res = {}
for name, a in SHAPES.items():
    sql = T.format(a=a)
    for tag, env in (("off", {"DSX_DISABLE_GROUPJOIN": "1"}), ("on_generated", {}), ("on_interpreter", {"DSX_DISABLE_JIT_FPROBE": "1"}), ("off_interp_mask", {"DSX_DISABLE_GROUPJOIN": "1", "DSX_DISABLE_JIT_FPROBE": "1"})):
        for k in ("DSX_DISABLE_GROUPJOIN", "DSX_DISABLE_JIT_FPROBE"): os.environ.pop(k, None)
        os.environ.update(env)
        for _ in range(3): c.sql(sql).compute()
        w = []
        for _ in range(20):
            t0 = time.perf_counter(); c.sql(sql).compute(); w.append(time.perf_counter() - t0)
        r.prof_enable(True); r.prof_reset()
        for _ in range(5): c.sql(sql).compute()
        p = r.prof_get(); r.prof_enable(False)
        res[f"{name}/{tag}"] = {"step_ms_median": round(statistics.median(w) * 1e3, 3),
                               "k_fprobe_agg_ms": round(p.get("k_fprobe_agg", {"ms": 0})["ms"] / 5, 4),
                               "kernel_ms": round(sum(v["ms"] for v in p.values()) / 5, 3)}
        print(name, tag, res[f"{name}/{tag}"], flush=True)
out = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "group_join_layouts.json"
out.write_text(json.dumps(res, indent=1) + "\n")
