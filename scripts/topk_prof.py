"""What the ORDER BY ... LIMIT tail costs per step, and how many host round
trips it makes (profiles/topk_select.json).

Two workloads, 30 timed steps after 3 warm-ups each:
- TPC-H Q3 SF10 (bench.py's default tables and query);
- a stand-alone 1.2 M-row frame, `SELECT a, r, d, p FROM t ORDER BY r DESC, d
  LIMIT 10` with r f64, once with DSX_DISABLE_TOPK=1 and once without (a tree
  that does not know the knob runs the same path twice).

Per workload: the median wall time of a step; then, in a second loop, the
median wall time of the Limit plugin's device top-k alone — the runtime is
synchronized before it, perf_counter wraps _device_topk_impl — and the
dsx_download / filter / gather / topk_rows calls made inside it per step.

    python scripts/topk_prof.py [--out profiles/topk_select.json]
"""
import argparse
import collections
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

import dask_sql_amd.physical.rel_plugins as rp  # noqa: E402
from dask_sql_amd.context import Context  # noqa: E402
from dask_sql_amd.runtime import Runtime  # noqa: E402
from datagen import Q3_SQL, gen_q3, register_q3_tables  # noqa: E402

STEPS, WARMUP = 30, 3
COUNTED = ("_download", "filter", "gather", "topk_rows")


class TailProbe:
    """Times _device_topk_impl and counts the runtime calls made inside."""

    def __init__(self):
        self.times = []
        self.calls = collections.Counter()
        self.inside = False
        self._orig_impl = rp._device_topk_impl
        self._orig = {}

    def __enter__(self):
        probe = self

        def impl(context, *a, **k):
            context._get_runtime().synchronize()
            probe.inside = True
            t0 = time.perf_counter()
            try:
                return probe._orig_impl(context, *a, **k)
            finally:
                probe.times.append(time.perf_counter() - t0)
                probe.inside = False

        rp._device_topk_impl = impl
        for name in COUNTED:
            orig = getattr(Runtime, name, None)
            if orig is None:
                continue
            self._orig[name] = orig

            def counted(self_, *a, _orig=orig, _name=name, **k):
                if probe.inside:
                    probe.calls[_name] += 1
                return _orig(self_, *a, **k)

            setattr(Runtime, name, counted)
        return self

    def __exit__(self, *exc):
        rp._device_topk_impl = self._orig_impl
        for name, orig in self._orig.items():
            setattr(Runtime, name, orig)


def measure(c, sql):
    for _ in range(WARMUP):
        c.sql(sql).compute()
    wall = []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        c.sql(sql).compute()
        wall.append(time.perf_counter() - t0)
    with TailProbe() as probe:
        for _ in range(STEPS):
            c.sql(sql).compute()
    per_step = {("dsx_download" if k == "_download" else k): v / STEPS
                for k, v in sorted(probe.calls.items())}
    return {
        "step_ms_median": statistics.median(wall) * 1e3,
        "step_ms_min": min(wall) * 1e3,
        "tail_ms_median": statistics.median(probe.times) * 1e3,
        "tail_ms_min": min(probe.times) * 1e3,
        "tail_calls_per_step": per_step,
        "steps": STEPS, "warmup": WARMUP,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" /
                                         "topk_select.json"))
    ap.add_argument("--skip-q3", action="store_true")
    args = ap.parse_args()
    res = {"has_topk_rows": hasattr(Runtime, "topk_rows")}

    n = 1_200_000
    rng = np.random.default_rng(12)
    df = pd.DataFrame({
        "a": np.arange(n, dtype=np.int64),
        "r": np.round(rng.random(n) * 5e5, 4),
        "d": (np.datetime64("1995-01-01")
              + rng.integers(0, 120, n).astype("timedelta64[D]")
              ).astype("datetime64[ns]"),
        "p": np.zeros(n, dtype=np.int32),
    })
    c = Context()
    c.create_table("t", df)
    sql = "SELECT a, r, d, p FROM t ORDER BY r DESC, d LIMIT 10"
    frames = {}
    for label, knob in (("frame_1p2m_knob_off", "1"),
                        ("frame_1p2m_knob_on", None)):
        if knob is None:
            os.environ.pop("DSX_DISABLE_TOPK", None)
        else:
            os.environ["DSX_DISABLE_TOPK"] = knob
        frames[label] = c.sql(sql).compute()
        res[label] = measure(c, sql)
        print(label, json.dumps(res[label]), flush=True)
    os.environ.pop("DSX_DISABLE_TOPK", None)
    pd.testing.assert_frame_equal(frames["frame_1p2m_knob_off"],
                                  frames["frame_1p2m_knob_on"])
    del c

    if not args.skip_q3:
        cust, orders, li = gen_q3()
        c = Context()
        register_q3_tables(c, cust, orders, li, persist=True)
        res["q3_sf10"] = measure(c, Q3_SQL)
        print("q3_sf10", json.dumps(res["q3_sf10"]), flush=True)

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
