"""Call-sequence characterisation of the join — test infrastructure only. A
fake runtime records what DaskJoinPlugin.convert and the aggregate's
group-join attempt (DaskAggregatePlugin._try_group_join) ask of the device
for a fixed list of cases over fake tables with preset statistics; no GPU, no
libdsxhip.so.

Run as a script it prints the traces as JSON:

    python tests/join_trace.py > tests/golden/join_trace.json

tests/test_join_trace.py replays the cases and compares with that file.

Per case the trace holds
  engine: in order, every run of a pending side's WHERE ("materialize", with
          its side) and every keypack / eval / hash_build / hash_build_cols /
          filter_probe_cols / filter_probe_groupby / hash_probe_cols /
          hash_probe / hash_unmatched / radix_join / filter / gather / upload
          / hash_table_free call with its columns, key specs, join type and
          flags, except
  setup:  the min-max calls and the dictionary remap's work (map upload,
          4-byte code upload, gather of the map through the codes), as a
          sorted set — a setup that is abandoned before a side runs its
          filter is not part of the contract;
  result: the output's column order, each column's source and the row count
          the fake reported, or the error raised.
"""
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from dask_sql_amd import runtime as rt  # noqa: E402
from dask_sql_amd.datacontainer import (ColumnContainer,  # noqa: E402
                                        DataContainer, DeferredFilter,
                                        DeviceTable)
from dask_sql_amd.physical.convert import RelConverter  # noqa: E402
from dask_sql_amd.physical.rel_plugins import (  # noqa: E402
    DaskAggregatePlugin, DaskJoinPlugin)
from dask_sql_amd.physical.rex import OP_COL, RexCompileError  # noqa: E402
from dask_sql_amd.planner.plan import (AggCall, AggregateNode,  # noqa: E402
                                       Call, Field, InputRef, JoinNode,
                                       Literal, LogicalPlan, RelDataType,
                                       SqlType)

KNOBS = ("DSX_DISABLE_RADIX", "DSX_RADIX_MIN_BUILD", "DSX_RADIX_MIN_PROBE",
         "DSX_DISABLE_JOINFUSE", "DSX_DISABLE_FILTERPROBE",
         "DSX_DISABLE_FILTERBUILD", "DSX_FILTERBUILD_MAX_ROWS",
         "DSX_FILTERBUILD_MIN_ROWS", "DSX_DISABLE_GROUPJOIN",
         "DSX_GROUPJOIN_MIN_ROWS")
N_OUT = 7       # rows every fused / pair probe reports
N_FILTER = 3    # rows every filter keeps
DICT = ["a", "b", "c"]


class FakeCol:
    """Stands in for a DeviceColumn: dtype, validity, len, a distinct `data`
    handle and, for base columns, preset statistics."""
    _next = [1000]

    def __init__(self, name, dtype, minmax=None, nullable=False,
                 dictionary=None, n=0, runtime=None):
        self.name = name
        self.dtype = dtype
        self.len = n
        self.rt = runtime
        FakeCol._next[0] += 16
        self.data = FakeCol._next[0] << 16
        self.validity = self.data + 1 if nullable else None
        if minmax is not None:
            self._minmax = minmax
        if dictionary is not None:
            self.dictionary = dictionary

    def to_numpy(self):
        return np.zeros(self.len, dtype=np.int64), None


class FakeRuntime:
    lib = None
    ctx = None
    GB_FIN_KINDS = rt.Runtime.GB_FIN_KINDS

    def __init__(self, refuse=(), raise_in=None, unmatched=0):
        self.calls = []
        self.refuse = set(refuse)
        self.raise_in = raise_in
        self.unmatched = unmatched
        self._by_data = {}
        self._uploads = {}
        self.tables = {}     # table id → what it was built from

    # ---- naming ----------------------------------------------------------
    def name(self, c):
        if c is None:
            return None
        nm = getattr(c, "name", None)
        if nm is not None:
            return nm
        ka = getattr(c, "_keep_alive", None)
        if isinstance(ka, tuple) and len(ka) == 4:
            # a build key remapped into the other side's dictionary:
            # (gather, source, map, codes)
            return f"remap({self.name(ka[1])})"
        if isinstance(ka, tuple) and len(ka) == 3:
            # one side's dense ids of a float key: (ids, lhs, rhs)
            side = "l" if c.data == ka[0].data else "r"
            return f"dense_{side}({self.name(ka[1])},{self.name(ka[2])})"
        hit = self._by_data.get(c.data)
        return hit.name if hit is not None else "?"

    def names(self, cols):
        return [self.name(c) for c in cols]

    def new(self, name, n, dtype=rt.I64, nullable=False):
        c = FakeCol(name, dtype, n=n, nullable=nullable, runtime=self)
        self._by_data[c.data] = c
        return c

    def _rec(self, call, **kw):
        rec = dict(call=call, **kw)
        self.calls.append(rec)
        if self.raise_in == call:
            raise rt.DsxError(f"injected failure in {call}")
        return rec

    @staticmethod
    def _specs(specs):
        return [list(s) for s in specs]

    @staticmethod
    def _prog(prog):
        return None if prog is None else [list(p) for p in prog]

    def _outs(self, srcs, n):
        return [self.new(f"out({self.name(c)})", n, c.dtype,
                         bool(c.validity)) for c in srcs]

    # ---- the Runtime surface the join uses -------------------------------
    @staticmethod
    def make_prog(instrs):
        return None if instrs is None else tuple(tuple(i) for i in instrs)

    def upload_column(self, arr, validity=None, dtype=None):
        arr = np.asarray(arr)
        rec = self._rec("upload", n=len(arr), dtype=dtype)
        c = self.new("upload", len(arr), dtype if dtype is not None
                     else rt.I64)
        self._uploads[c.data] = rec
        return c

    def empty_column(self, n, dtype, with_validity=False):
        return self.new("empty", n, dtype)

    def gather(self, col, sel_ptr, n, force_validity=False):
        through = self._by_data.get(sel_ptr)
        rec = self._rec("gather", col=self.name(col),
                        through=self.name(through), n=n,
                        force_validity=bool(force_validity))
        up, up_codes = self._uploads.get(col.data), self._uploads.get(sel_ptr)
        if up is not None and (
                up_codes is not None
                or getattr(through, "dictionary", None) is not None):
            # a code→code map gathered through dictionary codes: the remap
            for r in (rec, up, up_codes):
                if r is not None:
                    r["setup"] = True
        return self.new(f"gather({self.name(col)})", n, col.dtype,
                        force_validity or bool(col.validity))

    def minmax_i64(self, col):
        self._rec("minmax", col=self.name(col), setup=True)
        return (0, 9, col.len)

    def keypack(self, cols, specs, n):
        self._rec("keypack", cols=self.names(cols), specs=self._specs(specs),
                  n=n)
        space = 1
        for s in specs:
            space *= max(s[2], 1)
        return self.new(f"codes({','.join(self.name(cols[s[0]]) for s in specs)})",
                        n), space

    def eval(self, prog, cols, n, out_dtype, with_validity=True):
        self._rec("eval", prog=self._prog(prog), cols=self.names(cols), n=n,
                  with_validity=bool(with_validity))
        return self.new("eval", n, out_dtype)

    def _table(self, what):
        tid = f"T{len(self.tables) + 1}"
        self.tables[tid] = what
        return tid

    def hash_build(self, codes, validity_ptr=None, code_max=0,
                   key_filter=False):
        tid = self._table(self.name(codes))
        self._rec("hash_build", table=tid, codes=self.name(codes),
                  validity=validity_ptr is not None, code_max=code_max,
                  key_filter=bool(key_filter))
        return tid

    def hash_build_cols(self, prog, cols, keyspecs, n, code_max=0,
                        key_filter=False):
        tid = self._table("cols")
        self._rec("hash_build_cols", table=tid, prog=self._prog(prog),
                  cols=self.names(cols), specs=self._specs(keyspecs), n=n,
                  code_max=code_max, key_filter=bool(key_filter))
        return tid

    def hash_table_free(self, table):
        self._rec("hash_table_free", table=table)

    def filter_probe_cols(self, table, prog, cols, keyspecs, n, pcols, bcols):
        self._rec("filter_probe_cols", table=table, prog=self._prog(prog),
                  cols=self.names(cols), specs=self._specs(keyspecs), n=n,
                  pcols=self.names(pcols), bcols=self.names(bcols))
        if "filter_probe_cols" in self.refuse:
            return None
        return self._outs(list(pcols) + list(bcols), N_OUT), N_OUT

    def filter_probe_groupby(self, table, prog, cols, keyspecs, n, agg_specs,
                             calls, kcols):
        self._rec("filter_probe_groupby", table=table, prog=self._prog(prog),
                  cols=self.names(cols), specs=self._specs(keyspecs), n=n,
                  aggs=[[op, self._prog(p)] for op, p in agg_specs],
                  calls=[list(c) for c in calls], kcols=self.names(kcols))
        if "filter_probe_groupby" in self.refuse:
            return None
        return (self._outs(kcols, 5),
                [self.new(f"agg{i}", 5) for i in range(len(calls))], 5)

    def hash_probe_cols(self, table, codes, join_type, validity_ptr, pcols,
                        bcols, force_build_validity):
        self._rec("hash_probe_cols", table=table, codes=self.name(codes),
                  join_type=join_type, validity=validity_ptr is not None,
                  pcols=self.names(pcols), bcols=self.names(bcols),
                  force_build_validity=bool(force_build_validity))
        return self._outs(list(pcols) + list(bcols), N_OUT), N_OUT

    def hash_probe(self, table, codes, join_type, validity_ptr=None,
                   mark_matched=False):
        self._rec("hash_probe", table=table, codes=self.name(codes),
                  join_type=join_type, validity=validity_ptr is not None,
                  mark_matched=bool(mark_matched))
        # the float-key densification probes every row into its own group
        n = codes.len if self.tables[table] == "groups" else N_OUT
        return (self.new("probe_sel", n, rt.I32).data,
                self.new("build_sel", n, rt.I32).data, n)

    def hash_unmatched(self, table):
        self._rec("hash_unmatched", table=table)
        return self.new("unmatched", self.unmatched, rt.I32).data, \
            self.unmatched

    def radix_join(self, bcols, n_build, keyspecs_b, keyspecs_p, bpred_prog,
                   pcols, n_probe, join_type, out_specs):
        self._rec("radix_join", bcols=self.names(bcols), n_build=n_build,
                  specs_b=self._specs(keyspecs_b),
                  specs_p=self._specs(keyspecs_p),
                  bpred=self._prog(bpred_prog), pcols=self.names(pcols),
                  n_probe=n_probe, join_type=join_type,
                  out_specs=self._specs(out_specs))
        if "radix_join" in self.refuse:
            return None
        srcs = [(pcols if side == 0 else bcols)[ci]
                for side, ci, _ in out_specs]
        return self._outs(srcs, N_OUT), N_OUT

    def filter(self, prog, cols, n):
        self._rec("filter", prog=self._prog(prog), cols=self.names(cols), n=n)
        return self.new("filter_sel", N_FILTER, rt.I32).data, N_FILTER

    def wrap_sel(self, sel_ptr, count):
        c = self._by_data[sel_ptr]
        assert c.len == count, (c.name, c.len, count)
        return c

    def concat_columns(self, cols, dtype):
        return self.new(f"concat({','.join(self.names(cols))})",
                        sum(c.len for c in cols), dtype)

    def hash_groupby(self, cols, n, keyspecs, pred_prog, agg_specs):
        return self.new("groups", 5).data, 0, 0, 5

    def scatter_rows(self, col, sel_ptr, n_sel, n_out, with_validity=True):
        return self.new("ids", n_out, rt.I32)

    def _free(self, ptr):
        pass

    def _download(self, ptr, out):
        out[:] = 0

    # ---- the trace -------------------------------------------------------
    def trace(self):
        engine = [c for c in self.calls if not c.get("setup")]
        setup = sorted({json.dumps(c, sort_keys=True)
                        for c in self.calls if c.get("setup")})
        return engine, [json.loads(s) for s in setup]


# ---- fake tables --------------------------------------------------------
def side_table(runtime, prefix, n, dictionary=DICT, float_key=False,
               extra=0, null_key=False, wide_codes=False):
    """One input: k (the first join key), d (a dictionary column), f (a
    float column), x, y (nullable) and `extra` more integer columns."""
    lo = 0 if prefix == "L" else 10
    cols = [
        FakeCol(f"{prefix}.k", rt.F64 if float_key else rt.I64,
                None if float_key else (lo, lo + 99, n - 2 if null_key else n),
                nullable=null_key),
        FakeCol(f"{prefix}.d", rt.I64 if wide_codes else rt.I32,
                (0, len(dictionary) - 1, n), nullable=True,
                dictionary=dictionary),
        FakeCol(f"{prefix}.f", rt.F64),
        FakeCol(f"{prefix}.x", rt.I64, (1, 5, n)),
        FakeCol(f"{prefix}.y", rt.I64, (-3, 3, n - 1), nullable=True),
    ] + [FakeCol(f"{prefix}.e{i}", rt.I64, (0, 1, n)) for i in range(extra)]
    for c in cols:
        c.len = n
        c.rt = runtime
        runtime._by_data[c.data] = c
    names = [c.name for c in cols]
    return DataContainer(DeviceTable(dict(zip(names, cols))),
                         ColumnContainer(names))


K, D, F, X, Y, E0 = range(6)


def pending(runtime, dc, side, prog_cols):
    """dc under a WHERE that has not run; running it is recorded."""
    cols = dc.backend_cols()

    def materialize(d):
        runtime._rec("materialize", side=side)
        out = {}
        for name, src in d.base.table.columns.items():
            c = runtime.new(name + "'", N_FILTER, src.dtype,
                            bool(src.validity))
            if getattr(src, "dictionary", None) is not None:
                c.dictionary = src.dictionary
            c._stats_src = src
            out[name] = c
        return DeviceTable(out, num_rows=N_FILTER)

    prog = [(OP_COL, i, 0) for i in range(len(prog_cols))]
    return DeferredFilter(dc, dc.column_container, prog,
                          [cols[i] for i in prog_cols], materialize)


def _plan(node_type, inputs, names, payload):
    return LogicalPlan(node_type, inputs, RelDataType(
        [Field(n, SqlType("BIGINT")) for n in names]), payload)


class _TraceInputPlugin:
    """Plan leaf of the group-join cases: hands back a prepared container."""

    def convert(self, rel, context):
        return rel._payload


BIGINT = SqlType("BIGINT")


def _eq(i, j):
    return Call("=", [InputRef(i, BIGINT), InputRef(j, BIGINT)])


def _residual(kind, n_l):
    if kind == "lt":     # L.x < R.x
        return Call("<", [InputRef(X, BIGINT), InputRef(n_l + X, BIGINT)])
    if kind == "false":
        return Literal(False, SqlType("BOOLEAN"))
    raise KeyError(kind)


# (name, options). Options: jt (plan join type), n_l / n_r (rows), on (key
# pairs, side-local columns), pend {side: predicate columns}, out (output
# indices), residual, dict_r / wide_codes_r (the rhs dictionary), float_l /
# float_r, extra_l / extra_r, null_key, null_equal, null_aware, env, refuse,
# raise_in, unmatched; group (the aggregate over the join): build (the side
# whose key it groups by), probe_col (group by a probe-side column too).
FB0 = {"DSX_FILTERBUILD_MIN_ROWS": "0"}
GJ0 = {"DSX_GROUPJOIN_MIN_ROWS": "0"}
RADIX = {"DSX_RADIX_MIN_BUILD": "50", "DSX_RADIX_MIN_PROBE": "50"}
WIDE = list(range(E0, E0 + 16))  # 16 predicate columns, the key not among
CASES = [
    ("inner_l_larger", dict(jt="INNER", n_l=400, n_r=100)),
    ("inner_l_smaller", dict(jt="INNER", n_l=100, n_r=400)),
    ("left", dict(jt="LEFT")),
    ("right", dict(jt="RIGHT")),
    ("leftanti", dict(jt="LEFTANTI")),
    ("leftsemi_unpruned", dict(jt="LEFTSEMI")),
    ("leftsemi_pruned", dict(jt="LEFTSEMI", out=[K, X])),
    ("inner_build_cols", dict(jt="INNER", env=FB0)),
    ("left_build_cols", dict(jt="LEFT", env=FB0)),
    ("two_keys_nullable", dict(jt="INNER", on=[(K, K), (Y, Y)], env=FB0)),
    ("pend_lhs_smaller", dict(jt="INNER", n_l=100, n_r=400,
                              pend={"l": [X]})),
    ("pend_rhs_smaller", dict(jt="INNER", n_l=400, n_r=100,
                              pend={"r": [X]})),
    ("pend_probe_l", dict(jt="INNER", n_l=400, n_r=100, pend={"l": [X, K]})),
    ("pend_probe_r", dict(jt="INNER", n_l=100, n_r=400, pend={"r": [X]})),
    ("pend_probe_r_build_cols", dict(jt="INNER", n_l=100, n_r=400,
                                     pend={"r": [X]}, env=FB0)),
    ("pend_build_above_min", dict(jt="INNER", n_l=100, n_r=400,
                                  pend={"l": [X]}, env=FB0)),
    ("pend_build_above_max", dict(
        jt="INNER", n_l=100, n_r=400, pend={"l": [X]},
        env={**FB0, "DSX_FILTERBUILD_MAX_ROWS": "50"})),
    ("pend_both", dict(jt="INNER", n_l=100, n_r=400,
                       pend={"l": [X], "r": [Y, X]})),
    ("pend_both_build_cols", dict(jt="INNER", n_l=100, n_r=400,
                                  pend={"l": [X], "r": [Y, X]}, env=FB0)),
    ("pend_both_key_in_pred", dict(jt="INNER", n_l=400, n_r=100,
                                   pend={"l": [K], "r": [K, X]}, env=FB0)),
    ("pend_build_left", dict(jt="LEFT", pend={"r": [X]}, env=FB0)),
    ("pend_build_right", dict(jt="RIGHT", pend={"l": [X]}, env=FB0)),
    ("pend_build_anti", dict(jt="LEFTANTI", pend={"r": [X]}, env=FB0)),
    ("pend_probe_left", dict(jt="LEFT", pend={"l": [X]}, env=FB0)),
    ("dict_same", dict(jt="INNER", on=[(D, D)])),
    ("dict_equal_list", dict(jt="INNER", on=[(D, D)], dict_r=list(DICT))),
    ("dict_other_on_build", dict(jt="INNER", on=[(D, D)], n_l=400, n_r=100,
                                 dict_r=["c", "a", "q"], env=FB0)),
    ("dict_other_on_probe", dict(jt="INNER", on=[(D, D)], n_l=100, n_r=400,
                                 dict_r=["c", "a", "q"], env=FB0)),
    ("dict_other_wide_codes", dict(jt="LEFT", on=[(D, D)],
                                   dict_r=["c", "a", "q"],
                                   wide_codes_r=True)),
    ("dict_other_pend_build", dict(jt="INNER", on=[(D, D)], n_l=400, n_r=100,
                                   dict_r=["c", "a", "q"], pend={"r": [X]},
                                   env=FB0)),
    ("dict_other_pend_probe_swapped", dict(
        jt="INNER", on=[(D, D)], n_l=100, n_r=400, dict_r=["c", "a", "q"],
        pend={"r": [X]}, env=FB0)),
    ("dict_vs_plain", dict(jt="INNER", on=[(D, X)])),
    ("float_key", dict(jt="INNER", float_l=True, float_r=True)),
    ("float_key_pending", dict(jt="INNER", float_l=True, float_r=True,
                               n_l=100, n_r=400, pend={"l": [X], "r": [X]},
                               env=FB0)),
    # the side taken at first runs its WHERE last: rhs before lhs
    ("float_key_pending_l_larger", dict(
        jt="INNER", float_l=True, float_r=True, n_l=400, n_r=100,
        pend={"l": [X], "r": [X]})),
    ("wide_probe_l_17_pend_r", dict(
        jt="INNER", n_l=400, n_r=100, extra_l=16,
        pend={"l": WIDE, "r": [X]}, out=[K, X, 21 + K])),
    ("radix_pending_l_larger", dict(jt="INNER", n_l=400, n_r=100,
                                    pend={"l": [X], "r": [X]}, env=RADIX)),
    ("mixed_int_float_key", dict(jt="INNER", float_r=True)),
    ("wide_output_17", dict(jt="INNER", extra_l=4, extra_r=3)),
    ("wide_probe_17", dict(jt="INNER", n_l=100, n_r=400, extra_r=16,
                           pend={"r": WIDE}, out=[K, X, 5 + K], env=FB0)),
    ("wide_probe_17_pend_build", dict(
        jt="INNER", n_l=100, n_r=400, extra_r=16,
        pend={"l": [X], "r": WIDE}, out=[K, X, 5 + K], env=FB0)),
    ("wide_probe_17_pend_build_larger", dict(
        jt="INNER", n_l=400, n_r=100, extra_l=16,
        pend={"l": WIDE, "r": [X]}, out=[K, X, 21 + K], env=FB0)),
    ("wide_build_17", dict(jt="INNER", n_l=400, n_r=100, extra_r=16,
                           pend={"r": WIDE}, out=[K, X, 5 + K], env=FB0)),
    ("dup_keys", dict(jt="INNER", n_l=100, n_r=400, pend={"r": [X]},
                      refuse=["filter_probe_cols"])),
    ("dup_keys_probe_l", dict(jt="INNER", n_l=400, n_r=100, pend={"l": [X]},
                              refuse=["filter_probe_cols"], env=FB0)),
    ("dup_keys_dict_swapped", dict(
        jt="INNER", on=[(D, D)], n_l=100, n_r=400, dict_r=["c", "a", "q"],
        pend={"r": [X]}, refuse=["filter_probe_cols"])),
    ("dup_keys_pend_build", dict(
        jt="INNER", n_l=100, n_r=400, pend={"l": [X], "r": [X]},
        refuse=["filter_probe_cols"], env=FB0)),
    ("radix", dict(jt="INNER", n_l=100, n_r=400, env=RADIX)),
    ("radix_left_nullable", dict(jt="LEFT", on=[(K, K), (Y, Y)], env=RADIX)),
    ("radix_right_dict", dict(jt="RIGHT", on=[(D, D)],
                              dict_r=["c", "a", "q"], env=RADIX)),
    ("radix_pending", dict(jt="INNER", n_l=100, n_r=400,
                           pend={"l": [X], "r": [X]}, env=RADIX)),
    ("radix_probe_too_small", dict(
        jt="INNER", n_l=100, n_r=400,
        env={"DSX_RADIX_MIN_BUILD": "50", "DSX_RADIX_MIN_PROBE": "500"})),
    ("radix_declines", dict(jt="INNER", n_l=100, n_r=400, env=RADIX,
                            refuse=["radix_join"])),
    ("radix_float_key", dict(jt="INNER", float_l=True, float_r=True,
                             env=RADIX)),
    ("residual_inner", dict(jt="INNER", residual="lt")),
    ("residual_inner_pruned", dict(jt="INNER", residual="lt", out=[K, 5 + K],
                                   pend={"l": [X]})),
    ("residual_anti", dict(jt="LEFTANTI", residual="lt")),
    ("residual_false", dict(jt="INNER", residual="false")),
    ("residual_false_anti", dict(jt="LEFTANTI", residual="false")),
    ("outer_unmatched", dict(jt="FULL", unmatched=2)),
    ("outer_all_matched", dict(jt="FULL", null_key=True)),
    ("outer_pending", dict(jt="FULL", pend={"l": [X], "r": [X]}, env=FB0)),
    ("null_equal", dict(jt="LEFTSEMI", null_equal=True, null_key=True,
                        out=[K, X])),
    ("null_equal_anti", dict(jt="LEFTANTI", null_equal=True, null_key=True)),
    ("null_aware_anti_null", dict(jt="LEFTANTI", null_aware=True,
                                  null_key=True, out=[K, D])),
    ("null_aware_anti_no_null", dict(jt="LEFTANTI", null_aware=True)),
    ("cross", dict(jt="CROSS", on=[], n_l=3, n_r=2)),
    ("cross_pending", dict(jt="INNER", on=[], n_l=3, n_r=2,
                           pend={"l": [X]})),
    ("no_radix", dict(jt="INNER", n_l=100, n_r=400,
                      env={**RADIX, "DSX_DISABLE_RADIX": "1"})),
    ("no_radix_pending", dict(
        jt="INNER", n_l=100, n_r=400, pend={"l": [X], "r": [X]},
        env={**RADIX, **FB0, "DSX_DISABLE_RADIX": "1"})),
    ("no_joinfuse", dict(jt="INNER", pend={"l": [X]},
                         env={"DSX_DISABLE_JOINFUSE": "1"})),
    ("no_joinfuse_radix", dict(jt="INNER", n_l=100, n_r=400,
                               env={**RADIX, "DSX_DISABLE_JOINFUSE": "1"})),
    ("no_filterprobe", dict(jt="INNER", n_l=100, n_r=400,
                            pend={"l": [X], "r": [X]},
                            env={**FB0, "DSX_DISABLE_FILTERPROBE": "1"})),
    ("no_filterbuild", dict(jt="INNER", n_l=100, n_r=400,
                            pend={"l": [X], "r": [X]},
                            env={**FB0, "DSX_DISABLE_FILTERBUILD": "1"})),
    ("filterbuild_knobs_garbage", dict(
        jt="INNER", n_l=100, n_r=400, pend={"l": [X], "r": [X]},
        env={"DSX_FILTERBUILD_MIN_ROWS": "x",
             "DSX_FILTERBUILD_MAX_ROWS": "y"})),
    ("raise_hash_probe_cols", dict(jt="INNER", raise_in="hash_probe_cols")),
    ("raise_filter_probe_cols", dict(jt="INNER", n_l=100, n_r=400,
                                     pend={"r": [X]}, env=FB0,
                                     raise_in="filter_probe_cols")),
    ("raise_hash_probe", dict(jt="FULL", raise_in="hash_probe")),
    ("raise_keypack_after_dup", dict(jt="INNER", n_l=100, n_r=400,
                                     pend={"r": [X]}, env=FB0,
                                     refuse=["filter_probe_cols"],
                                     raise_in="keypack")),
    # the aggregate's group-join over the join (Q3's shape)
    ("gj_accepted", dict(jt="INNER", n_l=100, n_r=400, pend={"r": [Y]},
                         group={}, env=GJ0)),
    ("gj_accepted_build_cols", dict(jt="INNER", n_l=100, n_r=400,
                                    pend={"r": [Y]}, group={},
                                    env={**GJ0, **FB0})),
    ("gj_pend_both", dict(jt="INNER", n_l=100, n_r=400,
                          pend={"l": [X], "r": [Y]}, group={},
                          env={**GJ0, **FB0})),
    ("gj_probe_l", dict(jt="INNER", n_l=400, n_r=100, pend={"l": [Y]},
                        group={"build": "r"}, env={**GJ0, **FB0})),
    ("gj_declined_verdict", dict(jt="INNER", n_l=100, n_r=400,
                                 pend={"r": [Y]}, group={"probe_col": True},
                                 env={**GJ0, **FB0})),
    ("gj_pend_both_keypack", dict(jt="INNER", n_l=100, n_r=400,
                                  pend={"l": [X], "r": [Y]}, group={},
                                  env=GJ0)),
    ("gj_wide_probe_17_pend_build", dict(
        jt="INNER", n_l=100, n_r=400, extra_r=16,
        pend={"l": [X], "r": WIDE}, out=[K, X, 5 + K, 5 + F], group={},
        env={**GJ0, **FB0})),
    ("gj_no_pending_probe", dict(jt="INNER", n_l=100, n_r=400,
                                 pend={"l": [X]}, group={},
                                 env={**GJ0, **FB0})),
    ("gj_below_min_rows", dict(jt="INNER", n_l=100, n_r=400, pend={"r": [Y]},
                               group={}, env=FB0)),
    ("gj_disabled", dict(jt="INNER", n_l=100, n_r=400, pend={"r": [Y]},
                         group={},
                         env={**GJ0, **FB0, "DSX_DISABLE_GROUPJOIN": "1"})),
    ("gj_left_join", dict(jt="LEFT", pend={"l": [Y]}, group={},
                          env={**GJ0, **FB0})),
    ("gj_float_key", dict(jt="INNER", n_l=100, n_r=400, float_l=True,
                          float_r=True, pend={"r": [Y]}, group={},
                          env={**GJ0, **FB0})),
    ("gj_dict_key_rewritten", dict(
        jt="INNER", on=[(D, D)], n_l=400, n_r=100, dict_r=["c", "a", "q"],
        pend={"l": [Y]}, group={"build": "r"}, env={**GJ0, **FB0})),
    ("gj_wide_probe_17", dict(jt="INNER", n_l=100, n_r=400, extra_r=16,
                              pend={"r": WIDE}, out=[K, X, 5 + K, 5 + F],
                              group={}, env={**GJ0, **FB0})),
    ("gj_dup_keys", dict(jt="INNER", n_l=100, n_r=400, pend={"r": [Y]},
                         group={}, env=GJ0,
                         refuse=["filter_probe_groupby",
                                 "filter_probe_cols"])),
    ("gj_dup_keys_build_cols", dict(
        jt="INNER", n_l=100, n_r=400, pend={"r": [Y]}, group={},
        env={**GJ0, **FB0},
        refuse=["filter_probe_groupby", "filter_probe_cols"])),
    ("gj_raises", dict(jt="INNER", n_l=100, n_r=400, pend={"r": [Y]},
                       group={}, env={**GJ0, **FB0},
                       raise_in="filter_probe_groupby")),
    ("gj_dup_keys_join_raises", dict(
        jt="INNER", n_l=100, n_r=400, pend={"r": [Y]}, group={},
        env={**GJ0, **FB0}, refuse=["filter_probe_groupby"],
        raise_in="filter_probe_cols")),
]


def _build(runtime, opt):
    n_l, n_r = opt.get("n_l", 300), opt.get("n_r", 200)
    dict_r = opt.get("dict_r", DICT)
    dc_l = side_table(runtime, "L", n_l, float_key=opt.get("float_l", False),
                      extra=opt.get("extra_l", 0))
    dc_r = side_table(runtime, "R", n_r, dictionary=dict_r,
                      float_key=opt.get("float_r", False),
                      extra=opt.get("extra_r", 0),
                      null_key=opt.get("null_key", False),
                      wide_codes=opt.get("wide_codes_r", False))
    n_lc = len(dc_l.column_container.columns)
    n_rc = len(dc_r.column_container.columns)
    pend = opt.get("pend", {})
    if "l" in pend:
        dc_l = pending(runtime, dc_l, "l", pend["l"])
    if "r" in pend:
        dc_r = pending(runtime, dc_r, "r", pend["r"])
    cond = None
    for li, ri in opt.get("on", [(K, K)]):
        e = _eq(li, n_lc + ri)
        cond = e if cond is None else Call("AND", [cond, e])
    if "residual" in opt:
        cond = Call("AND", [cond, _residual(opt["residual"], n_lc)])
    node = JoinNode(opt["jt"], cond, opt.get("out"))
    if opt.get("null_equal"):
        node.null_equal = True
    if opt.get("null_aware"):
        node.null_aware = True
    if opt.get("out") is not None:
        n_out = len(opt["out"])
    elif opt["jt"] in ("LEFTSEMI", "LEFTANTI"):
        n_out = n_lc
    else:
        n_out = n_lc + n_rc
    leaves = [_plan("TraceInput", [], [], dc_l),
              _plan("TraceInput", [], [], dc_r)]
    rel = _plan("Join", leaves, [f"c{i}" for i in range(n_out)], node)
    return rel, n_lc


def _aggregate_over(rel, n_lc, opt):
    """Aggregate(Projection(Join)) in the pieces _try_group_join takes: GROUP
    BY the build side's key and x, SUM over a probe-side column, COUNT(*)."""
    g = opt["group"]
    build_l = g.get("build", "l") == "l"
    b0, p0 = (0, n_lc) if build_l else (n_lc, 0)
    cols = [b0 + K, b0 + X, p0 + X, p0 + K]
    out = opt.get("out")
    if out is not None:  # positions in the pruned join row
        cols = [out.index(c) for c in (b0 + K, b0 + X, p0 + F, p0 + K)]
    named = [(InputRef(c, BIGINT), f"p{i}") for i, c in enumerate(cols)]
    keys = [InputRef(0, BIGINT),
            InputRef(2 if g.get("probe_col") else 1, BIGINT)]
    calls = [AggCall("sum", [InputRef(2, BIGINT)], "SUM(p2)"),
             AggCall("count", [], "COUNT(*)")]
    node = AggregateNode(keys, calls)
    agg_rel = _plan("Aggregate", [rel], ["k", "x", "SUM(p2)", "COUNT(*)"],
                    node)
    return agg_rel, node, named, keys, calls


def _describe(runtime, dc):
    cc = dc.column_container
    cols = []
    for f in cc.columns:
        b = cc.get_backend_by_frontend_name(f)
        c = dc.table.col(b)
        cols.append({"name": f, "backend": b, "col": runtime.name(c),
                     "stats_src": runtime.name(getattr(c, "_stats_src",
                                                       None)),
                     "dictionary": getattr(c, "dictionary", None)})
    return {"columns": cols, "rows": dc.table.num_rows}


def run_case(case):
    """Runs one case; returns (trace dict, the FakeRuntime)."""
    name, opt = case
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(opt.get("env", {}))
    had = RelConverter._plugins.get("TraceInput")
    RelConverter._plugins["TraceInput"] = _TraceInputPlugin()
    RelConverter.add_plugin_class(DaskJoinPlugin, replace=False)
    runtime = FakeRuntime(opt.get("refuse", ()), opt.get("raise_in"),
                          opt.get("unmatched", 0))
    ctx = type("Ctx", (), {"_get_runtime": lambda self: runtime})()
    try:
        rel, n_lc = _build(runtime, opt)
        jp = RelConverter._plugins["Join"]
        try:
            if "group" in opt:
                agg_rel, node, named, gkeys, calls = _aggregate_over(
                    rel, n_lc, opt)
                ap = DaskAggregatePlugin.__new__(DaskAggregatePlugin)
                out, inputs, table = ap._try_group_join(
                    runtime, agg_rel, node, ctx, rel, named, gkeys, calls)
                via = "group_join"
                if out is None:
                    via = "join" if inputs is None else "join_with_inputs"
                    runtime._rec("join", inputs=inputs is not None,
                                 table=table)
                    out = jp.convert(rel, ctx, inputs=inputs, table=table) \
                        if inputs is not None else jp.convert(rel, ctx)
                result = dict(_describe(runtime, out), via=via)
            else:
                result = _describe(runtime, jp.convert(rel, ctx))
        except (rt.DsxError, RexCompileError, NotImplementedError) as e:
            result = {"error": f"{type(e).__name__}: {e}"}
    finally:
        if had is None:
            RelConverter._plugins.pop("TraceInput", None)
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    engine, setup = runtime.trace()
    return {"engine": engine, "setup": setup, "result": result}, runtime


def run_all():
    return {case[0]: run_case(case)[0] for case in CASES}


if __name__ == "__main__":
    traces = run_all()
    sys.stdout.write("{\n" + ",\n".join(
        f"{json.dumps(k)}: {json.dumps(traces[k], sort_keys=True)}"
        for k in sorted(traces)) + "\n}\n")
