"""Physical plugins: plan node → HIP kernel calls via the C ABI.

Each plugin mirrors the semantics of its reference counterpart (cited per
class) with the pandas/Dask delegation replaced by libdsxhip kernels
(DESIGN.md §3). Registered into RelConverter at package import
(reference context.py:118-152 default registration, replace=False)."""
from __future__ import annotations

import logging

import numpy as np

from dask_sql_amd import runtime as rt
from dask_sql_amd.datacontainer import (ColumnContainer, DataContainer,
                                        DeferredFilter, DeviceTable,
                                        HostDataContainer)
from dask_sql_amd.datacontainer import pending_filter as _pending_filter
from dask_sql_amd.physical import join_plan, keys
from dask_sql_amd.physical.convert import BaseRelPlugin, RelConverter
from dask_sql_amd.physical.join import DaskJoinPlugin, source_col
from dask_sql_amd.physical.keys import codes_i32 as _codes_i32
from dask_sql_amd.physical.keys import dicts_of as _dicts_of
from dask_sql_amd.physical.rex import (KB, KF, KI, OP_AND, OP_COL,
                                       OP_IS_NOT_NULL, OP_NOT,
                                       RexCompileError, compile_expr,
                                       scalar_literal)
from dask_sql_amd.planner.plan import Call, InputRef

logger = logging.getLogger(__name__)

_INT_KINDS = keys.INT_KINDS


def _gather_table(runtime, dc: DataContainer, sel_ptr, n_sel,
                  force_validity=False) -> DataContainer:
    """df[mask] / take: gather every backend column through a selection
    vector; gathers each backend buffer once."""
    cc = dc.column_container
    out_cols = {}
    for frontend in cc.columns:
        backend = cc.get_backend_by_frontend_name(frontend)
        if backend not in out_cols:
            col = dc.table.col(backend)
            g = runtime.gather(col, sel_ptr, n_sel, force_validity)
            if getattr(col, "dictionary", None) is not None:
                g.dictionary = col.dictionary
            g._stats_src = col  # range(subset) ⊆ range(source)
            out_cols[backend] = g
    return DataContainer(DeviceTable(out_cols, num_rows=n_sel), cc)


def _empty_like(runtime, dc: DataContainer) -> DataContainer:
    sel = runtime.empty_column(0, rt.I32)
    return _gather_table(runtime, dc, sel.data, 0)


def _case_string_rewrite(expr):
    """CASE whose value branches are string literals (or NULL) → the same
    CASE over dictionary codes + the dictionary (rex/core/call.py CASE with
    string outputs). Returns (rewritten Call, dictionary) or None."""
    from dask_sql_amd.planner.plan import Literal as PLit
    from dask_sql_amd.planner.plan import SqlType
    if not (isinstance(expr, Call) and expr.getOperatorName() == "CASE"):
        return None
    ops = expr.getOperands()
    vpos = list(range(1, len(ops) - 1, 2)) + [len(ops) - 1]
    has_str = False
    for p in vpos:
        o = ops[p]
        if not isinstance(o, PLit):
            return None
        v = o.getValue()
        if isinstance(v, str):
            has_str = True
        elif v is not None:
            return None
    if not has_str:
        return None
    d = []
    new_ops = list(ops)
    for p in vpos:
        v = ops[p].getValue()
        if v is None:
            continue
        if v not in d:
            d.append(v)
        new_ops[p] = PLit(d.index(v), SqlType("BIGINT"))
    return Call("CASE", new_ops, SqlType("BIGINT")), d


def _resolve_scalar_subs(expr, context):
    """Replace ScalarSub nodes with the Literal their (eagerly executed)
    subplan yields — ≤1 row enforced; 0 rows → NULL (SQL scalar subquery)."""
    from dask_sql_amd.planner.plan import ScalarSub
    if isinstance(expr, ScalarSub):
        dc = RelConverter.convert(expr.plan, context=context)
        from dask_sql_amd.materialize import to_pandas
        pdf = to_pandas(dc, context, expr.plan.getRowType())
        if len(pdf) > 1:
            raise RuntimeError(
                f"scalar subquery returned {len(pdf)} rows")
        import pandas as pd
        v = None if len(pdf) == 0 else pdf.iloc[0, 0]
        if v is not None and pd.isna(v):
            v = None
        if isinstance(v, np.integer):
            v = int(v)
        elif isinstance(v, np.floating):
            v = float(v)
        elif isinstance(v, np.bool_):
            v = bool(v)
        from dask_sql_amd.planner.plan import Literal as PLit
        return PLit(v, expr.getType())
    if isinstance(expr, Call):
        return Call(expr.getOperatorName(),
                    [_resolve_scalar_subs(o, context)
                     for o in expr.getOperands()], expr.getType())
    return expr


def _eval_udf_nodes(expr, cols, runtime, context):
    """Replace UDF:<name> Calls with InputRefs to freshly computed columns.

    The reference executes registered Python functions on pandas partition
    data (context.py:324 register_function → rex call) — we do EXACTLY the
    same: operand columns round-trip device→host, the Python callable runs
    vectorized, the result uploads back. This is the explicit UDF slow
    path, not a silent fallback. `cols` is extended in
    place; returns the rewritten expression."""
    if isinstance(expr, InputRef) or not hasattr(expr, "getOperands") \
            or not hasattr(expr, "getOperatorName"):
        return expr
    ops = [_eval_udf_nodes(o, cols, runtime, context) for o in
           expr.getOperands()]
    name = expr.getOperatorName()
    if not (isinstance(name, str) and name.startswith("UDF:")):
        if ops != list(expr.getOperands()):
            return Call(name, ops, expr.getType())
        return expr
    f, ret_sql, row_udf, params = context.catalog.functions[name[4:]]
    import pandas as pd
    args = []
    n = cols[0].len if cols else 0
    for o in ops:
        prog, kind = compile_expr(o, cols, _dicts_of(cols))
        col = runtime.eval(runtime.make_prog(prog), cols, n,
                           rt.F64 if kind == KF else rt.I64,
                           with_validity=True)
        arr, valid = col.to_numpy()
        ser = pd.Series(arr)
        if valid is not None:
            ser = ser.where(valid.astype(bool))
        args.append(ser)
    if row_udf:
        # reference row_udf: f(row) with row[param_name]
        # (test_function.py:24-33)
        frame = pd.DataFrame({pn: a for (pn, _), a in zip(params, args)})
        out = frame.apply(f, axis=1)
    else:
        out = f(*args)
    out = pd.Series(out)
    res = out.to_numpy()
    validity = None
    if res.dtype == object:
        res = res.astype(np.float64)
    if res.dtype.kind == "f":
        nan = np.isnan(res)
        if nan.any():
            validity = (~nan).astype(np.uint8)
    if res.dtype.kind == "b":
        res = res.astype(np.uint8)
        new_col = runtime.upload_column(res, validity, rt.BOOL8)
    elif res.dtype.kind in "iu":
        new_col = runtime.upload_column(res.astype(np.int64), validity)
    else:
        new_col = runtime.upload_column(res.astype(np.float64), validity)
    cols.append(new_col)
    from dask_sql_amd.planner.plan import SqlType
    return InputRef(len(cols) - 1, SqlType(ret_sql))


def _unique_backends(cc):
    backends = []
    for f in cc.columns:
        b = cc.get_backend_by_frontend_name(f)
        if b not in backends:
            backends.append(b)
    return backends


def _run_deferred_filter(d: DeferredFilter) -> DeviceTable:
    """First `.table` access of a DeferredFilter: the ordinary fused filter
    (dsx_filter_cols) over the base container's columns."""
    base = d.base
    runtime = d.prog_cols[0].rt
    backends = _unique_backends(base.column_container)
    mats = [base.table.col(b) for b in backends]
    out_list, count = runtime.filter_cols(
        runtime.make_prog(d.prog), d.prog_cols, base.table.num_rows, mats)
    out_cols = {}
    for b, src, col in zip(backends, mats, out_list):
        if getattr(src, "dictionary", None) is not None:
            col.dictionary = src.dictionary
        col._stats_src = src
        out_cols[b] = col
    return DeviceTable(out_cols, num_rows=count)


def _has_udf(expr) -> bool:
    if not hasattr(expr, "getOperands") or not hasattr(expr,
                                                       "getOperatorName"):
        return False
    name = expr.getOperatorName()
    if isinstance(name, str) and name.startswith("UDF:"):
        return True
    return any(_has_udf(o) for o in expr.getOperands())


def _defer_filter(runtime, dc, condition, context):
    """WHERE over a base-table scan → DeferredFilter (None = filter now).
    A second WHERE over a pending one joins it as a conjunction: a filter
    keeps a row only when its predicate is TRUE, so (p1 AND p2) keeps
    exactly the rows that p2 keeps of what p1 kept."""
    if join_plan.filterprobe_disabled():
        return None
    if _has_udf(condition):
        return None  # UDF nodes evaluate through the host, eagerly
    pending = _pending_filter(dc)
    if not pending and not getattr(dc, "base_scan", False):
        return None
    src = dc.unfiltered() if pending else dc
    base = dc.base if pending else dc
    if len(_unique_backends(base.column_container)) > 16:
        return None
    cols = src.backend_cols()
    if not cols:
        return None
    prog, _ = compile_expr(condition, cols, _dicts_of(cols))
    prog = [tuple(ins) for ins in prog]
    # keep only the columns the predicate reads (the join adds its key
    # columns to this list, and the kernels take 16 at most)
    merged = list(dc.prog_cols) if pending else []
    remap = {}
    for a in sorted({a for op, a, _ in prog if op == OP_COL}):
        j = next((k for k, m in enumerate(merged) if m is cols[a]), None)
        if j is None:
            merged.append(cols[a])
            j = len(merged) - 1
        remap[a] = j
    prog = [(op, remap[a], imm) if op == OP_COL else (op, a, imm)
            for op, a, imm in prog]
    if pending:
        prog = list(dc.prog) + prog + [(OP_AND, 0, 0)]
    cols = merged
    if not cols or len(cols) > rt.MAX_COLS:
        return None
    try:
        runtime.make_prog(prog)  # length / stack-depth limits
    except rt.DsxError:
        return None
    return DeferredFilter(base, dc.column_container, prog, cols,
                          _run_deferred_filter)


def _apply_filter(runtime, dc: DataContainer, condition,
                  context=None) -> DataContainer:
    """filter_or_scalar semantics (reference filter.py:20-45). Fused path:
    the filter's emit pass writes the surviving rows of every column
    directly (dsx_filter_cols) — no selection vector, no per-column
    gathers."""
    s = scalar_literal(condition)
    if s is not None:
        return dc if s else _empty_like(runtime, dc)
    deferred = _defer_filter(runtime, dc, condition, context)
    if deferred is not None:
        return deferred
    cols = dc.backend_cols()
    if context is not None and context.catalog.functions:
        condition = _eval_udf_nodes(condition, cols, runtime, context)
    prog, kind = compile_expr(condition, cols, _dicts_of(cols))
    cc = dc.column_container
    backends = _unique_backends(cc)
    mats = [dc.table.col(b) for b in backends]
    if len(mats) <= 16:
        out_list, count = runtime.filter_cols(runtime.make_prog(prog), cols,
                                              dc.table.num_rows, mats)
        out_cols = {}
        for b, src, col in zip(backends, mats, out_list):
            if getattr(src, "dictionary", None) is not None:
                col.dictionary = src.dictionary
            col._stats_src = src
            out_cols[b] = col
        return DataContainer(DeviceTable(out_cols, num_rows=count), cc)
    sel_ptr, count = runtime.filter(runtime.make_prog(prog), cols,
                                    dc.table.num_rows)
    sel = runtime.wrap_sel(sel_ptr, count)  # owns the library buffer
    out = _gather_table(runtime, dc, sel.data, count)
    return out


class DaskTableScanPlugin(BaseRelPlugin):
    """reference rel/logical/table_scan.py:21-119: pull the registered table;
    here: Arrow/numpy → HBM upload, cached on the registered table."""

    class_name = "TableScan"

    def convert(self, rel, context):
        scan = rel.table_scan()
        table = context._device_table(scan.getTableName())
        cc = ColumnContainer(table.names())
        if scan.containsProjections():
            cc = cc.limit_to(scan.getTableScanProjects())
        dc = DataContainer(table, cc)
        dc.base_scan = True  # a WHERE over it may be deferred into a join
        for f in scan.getFilters():
            dc = _apply_filter(context._get_runtime(), dc, f)
        cc = self.fix_column_to_row_type(dc.column_container, rel.getRowType())
        return dc.with_columns(cc)


class DaskFilterPlugin(BaseRelPlugin):
    """reference rel/logical/filter.py:48-74 — WHERE via fused predicate-eval
    + wave-ballot compaction (k_filter_mask/k_filter_emit)."""

    class_name = "Filter"

    def convert(self, rel, context):
        (dc,) = self.assert_inputs(rel, 1, context)
        condition = _resolve_scalar_subs(rel.filter().getCondition(), context)
        dc = _apply_filter(context._get_runtime(), dc, condition, context)
        cc = self.fix_column_to_row_type(dc.column_container, rel.getRowType())
        return dc.with_columns(cc)


class DaskProjectPlugin(BaseRelPlugin):
    """reference rel/logical/project.py:17-78: InputRef shortcut, else
    RexConverter + assign → here dsx_eval."""

    class_name = "Projection"

    def convert(self, rel, context):
        (dc,) = self.assert_inputs(rel, 1, context)
        runtime = context._get_runtime()
        cols = dc.backend_cols()
        dicts = _dicts_of(cols)
        named = rel.projection().getNamedProjects()
        out_cols = {}
        new_names = []
        from dask_sql_amd.physical.rex import (dict_int_fn, dict_string_fn,
                                               fold_string_literal)
        for i, (expr, name) in enumerate(named):
            backend_name = f"p{i}__{name}"
            if not isinstance(expr, InputRef):
                expr = _resolve_scalar_subs(expr, context)
            if context.catalog.functions and not isinstance(expr, InputRef):
                expr = _eval_udf_nodes(expr, cols, runtime, context)
            if isinstance(expr, InputRef) and expr.getIndex() >= len(
                    dc.column_container.columns):
                # UDF result column: materialize it directly
                out_cols[backend_name] = cols[expr.getIndex()]
                new_names.append((name, backend_name))
                continue
            sfn = None if isinstance(expr, InputRef) \
                else dict_string_fn(expr, dicts)
            ifn = None if isinstance(expr, InputRef) or sfn is not None \
                else dict_int_fn(expr, dicts)
            const_s = None
            csr = None
            if not isinstance(expr, InputRef) and sfn is None and ifn is None:
                const_s = fold_string_literal(expr)
                if const_s is None:
                    csr = _case_string_rewrite(expr)
            if isinstance(expr, InputRef):
                src = cols[expr.getIndex()]
                out_cols[backend_name] = src  # zero-copy reuse
            elif ifn is not None:
                # int-valued string function (CHAR_LENGTH): per-dictionary
                # LUT gathered by the code column (test_rex.py:603)
                ci, f = ifn
                src = cols[ci]
                lut = np.array([f(s_) if s_ is not None else 0
                                for s_ in src.dictionary], dtype=np.int64)
                lut_col = runtime.upload_column(lut)
                g = runtime.gather(lut_col, src.data, src.len)
                out_cols[backend_name] = rt.DeviceColumn(
                    runtime, g.data, src.validity, src.len, rt.I64,
                    owner=False, keep_alive=(g, src, lut_col))
            elif const_s is not None:
                # literal-only string chain → constant dict column
                n_ = dc.table.num_rows
                col = runtime.upload_column(
                    np.zeros(n_, dtype=np.int32), dtype=rt.I32)
                col.dictionary = [const_s]
                out_cols[backend_name] = col
            elif csr is not None:
                # string-valued CASE → integer-code CASE + dictionary
                e2, d = csr
                prog, _k = compile_expr(e2, cols, dicts)
                col = runtime.eval(runtime.make_prog(prog), cols,
                                   dc.table.num_rows, rt.I64,
                                   with_validity=True)
                col.dictionary = d
                out_cols[backend_name] = col
            elif sfn is not None:
                # string function over a dict column: same codes, the
                # transform runs once over the dictionary
                # (rex/core/call.py:1069-1135 string ops)
                ci, f = sfn
                src = cols[ci]
                col = rt.DeviceColumn(runtime, src.data, src.validity,
                                      src.len, src.dtype, owner=False,
                                      keep_alive=src)
                col.dictionary = [f(s) if s is not None else None
                                  for s in src.dictionary]
                out_cols[backend_name] = col
            else:
                prog, kind = compile_expr(expr, cols, dicts)
                out_dtype = rt.F64 if kind == KF else (
                    rt.BOOL8 if kind == KB else rt.I64)
                col = runtime.eval(runtime.make_prog(prog), cols,
                                   dc.table.num_rows, out_dtype,
                                   with_validity=True)
                out_cols[backend_name] = col
            new_names.append((name, backend_name))
        cc = ColumnContainer([n for n, _ in new_names],
                             dict(new_names))
        cc = self.fix_column_to_row_type(cc, rel.getRowType())
        return DataContainer(DeviceTable(out_cols,
                                         num_rows=dc.table.num_rows), cc)


# aggregates the device kernels do not carry; the reference itself runs
# them as pandas reductions (custom dask Aggregations)
_HOST_ONLY_AGGS = {"bit_and", "bit_or", "bit_xor"}


class DaskAggregatePlugin(BaseRelPlugin):
    """reference rel/logical/aggregate.py:91-589.

    Aggregations bucketed by (filter, distinct) like _collect_aggregations
    (:377-520); each bucket is ONE fused k_groupby kernel (pred program =
    the bucket's filter column expression); groupby(dropna=False) (:575-577)
    falls out of NULL key codes; SUM min_count=1 (:486-493) finalized from
    the per-agg non-NULL counts. AVG = SUM+COUNT finalize (dask 'mean')."""

    class_name = ["Aggregate", "Distinct"]

    AGG_OPS = {"sum", "count", "avg", "min", "max", "any_value",
               "single_value", "stddev", "stddev_samp", "stddev_pop",
               "var_samp", "var_pop", "variance", "every", "bool_and",
               "bool_or"}

    # stddev/variance family: ONE call decomposes into TWO kernel slots
    # (SUM(x), SUM(x*x)); finalize composes m2 = Σx² − (Σx)²/n like the
    # reference's dask std aggregation (aggregate.py AGGREGATION_MAPPING
    # "stddev" → dd.Aggregation over sum/count moments), ddof=1 for the
    # sample forms (pandas default), ddof=0 for *_POP.
    STD_FINS = {"std_samp", "std_pop", "var_samp", "var_pop"}

    _HOST_ONLY_AGGS = frozenset()  # set below the class (shared)

    def _host_udf_aggregate(self, rel, agg, context):
        """Registered aggregate UDFs run as Python on host frames — the
        reference's own execution model for register_aggregation
        (dd.Aggregation chunk/agg[/finalize], context.py:415; executed by
        pandas either way). Single partition: chunk over the groupby, agg
        over the chunk results, optional finalize. Built-in aggs mixed
        into the same node run with their pandas equivalents
        (aggregate.py:117-231 semantics)."""
        import pandas as pd

        from dask_sql_amd.context import _from_pandas
        from dask_sql_amd.materialize import to_pandas

        (dc,) = self.assert_inputs(rel, 1, context)
        pdf = to_pandas(dc, context)
        group_idx = [e.getIndex() for e in agg.getGroupSets()]
        keys = [pdf.columns[i] for i in group_idx]
        work = pdf.assign(__const_1__=1)
        gb_keys = keys if keys else ["__const_1__"]
        field_names = [str(f) for f in rel.getRowType().getFieldNames()]
        results = {}
        def _bitred(np_op):
            def f(sg):
                return sg.agg(lambda s: np_op.reduce(
                    s.dropna().astype(np.int64))
                    if s.notna().any() else None)
            return f

        def _strsafe(how):
            # string columns with NULLs: pandas' object min/max compares
            # None against str — reduce over the non-NULL values instead
            def f(sg):
                if sg.obj.dtype == object:
                    return sg.agg(lambda s: getattr(s.dropna(), how)()
                                  if s.notna().any() else None)
                return getattr(sg, how)()
            return f

        builtin = {"sum": lambda sg: sg.sum(min_count=1),
                   "count": lambda sg: sg.count(),
                   "avg": lambda sg: sg.mean(),
                   "min": _strsafe("min"), "max": _strsafe("max"),
                   "bit_and": _bitred(np.bitwise_and),
                   "bit_or": _bitred(np.bitwise_or),
                   "bit_xor": _bitred(np.bitwise_xor),
                   "every": lambda sg: sg.agg(
                       lambda s: bool(s.dropna().astype(bool).all())
                       if s.notna().any() else None),
                   "bool_and": lambda sg: sg.agg(
                       lambda s: bool(s.dropna().astype(bool).all())
                       if s.notna().any() else None),
                   "bool_or": lambda sg: sg.agg(
                       lambda s: bool(s.dropna().astype(bool).any())
                       if s.notna().any() else None),
                   "single_value": lambda sg: sg.first(),
                   "any_value": lambda sg: sg.first(),
                   "stddev": lambda sg: sg.std(),
                   "stddev_samp": lambda sg: sg.std(),
                   "stddev_pop": lambda sg: sg.std(ddof=0),
                   "var_samp": lambda sg: sg.var(),
                   "variance": lambda sg: sg.var(),
                   "var_pop": lambda sg: sg.var(ddof=0)}
        for pos, call in enumerate(agg.getNamedAggCalls()):
            func = agg.getAggregationFuncName(call).lower()
            args = agg.getArgs(call)
            if args:
                if not isinstance(args[0], InputRef):
                    raise RexCompileError(
                        "UDF aggregate over an expression: project it to a "
                        "column first")
                in_col = pdf.columns[args[0].getIndex()]
            else:
                in_col = "__const_1__"
            sg = work.groupby(gb_keys, dropna=False)[in_col]
            if func.startswith("udf:"):
                obj = context.catalog.aggregations[func[4:]][0]
                if hasattr(obj, "chunk") and hasattr(obj, "agg"):
                    chunked = obj.chunk(sg)
                    # single partition: the tree-reduce step runs once
                    r = obj.agg(chunked.groupby(
                        level=list(range(len(gb_keys)))))
                    fin = getattr(obj, "finalize", None)
                    if fin is not None:
                        r = fin(r.to_frame().groupby(
                            level=list(range(len(gb_keys)))))
                        r = pd.Series(r)
                else:
                    r = sg.agg(obj)
            elif func in builtin:
                r = builtin[func](sg)
            else:
                raise RexCompileError(
                    f"aggregate {func} beside a UDF aggregate (round-3)")
            results[field_names[len(keys) + pos]] = r
        out = pd.DataFrame(results).reset_index()
        if not keys:
            out = out.drop(columns=["__const_1__"], errors="ignore")
        out.columns = field_names[len(keys):] if not keys else (
            field_names[:len(keys)] + list(out.columns[len(keys):]))
        out = out[[c for c in field_names if c in out.columns]]
        runtime = context._get_runtime()
        host_cols = _from_pandas(out)
        dev = {}
        for n_, h in host_cols.items():
            col = runtime.upload_column(h.arr, h.validity, h.dtype)
            if h.dictionary is not None:
                col.dictionary = h.dictionary
            dev[n_] = col
        cc = ColumnContainer(list(out.columns))
        cc = self.fix_column_to_row_type(cc, rel.getRowType())
        return DataContainer(DeviceTable(dev, num_rows=len(out)), cc)

    def convert(self, rel, context):
        runtime = context._get_runtime()
        agg = rel.aggregate()

        # FUSION PEEPHOLE (the north-star kernel, SURVEY §3 call stacks
        # (2)+(4) fused): Aggregate(Projection(Filter*(X))) → ONE kernel over
        # X's columns with the WHERE predicate as the kernel's pred program
        # and the projection arithmetic folded into each agg program. This is
        # what replaces the reference's filter→assign→groupby pass chain with
        # a single HBM scan.
        if not agg.isDistinctNode():
            calls = agg.getNamedAggCalls()

            def _is_host_only(c):
                fn = agg.getAggregationFuncName(c).lower()
                if fn.startswith("udf:") or fn in _HOST_ONLY_AGGS:
                    return True
                if fn in ("min", "max", "single_value", "any_value"):
                    # string (dict-encoded) MIN/MAX must compare by STRING
                    # order, not appearance-order codes — pandas does this
                    # on host exactly like the reference
                    args = agg.getArgs(c)
                    if args and isinstance(args[0], InputRef):
                        in_fields = rel.get_inputs()[0].getRowType()                             .getFieldList()
                        i = args[0].getIndex()
                        if i < len(in_fields) and in_fields[i].getType()                                 .getSqlType() == "VARCHAR":
                            return True
                return False

            if any(_is_host_only(c) for c in calls):
                # registered UDF aggregates, and the bitwise reductions the
                # device kernels don't carry — the reference computes BOTH
                # as custom dask Aggregations on pandas (rel/custom/
                # wrappers ReduceAggregation bit_and/bit_or), so host
                # evaluation IS the reference execution model
                return self._host_udf_aggregate(rel, agg, context)

        import os
        fused = None
        if not os.environ.get("DSX_DISABLE_FUSED"):
            fused = self._try_fused(runtime, rel, agg, context)
        if fused is not None:
            return fused

        (dc,) = self.assert_inputs(rel, 1, context)
        cols = dc.backend_cols()

        if agg.isDistinctNode():
            group_idx = list(range(len(dc.column_container.columns)))
            agg_calls = []
        else:
            group_exprs = agg.getGroupSets()
            group_idx = []
            for e in group_exprs:
                assert isinstance(e, InputRef), "group expr must be InputRef"
                group_idx.append(e.getIndex())
            agg_calls = agg.getNamedAggCalls()

        # key specs from minmax (float key: bit-pattern mode, single key;
        # floats inside composite key sets are densified to integer ids)
        name_idx = list(group_idx)
        # DISTINCT aggregates extend the integer key with the argument, so
        # a single float key is densified for them too
        cols, group_idx, key_restore = self._densify_float_keys(
            runtime, cols, group_idx,
            force=any(c.isDistinctAgg() for c in agg_calls))
        keyspecs = self._keyspecs_for(runtime, cols, group_idx)

        # bucket aggs by (filter_col_index, distinct) — aggregate.py:377-520
        from collections import OrderedDict
        buckets = OrderedDict()
        for call in agg_calls:
            func = agg.getAggregationFuncName(call).lower()
            if func not in self.AGG_OPS:
                raise RexCompileError(f"aggregate {func} (round-2)")
            filt = call.getFilterExpr()
            filt_key = filt.getIndex() if filt is not None else None
            distinct = call.isDistinctAgg()
            buckets.setdefault((filt_key, distinct), []).append(call)

        single_plain = (len(buckets) <= 1 and not any(
            d for (_, d) in buckets.keys()))
        if single_plain:
            # FAST PATH (all bench configs): one fused kernel, result stays
            # device-resident; finalize via dsx_eval.
            calls = list(agg_calls)
            filt_idx = next(iter(buckets.keys()))[0] if buckets else None
            return self._convert_device(runtime, rel, dc, cols, keyspecs,
                                        group_idx, filt_idx, calls, agg,
                                        name_idx, key_restore)

        # GENERAL PATH: several (filter, distinct) buckets → merge on host
        # like the reference's multi-pass _do_aggregations (aggregate.py:336+)
        keys_sorted = sorted(buckets.keys(),
                             key=lambda k: (k[0] is not None, k[1], str(k)))
        results = []
        for bkey in keys_sorted:
            calls = buckets[bkey]
            filt_idx, distinct = bkey
            if distinct:
                res = self._distinct_bucket(runtime, agg, dc, cols, keyspecs,
                                            filt_idx, calls)
            else:
                res = self._run_bucket(runtime, agg, dc, cols, keyspecs,
                                       filt_idx, calls)
            results.append((bkey, calls, *res))

        codes_np = results[0][2]
        merged = {}  # call name -> (vals np, cnts np) aligned to codes_np
        for bkey, calls, bcodes, percall in results:
            if bcodes is codes_np or np.array_equal(bcodes, codes_np):
                for call, vc in zip(calls, percall):
                    merged[call.toString()] = vc
            else:
                # align bucket groups into base group order; missing → cnt 0
                pos = {c: i for i, c in enumerate(bcodes.tolist())}
                idx = np.array([pos.get(c, -1) for c in codes_np.tolist()],
                               dtype=np.int64)
                for call, (vals, cnts) in zip(calls, percall):
                    hit = idx >= 0
                    ac = np.zeros(len(codes_np), dtype=np.uint64)
                    ac[hit] = cnts[idx[hit]]

                    def align(v):
                        av = np.zeros(len(codes_np), dtype=v.dtype)
                        av[hit] = v[idx[hit]]
                        return av

                    if isinstance(vals, tuple):  # stddev family moments
                        merged[call.toString()] = (
                            tuple(align(v) for v in vals), ac)
                    else:
                        merged[call.toString()] = (align(vals), ac)

        return self._build_output(runtime, rel, dc, keyspecs, group_idx,
                                  codes_np, agg_calls, merged,
                                  name_idx=name_idx, key_restore=key_restore)

    # ------------------------------------------------------------------
    def _try_fused(self, runtime, rel, agg, context):
        """Fusion peephole; returns a DataContainer or None (fall back)."""
        from dask_sql_amd.planner.plan import Literal as PLiteral
        from dask_sql_amd.planner.plan import SqlType

        if agg.isDistinctNode():
            return None
        calls = agg.getNamedAggCalls()
        if not calls:
            return None
        if any(c.getFilterExpr() is not None or c.isDistinctAgg()
               for c in calls):
            return None
        input_rel = rel.get_inputs()[0]
        if input_rel.get_current_node_type() != "Projection":
            return None
        named = input_rel.projection().getNamedProjects()
        node = input_rel.get_inputs()[0]
        pred_exprs = []
        while node.get_current_node_type() == "Filter":
            cond = node.filter().getCondition()
            if scalar_literal(cond) is not None:
                return None
            pred_exprs.append(cond)
            node = node.get_inputs()[0]
        base_rel = node
        group_exprs = agg.getGroupSets()
        if not all(isinstance(e, InputRef) for e in group_exprs):
            return None
        for e in group_exprs:
            if not isinstance(named[e.getIndex()][0], InputRef):
                return None
        join_inputs = None
        if base_rel.get_current_node_type() == "Join" and not pred_exprs:
            out, join_inputs, join_table = self._try_group_join(
                runtime, rel, agg, context, base_rel, named, group_exprs,
                calls)
            if out is not None:
                return out
        try:
            if join_inputs is not None:
                # the attempt converted the join's inputs; they run once
                base_dc = RelConverter._plugins["Join"].convert(
                    base_rel, context, inputs=join_inputs, table=join_table)
            else:
                base_dc = RelConverter.convert(base_rel, context)
            base_cols = base_dc.backend_cols()
            dicts = _dicts_of(base_cols)
            group_meta = []
            gidx = []
            for e in group_exprs:
                proj_expr, proj_name = named[e.getIndex()]
                bi = proj_expr.getIndex()
                gidx.append(bi)
                group_meta.append((proj_name, base_cols[bi]))
            keyspecs = self._keyspecs_for(runtime, base_cols, gidx)
            pred_prog = None
            if pred_exprs:
                cond = pred_exprs[0]
                for p in pred_exprs[1:]:
                    cond = Call("AND", [cond, p])
                cond = _resolve_scalar_subs(cond, context)
                prog, _ = compile_expr(cond, base_cols, dicts)
                pred_prog = runtime.make_prog(prog)
            specs, fins, slab = [], [], []
            for call in calls:
                func = agg.getAggregationFuncName(call).lower()
                if func not in self.AGG_OPS:
                    return None
                args = agg.getArgs(call)
                if args:
                    if not isinstance(args[0], InputRef):
                        return None
                    expr = named[args[0].getIndex()][0]
                else:
                    expr = PLiteral(1, SqlType("BIGINT"))
                speclist, fin = self._agg_spec_expr(func, expr, base_cols,
                                                    dicts)
                slab.append(len(specs))
                for op, prog in speclist:
                    specs.append((op, runtime.make_prog(prog)))
                fins.append(fin)
        except RexCompileError:
            return None
        logger.debug("aggregate: fused scan over %s",
                     base_rel.get_current_node_type())
        return self._device_exec(runtime, rel, base_cols,
                                 base_dc.table.num_rows, keyspecs, group_meta,
                                 pred_prog, calls, specs, fins, slab)

    def _finished_output(self, rel, group_meta, kcols, calls, acols,
                         float_key=None):
        """The aggregate's container from finished device columns: key
        columns (hash_groupby_cols / filter_probe_groupby) named and typed
        after group_meta's (name, source column), then one column per
        call."""
        out_cols = {}
        order_names = []
        float_key = float_key or [False] * len(kcols)
        for fk, (name, src), col in zip(float_key, group_meta, kcols):
            if not fk and getattr(src, "dictionary", None) is not None:
                col.dictionary = src.dictionary
            col.logical_dtype = src.dtype
            out_cols[f"g__{name}"] = col
            order_names.append((name, f"g__{name}"))
        for call, col in zip(calls, acols):
            name = call.toString()
            out_cols[f"a__{name}"] = col
            order_names.append((name, f"a__{name}"))
        cc = ColumnContainer([n for n, _ in order_names],
                             dict(order_names))
        cc = self.fix_column_to_row_type(cc, rel.getRowType())
        return DataContainer(DeviceTable(out_cols), cc)

    def _try_group_join(self, runtime, rel, agg, context, base_rel, named,
                        group_exprs, calls):
        """Aggregate(Projection(Join)) as one group-join sweep
        (physical/group_join.py, Runtime.filter_probe_groupby). Returns
        (DataContainer or None, inputs, table): inputs are the join's
        converted inputs once this attempt has converted them, and table the
        hash table of an attempt that the entry declined, both for the
        caller to hand to the join (which frees the table)."""
        from dask_sql_amd.physical import group_join as gj
        from dask_sql_amd.planner.plan import Literal as PLiteral
        from dask_sql_amd.planner.plan import SqlType
        from dask_sql_amd.planner.prune import _expr_refs, _remap

        jp = RelConverter._plugins.get("Join")
        if gj.disabled() or not isinstance(jp, DaskJoinPlugin):
            return None, None, None
        if str(base_rel.join().getJoinType()) != "INNER":
            return None, None, None
        # the prepared join stands for its inputs from here on
        inputs = J = jp.prepare(base_rel,
                                *jp.assert_inputs(base_rel, 2, context))
        R = jp.route(J, group_join=True)  # the build side's WHERE runs first
        fprobe = R.fprobe
        out_idx = J.out_idx

        key_dtypes = [(jp.key_dtype(lc, "l"), jp.key_dtype(rc, "r"))
                      for lc, rc in zip(*jp.key_columns(J))]
        group_cols = []
        for e in group_exprs:
            pe = named[e.getIndex()][0]
            group_cols.append(out_idx[pe.getIndex()]
                              if isinstance(pe, InputRef) else None)
        facts, arg_exprs = [], []
        for call in calls:
            args = agg.getArgs(call)
            expr, refs = None, None
            if args:
                if not isinstance(args[0], InputRef):
                    return None, inputs, None
                expr = named[args[0].getIndex()][0]
                refs = set()
                _expr_refs(expr, refs)
            arg_exprs.append((expr, refs))
            facts.append(gj.AggFact(
                agg.getAggregationFuncName(call).lower(),
                None if refs is None else frozenset(out_idx[i] for i in refs),
                bool(call.isDistinctAgg()),
                call.getFilterExpr() is not None))
        v = gj.verdict(
            join_type=J.join_type, residual=bool(J.residual),
            null_equal=J.null_eq, probe_side=fprobe,
            n_lhs_cols=J.n_lhs_cols, lhs_on=J.lhs_on, rhs_on=J.rhs_on,
            key_dtypes=key_dtypes, group_cols=group_cols, aggs=facts,
            max_aggs=rt.MAX_AGGS, max_keys=rt.MAX_KEYS)
        if not v:
            logger.debug("aggregate: no group-join (%s)", v.reason)
            return None, inputs, None
        pending = J.dc_lhs if fprobe == "l" else J.dc_rhs
        if pending.max_rows < gj.min_rows():
            return None, inputs, None
        R = jp.settle(J, R, group_join=True)
        S = jp.fused_setup(runtime, J, R)

        def src_col(ci):
            return source_col(J, ci, S.dc_lhs, S.dc_rhs)

        # the aggregate arguments' probe columns join the predicate's and
        # the keys' in the entry's one column list
        fp_cols = list(S.fp_cols)

        def fp_index(k):
            col = src_col(out_idx[k])
            ci = next((i for i, c in enumerate(fp_cols) if c is col), None)
            if ci is None:
                fp_cols.append(col)
                ci = len(fp_cols) - 1
            return ci

        remapped = []
        for expr, refs in arg_exprs:
            if expr is None:
                remapped.append(PLiteral(1, SqlType("BIGINT")))
            else:
                remapped.append(_remap(expr, {k: fp_index(k) for k in refs}))
        if len(fp_cols) > rt.MAX_COLS:
            return None, inputs, None
        try:
            dicts = _dicts_of(fp_cols)
            specs, fins, slab = [], [], []
            for fact, expr in zip(facts, remapped):
                speclist, fin = self._agg_spec_expr(fact.func, expr, fp_cols,
                                                    dicts)
                slab.append(len(specs))
                for op, prog in speclist:
                    specs.append((op, runtime.make_prog(prog)))
                fins.append(fin)
        except RexCompileError:
            return None, inputs, None
        if not all(f in runtime.GB_FIN_KINDS for f in fins) \
                or len(specs) > rt.MAX_AGGS:
            return None, inputs, None
        build_cols = (S.dc_lhs if S.swap else S.dc_rhs).backend_cols()
        kcols, group_meta = [], []
        for e, g, (kind, i) in zip(group_exprs, group_cols, v.key_sources):
            # a probe-side join key comes out as its build-side twin
            kcols.append(build_cols[S.build_on[i]] if kind == "key"
                         else src_col(g))
            group_meta.append((named[e.getIndex()][1], src_col(g)))
        # the build side is materialized by now, so the build-from-columns
        # entry takes it with an empty predicate
        table = jp.build_table(runtime, S, R, key_filter=True)
        try:
            res = runtime.filter_probe_groupby(
                table, runtime.make_prog(S.pending.prog), fp_cols, S.fp_keys,
                S.pending.max_rows, specs, list(zip(fins, slab)), kcols)
        except BaseException:
            runtime.hash_table_free(table)
            raise
        if res is None:
            # duplicate build keys: join, then group, over the same table
            return None, inputs, table
        runtime.hash_table_free(table)
        out_k, out_a, _ = res
        logger.debug("aggregate: group-join over %s", fprobe)
        return self._finished_output(
            rel, group_meta, out_k, calls, out_a,
            [c.dtype in (rt.F64, rt.F32) for c in kcols]), inputs, None

    @staticmethod
    def _keyspecs_for(runtime, cols, group_idx):
        """(idx, min, range, nullable[, mode]) per key. A single float key
        groups by canonical f64 bit pattern (mode 1) through the CAS hash
        path; float keys in COMPOSITE key sets are densified first
        (_densify_float_keys) — pandas float group keys compare exactly,
        NaN is one group under dropna=False (aggregate.py:575-577)."""
        keyspecs = []
        for gi in group_idx:
            col = cols[gi]
            if col.dtype in (rt.F64, rt.F32):
                if len(group_idx) != 1:
                    raise RexCompileError(
                        "a float GROUP BY key must be the only key "
                        "(densify composites first)")
                keyspecs.append((gi, 0, 0, True, 1))
                continue
            if col.dtype not in _INT_KINDS:
                raise RexCompileError(
                    "unsupported GROUP BY key dtype on GPU path")
            mn, rng = keys.key_range(runtime, col)
            keyspecs.append((gi, mn, rng, bool(col.validity)))
        return keyspecs

    @staticmethod
    def _densify_float_keys(runtime, cols, group_idx, force=False):
        """Composite key sets with float columns: each float key becomes a
        dense integer id (distinct floats via the bits-mode groupby, ids
        assigned by table position, joined back per row) so radix packing
        applies; the output restores the float via a host LUT. Returns
        (cols2, group_idx2, restore {key_pos: np.float64 LUT})."""
        if (len(group_idx) <= 1 and not force) or not any(
                cols[gi].dtype in (rt.F64, rt.F32) for gi in group_idx):
            return cols, group_idx, {}
        cols = list(cols)
        group_idx = list(group_idx)
        restore = {}
        for j, gi in enumerate(group_idx):
            col = cols[gi]
            if col.dtype not in (rt.F64, rt.F32):
                continue
            oc, ov, on, G = runtime.hash_groupby(
                [col], col.len, [(0, 0, 0, True, 1)], None, [])
            runtime._free(ov)
            runtime._free(on)
            codes = np.empty(max(G, 1), dtype=np.uint64)
            if G:
                runtime._download(oc, codes)
            codes = codes[:G]
            lut = np.where(codes > 0, codes - 1, 0).astype(
                np.uint64).view(np.float64)
            lut = np.where(codes > 0, lut, np.nan)

            class _H:
                def __init__(s, rt_, ptrs):
                    s.rt = rt_
                    s.ptrs = ptrs

                def __del__(s):
                    for p in s.ptrs:
                        try:
                            s.rt._free(p)
                        except Exception:
                            pass

            h = _H(runtime, [oc])
            bcol = rt.DeviceColumn(runtime, oc, None, G, rt.I64,
                                   owner=False, keep_alive=h)
            pcodes, _ = runtime.keypack([col], [(0, 0, 0, True, 1)],
                                        col.len)
            table = runtime.hash_build(bcol, None, code_max=0)
            try:
                p, b, cnt = runtime.hash_probe(table, pcodes,
                                               rt.JOIN_INNER, None)
                psel = runtime.wrap_sel(p, cnt)
                bsel = runtime.wrap_sel(b, cnt)
                assert cnt == col.len, (cnt, col.len)
                fid = runtime.scatter_rows(bsel, psel.data, cnt, col.len,
                                           with_validity=False)
            finally:
                runtime.hash_table_free(table)
            cols.append(fid)
            restore[j] = lut
            group_idx[j] = len(cols) - 1
        return cols, group_idx, restore

    def _convert_device(self, runtime, rel, dc, cols, keyspecs, group_idx,
                        filt_idx, calls, agg, name_idx=None,
                        key_restore=None):
        """Single-bucket kernel over the already-converted input."""
        specs = []
        fins = []
        slab = []
        for call in calls:
            speclist, fin = self._agg_spec_for(agg, call, cols)
            slab.append(len(specs))
            for op, prog in speclist:
                specs.append((op, runtime.make_prog(prog)))
            fins.append(fin)
        pred_prog = runtime.make_prog([(OP_COL, filt_idx, 0)]) \
            if filt_idx is not None else None
        cc_in = dc.column_container
        names = name_idx if name_idx is not None else group_idx
        group_meta = [(cc_in.columns[ni], cols[gi])
                      for ni, gi in zip(names, group_idx)]
        return self._device_exec(runtime, rel, cols, dc.table.num_rows,
                                 keyspecs, group_meta, pred_prog, calls,
                                 specs, fins, slab,
                                 key_restore=key_restore or {})

    def _device_exec(self, runtime, rel, cols, n_rows, keyspecs, group_meta,
                     pred_prog, calls, specs, fins, slab=None,
                     key_restore=None):
        """Run the fused kernel; finalize device-resident.
        slab[i] = first kernel-slot index of call i (stddev family spans 2)."""
        from dask_sql_amd.physical.rex import (OP_LIT_I64, OP_GT_I64,
                                               OP_LIT_NULL, OP_SELECT,
                                               OP_DIV_F64, OP_I64_TO_F64)
        if slab is None:
            slab = list(range(len(calls)))
        import os
        if (group_meta and not key_restore
                and all(f in runtime.GB_FIN_KINDS for f in fins)
                and os.environ.get("DSX_DISABLE_GBFINISH") != "1"):
            # keys unpacked and calls finalized by the group-by itself, one
            # launch for all output columns (dsx_hash_groupby_cols). Densified
            # float keys (host LUT) and the stddev family keep the code below.
            kcols, acols, G = runtime.hash_groupby_cols(
                cols, n_rows, keyspecs, pred_prog, specs,
                list(zip(fins, slab)))
            return self._finished_output(
                rel, group_meta, kcols, calls, acols,
                [len(ks) > 4 and ks[4] == 1 for ks in keyspecs])
        oc, ov, on, G = runtime.hash_groupby(cols, n_rows,
                                             keyspecs, pred_prog, specs)

        if G == 0 and not group_meta:
            # global aggregate over zero selected rows: SQL mandates ONE row
            # (COUNT = 0, everything else NULL) — reference aggregate.py:251
            # agg-on-whole-frame path
            runtime._free(oc)
            runtime._free(ov)
            runtime._free(on)
            out_cols = {}
            order_names = []
            for call, fin in zip(calls, fins):
                name = call.toString()
                if fin == "count":
                    col = runtime.upload_column(np.zeros(1, dtype=np.int64))
                else:
                    f64 = fin in ("avg", "sum_f", "min_f", "max_f") \
                        or fin in self.STD_FINS
                    col = runtime.upload_column(
                        np.zeros(1, dtype=np.float64 if f64 else np.int64),
                        validity=np.zeros(1, dtype=np.uint8))
                out_cols[f"a__{name}"] = col
                order_names.append((name, f"a__{name}"))
            cc = ColumnContainer([n for n, _ in order_names],
                                 dict(order_names))
            cc = self.fix_column_to_row_type(cc, rel.getRowType())
            return DataContainer(DeviceTable(out_cols, num_rows=1), cc)

        class _Holder:
            def __init__(self, runtime, ptrs):
                self.runtime = runtime
                self.ptrs = ptrs

            def __del__(self):
                for p in self.ptrs:
                    try:
                        self.runtime._free(p)
                    except Exception:
                        pass

        holder = _Holder(runtime, [oc, ov, on])
        codes_col = rt.DeviceColumn(runtime, oc, None, G, rt.I64, owner=False,
                                    keep_alive=holder)

        out_cols = {}
        order_names = []

        # group keys: unpack on device — part = (code / stride) % space
        from dask_sql_amd.physical.rex import OP_BITS_F64, OP_SUB_I64
        stride = 1
        key_restore = key_restore or {}
        for j, (ks, (name, src)) in enumerate(zip(keyspecs, group_meta)):
            gi, mn, rng, nullable = ks[:4]
            if j in key_restore:
                # densified float key: unpack the dense id, restore the
                # float through the host LUT (small: one value per distinct)
                space = rng + (1 if nullable else 0)
                prog = [(OP_COL, 0, 0), (OP_LIT_I64, 0, stride), (17, 0, 0),
                        (OP_LIT_I64, 0, space), (18, 0, 0),
                        (OP_LIT_I64, 0, mn), (14, 0, 0)]
                stride *= space
                fid_col = runtime.eval(runtime.make_prog(prog), [codes_col],
                                       G, rt.I64, with_validity=False)
                fid = np.empty(G, dtype=np.int64)
                if G:
                    runtime._download(fid_col.data, fid)
                lut = key_restore[j]
                vals = lut[np.clip(fid, 0, max(len(lut) - 1, 0))] \
                    if len(lut) else np.full(G, np.nan)
                nanm = np.isnan(vals)
                col = runtime.upload_column(
                    np.where(nanm, 0.0, vals),
                    validity=(~nanm).astype(np.uint8) if nanm.any()
                    else None)
                out_cols[f"g__{name}"] = col
                order_names.append((name, f"g__{name}"))
                continue
            if len(ks) > 4 and ks[4] == 1:
                # f64-bits key: value = bitcast(code-1); code 0 = NaN/NULL.
                # code != 0, not code > 0: the code of a negative double has
                # its top bit set and is negative as an i64
                from dask_sql_amd.physical.rex import OP_NE_I64
                prog = [(OP_COL, 0, 0), (OP_LIT_I64, 0, 0),
                        (OP_NE_I64, 0, 0),
                        (OP_COL, 0, 0), (OP_LIT_I64, 0, 1), (OP_SUB_I64, 0, 0),
                        (OP_BITS_F64, 0, 0),
                        (OP_LIT_NULL, 0, 0), (OP_SELECT, 0, 0)]
                col = runtime.eval(runtime.make_prog(prog), [codes_col], G,
                                   rt.F64, with_validity=True)
                col.logical_dtype = src.dtype
                out_cols[f"g__{name}"] = col
                order_names.append((name, f"g__{name}"))
                continue
            space = rng + (1 if nullable else 0)
            prog = [(OP_COL, 0, 0), (OP_LIT_I64, 0, stride), (17, 0, 0),
                    (OP_LIT_I64, 0, space), (18, 0, 0)]  # DIV, MOD
            if nullable:
                # SELECT(part > 0, part - 1 + mn, NULL)
                prog = prog + [
                    (OP_LIT_I64, 0, 0), (OP_GT_I64, 0, 0),
                ]
                # need part again: recompute (cheap G rows)
                prog += [(OP_COL, 0, 0), (OP_LIT_I64, 0, stride), (17, 0, 0),
                         (OP_LIT_I64, 0, space), (18, 0, 0),
                         (OP_LIT_I64, 0, 1), (15, 0, 0),  # SUB
                         (OP_LIT_I64, 0, mn), (14, 0, 0),  # ADD
                         (OP_LIT_NULL, 0, 0), (OP_SELECT, 0, 0)]
            else:
                prog += [(OP_LIT_I64, 0, mn), (14, 0, 0)]  # ADD
            stride *= space
            col = runtime.eval(runtime.make_prog(prog), [codes_col], G,
                               rt.I64, with_validity=nullable)
            if getattr(src, "dictionary", None) is not None:
                col.dictionary = src.dictionary
            col.logical_dtype = src.dtype
            out_cols[f"g__{name}"] = col
            order_names.append((name, f"g__{name}"))

        # agg finalize on device over (vals_a, cnts_a) slabs
        from dask_sql_amd.physical.rex import (OP_LIT_F64, OP_GE_I64,
                                               OP_SUB_I64, OP_SUB_F64,
                                               OP_MUL_F64, OP_GT_F64,
                                               OP_SQRT_F64)
        for call, fin, s in zip(calls, fins, slab):
            name = call.toString()
            val_col = rt.DeviceColumn(runtime, ov + s * G * 8, None, G,
                                      rt.F64 if fin in ("avg", "sum_f",
                                                        "min_f", "max_f")
                                      or fin in self.STD_FINS
                                      else rt.I64,
                                      owner=False, keep_alive=holder)
            cnt_col = rt.DeviceColumn(runtime, on + s * G * 8, None, G,
                                      rt.I64, owner=False, keep_alive=holder)
            if fin == "count":
                out = cnt_col  # always valid
            elif fin in self.STD_FINS:
                # moments: slot s = Σx (f64), slot s+1 = Σx², count = non-NULL
                # x per group. m2 = Σx² − (Σx)²/n, clamped at 0 (fp rounding),
                # ÷ (n−ddof); NULL below the minimum count (pandas ddof rules)
                sq_col = rt.DeviceColumn(runtime, ov + (s + 1) * G * 8, None,
                                         G, rt.F64, owner=False,
                                         keep_alive=holder)
                pop = fin.endswith("_pop")
                prog_var = [(OP_COL, 1, 0),                       # Σx²
                            (OP_COL, 0, 0), (OP_COL, 0, 0),
                            (OP_MUL_F64, 0, 0),                   # (Σx)²
                            (OP_COL, 2, 0), (OP_I64_TO_F64, 0, 0),
                            (OP_DIV_F64, 0, 0), (OP_SUB_F64, 0, 0)]  # m2
                if pop:
                    prog_var += [(OP_COL, 2, 0), (OP_I64_TO_F64, 0, 0),
                                 (OP_DIV_F64, 0, 0)]
                else:
                    prog_var += [(OP_COL, 2, 0), (OP_LIT_I64, 0, 1),
                                 (OP_SUB_I64, 0, 0), (OP_I64_TO_F64, 0, 0),
                                 (OP_DIV_F64, 0, 0)]
                var_col = runtime.eval(runtime.make_prog(prog_var),
                                       [val_col, sq_col, cnt_col], G, rt.F64,
                                       with_validity=False)
                mink = 1 if pop else 2
                prog_fin = [(OP_COL, 1, 0), (OP_LIT_I64, 0, mink),
                            (OP_GE_I64, 0, 0),
                            (OP_COL, 0, 0), (OP_LIT_F64, 0, 0.0),
                            (OP_GT_F64, 0, 0),
                            (OP_COL, 0, 0), (OP_LIT_F64, 0, 0.0),
                            (OP_SELECT, 0, 0)]                   # max(var, 0)
                if fin.startswith("std"):
                    prog_fin += [(OP_SQRT_F64, 0, 0)]
                prog_fin += [(OP_LIT_NULL, 0, 0), (OP_SELECT, 0, 0)]
                out = runtime.eval(runtime.make_prog(prog_fin),
                                   [var_col, cnt_col], G, rt.F64)
            elif fin == "avg":
                prog = [(OP_COL, 1, 0), (OP_LIT_I64, 0, 0), (OP_GT_I64, 0, 0),
                        (OP_COL, 0, 0),
                        (OP_COL, 1, 0), (OP_I64_TO_F64, 0, 0),
                        (OP_DIV_F64, 0, 0),
                        (OP_LIT_NULL, 0, 0), (OP_SELECT, 0, 0)]
                out = runtime.eval(runtime.make_prog(prog),
                                   [val_col, cnt_col], G, rt.F64)
            else:
                # SUM/MIN/MAX: NULL when no non-NULL input in group
                # (custom_sum min_count=1, aggregate.py:486-493)
                prog = [(OP_COL, 1, 0), (OP_LIT_I64, 0, 0), (OP_GT_I64, 0, 0),
                        (OP_COL, 0, 0), (OP_LIT_NULL, 0, 0),
                        (OP_SELECT, 0, 0)]
                dtype = rt.F64 if fin in ("sum_f", "min_f", "max_f") else rt.I64
                out = runtime.eval(runtime.make_prog(prog),
                                   [val_col, cnt_col], G, dtype)
            out_cols[f"a__{name}"] = out
            order_names.append((name, f"a__{name}"))

        cc = ColumnContainer([n for n, _ in order_names], dict(order_names))
        cc = self.fix_column_to_row_type(cc, rel.getRowType())
        return DataContainer(DeviceTable(out_cols), cc)

    # ------------------------------------------------------------------
    def _agg_spec_for(self, agg, call, cols):
        """([(kernel op, program), ...], finalize) for one agg call."""
        func = agg.getAggregationFuncName(call).lower()
        args = agg.getArgs(call)
        return self._agg_spec_expr(func, args[0] if args else None, cols,
                                   _dicts_of(cols))

    def _agg_spec_expr(self, func, expr, cols, dicts):
        if expr is not None:
            prog, kind = compile_expr(expr, cols, dicts)
        else:
            prog, kind = [(3, 0, 1)], KI  # LIT_I64 1 — COUNT(*)
        if func == "count":
            return [(rt.AGG_COUNT, prog)], "count"
        if func == "avg":
            if kind != KF:
                prog = prog + [(50, 0, 0)]  # I64_TO_F64
            return [(rt.AGG_SUM_F64, prog)], "avg"
        if func == "sum":
            if kind == KF:
                return [(rt.AGG_SUM_F64, prog)], "sum_f"
            return [(rt.AGG_SUM_I64, prog)], "sum_i"
        if func in ("every", "bool_and", "bool_or"):
            # boolean aggregates = MIN/MAX over {0,1} ignoring NULLs
            # (reference aggregate.py AGGREGATION_MAPPING every/bool ops)
            if kind != KB:
                raise RexCompileError(f"{func} needs a boolean argument")
            op_ = rt.AGG_MIN_I64 if func in ("every", "bool_and") \
                else rt.AGG_MAX_I64
            return [(op_, prog)], "min_i" if func != "bool_or" else "max_i"
        if func in ("min", "any_value", "single_value"):
            return ([((rt.AGG_MIN_F64 if kind == KF else rt.AGG_MIN_I64),
                      prog)],
                    ("min_f" if kind == KF else "min_i"))
        if func == "max":
            return ([((rt.AGG_MAX_F64 if kind == KF else rt.AGG_MAX_I64),
                      prog)],
                    ("max_f" if kind == KF else "max_i"))
        if func in ("stddev", "stddev_samp", "stddev_pop", "var_samp",
                    "var_pop", "variance"):
            if kind != KF:
                prog = prog + [(50, 0, 0)]  # I64_TO_F64
            sq = prog + prog + [(12, 0, 0)]  # MUL_F64 (x·x, NULL iff x NULL)
            fin = {"stddev": "std_samp", "stddev_samp": "std_samp",
                   "stddev_pop": "std_pop", "var_samp": "var_samp",
                   "variance": "var_samp", "var_pop": "var_pop"}[func]
            return [(rt.AGG_SUM_F64, prog), (rt.AGG_SUM_F64, sq)], fin
        raise RexCompileError(f"aggregate {func}")

    def _run_bucket(self, runtime, agg, dc, cols, keyspecs, filt_idx, calls):
        """One fused kernel pass. Returns (codes np.uint64 sorted,
        [(vals np | tuple of np, cnts np) per call]) — stddev-family calls
        carry a (Σx, Σx²) tuple."""
        pred_prog = None
        if filt_idx is not None:
            pred_prog = runtime.make_prog([(OP_COL, filt_idx, 0)])
        specs = []
        fins = []
        slab = []
        for call in calls:
            speclist, fin = self._agg_spec_for(agg, call, cols)
            slab.append(len(specs))
            for op, prog in speclist:
                specs.append((op, runtime.make_prog(prog)))
            fins.append(fin)
        nspec = len(specs)
        oc, ov, on, G = runtime.hash_groupby(cols, dc.table.num_rows,
                                             keyspecs, pred_prog, specs)
        codes = np.empty(G, dtype=np.uint64)
        if G:
            runtime._download(oc, codes)
        vals_all = np.empty(G * max(nspec, 1), dtype=np.uint64)
        cnts_all = np.empty(G * max(nspec, 1), dtype=np.uint64)
        if G and specs:
            runtime._download(ov, vals_all)
            runtime._download(on, cnts_all)
        runtime._free(oc)
        runtime._free(ov)
        runtime._free(on)
        # sort by code for deterministic output & merging
        order = np.argsort(codes, kind="stable")
        codes = codes[order]

        def slot(a, as_f64):
            u = vals_all[a * G:(a + 1) * G][order] if G else \
                np.empty(0, dtype=np.uint64)
            return u.view(np.float64) if as_f64 else u.view(np.int64)

        percall = []
        for fin, s in zip(fins, slab):
            cnts = cnts_all[s * G:(s + 1) * G][order] if G else \
                np.empty(0, dtype=np.uint64)
            if fin in self.STD_FINS:
                vals = (slot(s, True), slot(s + 1, True))
            elif fin in ("avg", "sum_f", "min_f", "max_f"):
                vals = slot(s, True)
            else:
                vals = slot(s, False)
            percall.append((vals, cnts))
        return codes, percall

    def _distinct_bucket(self, runtime, agg, dc, cols, keyspecs, filt_idx,
                         calls):
        """SUM/AVG/COUNT(DISTINCT x): two-level groupby — first
        (group, x) distinct pairs, then aggregate (aggregate.py:562-565)."""
        if any(len(k) > 4 and k[4] == 1 for k in keyspecs):
            raise RexCompileError(
                "DISTINCT aggregate with a float GROUP BY key")
        float_ids = {}
        for call in calls:
            args = agg.getArgs(call)
            if not args or not isinstance(args[0], InputRef):
                raise RexCompileError("DISTINCT agg needs a plain column")
            ci = args[0].getIndex()
            if cols[ci].dtype == rt.F64:
                fname = agg.getAggregationFuncName(call).lower()
                if fname != "count":
                    raise RexCompileError(
                        "SUM/AVG DISTINCT on a float column (COUNT "
                        "DISTINCT densifies; value-carrying distincts "
                        "are round-3)")
                # COUNT(DISTINCT f64): only DISTINCTNESS matters — give
                # each bit-canonical value a dense id (same primitive
                # chain as _densify_float_keys) and count ids
                if ci not in float_ids:
                    col = cols[ci]
                    n_ = col.len
                    oc, ov, on_, G = runtime.hash_groupby(
                        [col], n_, [(0, 0, 0, True, 1)], None, [])
                    runtime._free(ov)
                    runtime._free(on_)
                    bcol = rt.DeviceColumn(runtime, oc, None, max(G, 1),
                                           rt.I64, owner=True)
                    pcodes, _ = runtime.keypack([col], [(0, 0, 0, True, 1)],
                                                n_)
                    table = runtime.hash_build(bcol, None, code_max=0)
                    try:
                        p_, b_, cnt = runtime.hash_probe(
                            table, pcodes, rt.JOIN_INNER, None)
                        psel = runtime.wrap_sel(p_, cnt)
                        bsel = runtime.wrap_sel(b_, cnt)
                        fid = runtime.scatter_rows(bsel, psel.data, cnt,
                                                   n_,
                                                   with_validity=False)
                    finally:
                        runtime.hash_table_free(table)
                    # scattered build positions are 4-byte ids (fid.dtype)
                    idcol = rt.DeviceColumn(runtime, fid.data,
                                            col.validity, n_, fid.dtype,
                                            owner=False,
                                            keep_alive=(fid, col))
                    cols = list(cols)
                    cols.append(idcol)
                    float_ids[ci] = len(cols) - 1
            elif cols[ci].dtype not in _INT_KINDS:
                raise RexCompileError("DISTINCT agg on non-integer key "
                                      "type")
        # distinct over (group keys + arg col): one kernel with extended keys
        out = []
        codes_ref = None
        for call in calls:
            ai = agg.getArgs(call)[0].getIndex()
            ai = float_ids.get(ai, ai)
            mn, rng = keys.key_range(runtime, cols[ai])
            ks2 = keyspecs + [(ai, mn, rng, bool(cols[ai].validity))]
            pred_prog = runtime.make_prog([(OP_COL, filt_idx, 0)]) \
                if filt_idx is not None else None
            oc, ov, on, G = runtime.hash_groupby(cols, dc.table.num_rows,
                                                 ks2, pred_prog, [])
            pairs = np.empty(G, dtype=np.uint64)
            if G:
                runtime._download(oc, pairs)
            runtime._free(oc)
            runtime._free(ov)
            runtime._free(on)
            # unpack: group code = pairs % group_space; value part on top
            group_space = 1
            for ks in keyspecs:
                _, _, rng, nullable = ks[:4]
                if len(ks) > 4 and ks[4] == 1:
                    raise RexCompileError(
                        "DISTINCT aggregate with a float GROUP BY key")
                group_space *= rng + (1 if nullable else 0)
            gcodes = pairs % group_space
            vpart = pairs // group_space
            a_nullable = bool(cols[ai].validity)
            if a_nullable:
                valid = vpart != 0
                vvals = vpart.astype(np.int64) - 1 + mn
            else:
                valid = np.ones(len(vpart), dtype=bool)
                vvals = vpart.astype(np.int64) + mn
            func = agg.getAggregationFuncName(call).lower()
            # aggregate per group on host (distinct pair count is small)
            uniq, inv = np.unique(gcodes, return_inverse=True)
            if func == "count":
                vals = np.zeros(len(uniq), dtype=np.int64)
                np.add.at(vals, inv[valid], 1)
                cnts = vals.astype(np.uint64)
            elif func in ("sum", "avg"):
                s = np.zeros(len(uniq), dtype=np.float64)
                np.add.at(s, inv[valid], vvals[valid].astype(np.float64))
                c = np.zeros(len(uniq), dtype=np.int64)
                np.add.at(c, inv[valid], 1)
                if func == "sum":
                    vals = s.astype(np.int64) if True else s
                    vals = np.where(c > 0, s, 0).astype(np.int64)
                else:
                    vals = s  # finalized later as avg: sum/count
                cnts = c.astype(np.uint64)
            else:
                raise RexCompileError(f"DISTINCT {func} (round-2)")
            out.append((vals, cnts))
            codes_ref = uniq
        return codes_ref, out

    # ------------------------------------------------------------------
    def _build_output(self, runtime, rel, dc, keyspecs, group_idx, codes_np,
                      agg_calls, merged, name_idx=None, key_restore=None):
        """Unpack group codes → key columns; finalize agg columns
        (SUM min_count=1 → NULL on zero count; AVG = sum/count)."""
        G = len(codes_np)
        if G == 0 and not keyspecs and agg_calls:
            # global aggregate over zero rows → ONE row (COUNT=0, rest NULL);
            # zero-count synthesis lets the normal finalize below produce it
            codes_np = np.zeros(1, dtype=np.uint64)
            fixed = {}
            for k, (vals, cnts) in merged.items():
                if isinstance(vals, tuple):
                    vals = tuple(np.zeros(1, dtype=v.dtype) for v in vals)
                else:
                    vals = np.zeros(1, dtype=vals.dtype)
                fixed[k] = (vals, np.zeros(1, dtype=np.uint64))
            merged = fixed
            G = 1
        out_cols = {}
        order_names = []
        cols = dc.backend_cols()
        cc_in = dc.column_container

        # group key columns
        stride = 1
        key_restore = key_restore or {}
        names = name_idx if name_idx is not None else group_idx
        for j, ks in enumerate(keyspecs):
            gi, mn, rng, nullable = ks[:4]
            ni = names[j]
            if j in key_restore:
                space = rng + (1 if nullable else 0)
                fid = ((codes_np // stride) % space).astype(np.int64) + mn
                stride *= space
                lut = key_restore[j]
                vals = lut[np.clip(fid, 0, max(len(lut) - 1, 0))] \
                    if len(lut) else np.full(G, np.nan)
                nanm = np.isnan(vals)
                col = runtime.upload_column(
                    np.where(nanm, 0.0, vals),
                    validity=(~nanm).astype(np.uint8) if nanm.any()
                    else None)
                name = cc_in.columns[ni]
                out_cols[f"g__{name}"] = col
                order_names.append((name, f"g__{name}"))
                continue
            if len(ks) > 4 and ks[4] == 1:
                # f64-bits key (host path): bitcast(code-1), code 0 → NaN
                src = cols[gi]
                vals = np.where(codes_np > 0,
                                (codes_np - 1).astype(np.uint64),
                                np.uint64(0)).view(np.float64)
                vals = np.where(codes_np > 0, vals, np.nan)
                col = runtime.upload_column(vals.astype(np.float64))
                name = cc_in.columns[ni]
                out_cols[f"g__{name}"] = col
                order_names.append((name, f"g__{name}"))
                continue
            space = rng + (1 if nullable else 0)
            part = (codes_np // stride) % space
            stride *= space
            src = cols[gi]
            if nullable:
                valid = part != 0
                vals = part.astype(np.int64) - 1 + mn
                vals[~valid] = 0
            else:
                valid = None
                vals = part.astype(np.int64) + mn
            np_dtype = {rt.I64: np.int64, rt.I32: np.int32, rt.I8: np.int8,
                        rt.BOOL8: np.uint8}[src.dtype]
            col = runtime.upload_column(
                vals.astype(np_dtype),
                validity=valid.astype(np.uint8) if valid is not None else None,
                dtype=src.dtype)
            if getattr(src, "dictionary", None) is not None:
                col.dictionary = src.dictionary
            name = cc_in.columns[ni]
            out_cols[f"g__{name}"] = col
            order_names.append((name, f"g__{name}"))

        # agg columns
        for call in agg_calls:
            name = call.toString()
            vals, cnts = merged[name]
            agg_obj = rel.aggregate()
            func = agg_obj.getAggregationFuncName(call).lower()
            has_null = (cnts == 0).any()
            if func == "count":
                col = runtime.upload_column(cnts.astype(np.int64))
            elif func in ("stddev", "stddev_samp", "stddev_pop", "var_samp",
                          "var_pop", "variance"):
                s, ss = vals  # (Σx, Σx²) moments from the two kernel slots
                pop = func.endswith("_pop")
                n = cnts.astype(np.float64)
                with np.errstate(invalid="ignore", divide="ignore"):
                    m2 = np.maximum(ss - s * s / n, 0.0)
                    v = m2 / (n if pop else n - 1.0)
                if func.startswith("stddev"):
                    v = np.sqrt(v)
                ok = cnts >= (1 if pop else 2)
                v = np.where(ok, v, 0.0)
                col = runtime.upload_column(
                    v, validity=ok.astype(np.uint8) if not ok.all() else None)
            elif func == "avg":
                with np.errstate(invalid="ignore", divide="ignore"):
                    a = vals.astype(np.float64) / cnts.astype(np.float64)
                col = runtime.upload_column(
                    a, validity=(cnts > 0).astype(np.uint8) if has_null
                    else None)
            else:
                if vals.dtype == np.float64:
                    col = runtime.upload_column(
                        vals, validity=(cnts > 0).astype(np.uint8)
                        if has_null else None)
                else:
                    col = runtime.upload_column(
                        vals.astype(np.int64),
                        validity=(cnts > 0).astype(np.uint8) if has_null
                        else None)
            out_cols[f"a__{name}"] = col
            order_names.append((name, f"a__{name}"))

        if not out_cols:  # zero groups, zero aggs
            pass
        cc = ColumnContainer([n for n, _ in order_names], dict(order_names))
        cc = self.fix_column_to_row_type(cc, rel.getRowType())
        return DataContainer(DeviceTable(out_cols), cc)


class DaskSortPlugin(BaseRelPlugin):
    """ORDER BY (reference physical/utils/sort.py:9-60, pandas mergesort
    per partition). convert sorts tables of at least DSX_SORT_MIN rows
    through _device_sort and everything else, or whatever that declines,
    with pandas on the host.

    _device_sort resolves every collation key once into a key record
    (physical/keys.py owns that: a key's range, the rank column of a
    dictionary string key, the dtypes the device sorts), adds the ORDER BY
    mode bits (2 = DESC, 4 = NULLS LAST), and feeds one of two engines
    from the same records, then gathers each column through the
    permutation:

    - all keys integer-kind (ints, dates, bools, ranked dictionary
      strings): order-preserving packed codes → range partition →
      per-bucket LDS bitonic (dsx_sort_perm, stable via rowid tiebreak;
      VERDICT r1 #6);
    - any float key, or dsx_sort_perm declining (skew-overloaded bucket,
      key space > 2^62, more than 4 keys, a table wider than 16 columns):
      the radix chain — plan_sort_words cuts the records into 64-bit
      words and keys.run_words runs dsx_sort_word (stable LSD radix) over
      them least significant first.

    It declines (→ host) key dtypes the device does not hold and a single
    integer key spanning more than 2^62. DSX_DISABLE_RADIXSORT=1 turns the
    chain off (float keys and whatever dsx_sort_perm declines sort on the
    host again); DSX_SORT_RADIX=1 sends all-integer collations to the
    chain as well. Both are read per call."""

    class_name = "Sort"

    def convert(self, rel, context):
        import os as _os
        (dc,) = self.assert_inputs(rel, 1, context, host_ok=True)
        min_dev = int(_os.environ.get("DSX_SORT_MIN", 65536))
        if isinstance(dc, DataContainer) and dc.table.num_rows >= min_dev:
            out = self._device_sort(context, dc, rel.sort().getCollation())
            if out is not None:
                return out
        from dask_sql_amd.materialize import to_pandas
        pdf = to_pandas(dc, context)
        for idx, asc, nulls_first in reversed(rel.sort().getCollation()):
            col = pdf.columns[idx]
            pdf = pdf.sort_values(
                col, ascending=asc,
                na_position="first" if nulls_first else "last",
                kind="mergesort")
        return HostDataContainer(pdf.reset_index(drop=True))

    def _device_sort(self, context, dc, collation):
        import os as _os
        from dask_sql_amd.physical.sort_words import plan_sort_words
        runtime = context._get_runtime()
        work = list(dc.backend_cols())  # + rank columns of dictionary keys
        n = dc.table.num_rows
        use_radix = _os.environ.get("DSX_DISABLE_RADIXSORT", "0") != "1"
        force_radix = use_radix and \
            _os.environ.get("DSX_SORT_RADIX", "0") == "1"
        recs = []
        for idx, asc, nulls_first in collation:
            mode = (2 if not asc else 0) | (0 if nulls_first else 4)
            rec = keys.key_record(runtime, work, n, idx, mode, rank=True)
            if rec is None or (rec[1] and not use_radix):
                return None  # float keys on host, as before the chain
            recs.append(rec)
        perm = None
        if not force_radix and not any(rec[1] for rec in recs):
            # first ORDER BY key → highest stride: pass reversed
            perm = runtime.sort_perm(
                work, [keys.bucket_spec(rec) for rec in reversed(recs)], n)
        if perm is None and use_radix:
            perm = keys.run_words(runtime, plan_sort_words(recs), work, n)
        if perm is None:
            return None
        cc = dc.column_container
        out_cols = {}
        for f in cc.columns:
            b = cc.get_backend_by_frontend_name(f)
            if b in out_cols:
                continue
            src = dc.table.col(b)
            g = runtime.gather(src, perm.data, n, bool(src.validity))
            if getattr(src, "dictionary", None) is not None:
                g.dictionary = src.dictionary
            g._stats_src = src
            out_cols[b] = g
        return DataContainer(DeviceTable(out_cols, num_rows=n), cc)


class DaskLimitPlugin(BaseRelPlugin):
    """LIMIT/OFFSET (reference rel/logical/limit.py:24-113). Sort+Limit is
    fused into a top-k (the reference's apply_sort topk optimization,
    physical/utils/sort.py:9-34 / sql.yaml topk-nelem-limit): argpartition
    the primary key, full-sort only the candidate set."""

    class_name = "Limit"

    def convert(self, rel, context):
        node = rel.limit()
        below = rel.get_inputs()[0]
        ncols_in = max(1, len(below.getRowType().getFieldList()))
        from dask_sql_amd import config as _config
        nelem_limit = _config.get("sql.sort.topk-nelem-limit", 1_000_000)
        if (below.get_current_node_type() == "Sort"
                and node.fetch is not None
                and (node.fetch + node.offset) * ncols_in <= nelem_limit):
            (inp,) = self.assert_inputs(below, 1, context, host_ok=True)
            keys = below.sort().getCollation()
            k = node.fetch + node.offset
            from dask_sql_amd.materialize import to_pandas
            if isinstance(inp, DataContainer):
                # device top-k: sampled threshold + device filter keep only
                # ~k candidate rows; the full frame never leaves the GPU
                pdf = _device_topk_impl(context, inp, below, keys, k)
                if pdf is not None:
                    pdf = pdf.iloc[node.offset:]
                    return HostDataContainer(pdf.reset_index(drop=True))
            pdf = to_pandas(inp, context)
            pdf = _topk(pdf, keys, k).iloc[node.offset:]
            return HostDataContainer(pdf.reset_index(drop=True))
        (inp,) = self.assert_inputs(rel, 1, context, host_ok=True)
        if isinstance(inp, HostDataContainer):
            pdf = inp.pdf
        else:
            from dask_sql_amd.materialize import to_pandas
            pdf = to_pandas(inp, context)
        if node.offset:
            pdf = pdf.iloc[node.offset:]
        if node.fetch is not None:
            pdf = pdf.iloc[: node.fetch]
        return HostDataContainer(pdf.reset_index(drop=True))


def _device_topk_impl(context, inp, below, keys, k):
    """ORDER BY + LIMIT over a large result. k <= 1024 over a frame of at
    most 16 fixed-width columns: dsx_topk_rows selects the exact candidate
    rows and returns them with their columns in one host wait
    (_topk_select_device; DSX_DISABLE_TOPK=1, read per call, turns it
    off). Everything else, and what that call declines: device
    sampled-threshold
    selection — a strided device sample picks an approximate k-th key,
    a device filter keeps only rows at or beyond it, and the (tiny)
    candidate set is sorted exactly on host with full tie-breaking.
    Replaces the reference's topk_sort nsmallest/nlargest
    (physical/utils/sort.py:9-34) without downloading the column."""
    from dask_sql_amd.physical.rex import (OP_GE_F64, OP_GE_I64, OP_LE_F64,
                                           OP_LE_I64, OP_LIT_F64, OP_LIT_I64,
                                           OP_NE_F64)
    runtime = context._get_runtime()
    cc = inp.column_container
    n = inp.table.num_rows
    if n <= max(4 * k, 4096):
        return None  # small: plain path is fine
    idx0, asc0, _ = keys[0]
    col0 = inp.table.col(cc.get_backend_by_frontend_name(cc.columns[idx0]))
    if col0.dtype not in (rt.F64, rt.I64, rt.I32, rt.I8):
        return None  # unsupported key dtype: host fallback
    isf = col0.dtype == rt.F64
    # exact selection in one native call; whatever it declines (see
    # _topk_select_device) takes the sampled-threshold path below unchanged
    picked = _topk_select_device(runtime, inp, keys, k, n)
    if picked is not None:
        pdf = _topk_raw_frame(*picked, cc.columns, below, keys, k)
        if pdf is not None:
            return pdf
    # NULL/NaN keys are folded into the candidate filter below (they all
    # pass it and surface on host); no separate full scan + sync needed
    # strided device sample → approximate k-th order statistic. The index
    # vector depends only on (n, S): cached on the runtime across steps.
    S = int(min(16384, n))
    cache = getattr(runtime, "_topk_sample_cache", None)
    if cache is None:
        cache = runtime._topk_sample_cache = {}
    sel = cache.get((n, S))
    if sel is None:
        if len(cache) > 32:
            cache.clear()
        sel = runtime.upload_column(
            np.linspace(0, n - 1, S).astype(np.uint32), dtype=rt.I32)
        cache[(n, S)] = sel
    sv, _ = runtime.gather(col0, sel.data, S).to_numpy()
    if isf and np.isnan(sv).any():
        return None  # NaN in sample: host fallback (ordering on host)
    key_s = sv if asc0 else -sv.astype(np.float64 if isf else np.int64)
    cand_ptr = None
    cnt = 0
    r = min(S - 1, max(int(np.ceil(k * S / n * 4)) + 8, k))
    for _attempt in range(2):
        thr_key = np.partition(key_s, r)[r]  # native dtype (int precision)
        thr = thr_key if asc0 else -thr_key
        if isf:
            op = OP_LE_F64 if asc0 else OP_GE_F64
            prog = [(OP_COL, 0, 0), (OP_LIT_F64, 0, float(thr)), (op, 0, 0)]
        else:
            op = OP_LE_I64 if asc0 else OP_GE_I64
            prog = [(OP_COL, 0, 0), (OP_LIT_I64, 0, int(thr)), (op, 0, 0)]
        # NULL/NaN keys also become candidates (no separate scan); if any
        # survive to the host frame we fall back (see below)
        from dask_sql_amd.physical.rex import OP_IS_NULL, OP_OR
        if col0.validity:
            prog += [(OP_COL, 0, 0), (OP_IS_NULL, 0, 0), (OP_OR, 0, 0)]
        if isf:
            prog += [(OP_COL, 0, 0), (OP_COL, 0, 0), (OP_NE_F64, 0, 0),
                     (OP_OR, 0, 0)]
        cand_ptr, cnt = runtime.filter(runtime.make_prog(prog), [col0], n)
        if cnt >= k:
            break
        runtime.wrap_sel(cand_ptr, cnt)  # free; loosen and retry
        cand_ptr = None
        r = min(S - 1, r * 8)
    if cand_ptr is None or cnt < k or cnt > max(40 * k, 40_000):
        if cand_ptr is not None:
            runtime.wrap_sel(cand_ptr, cnt)
        return None  # sample missed or degenerate ties: host fallback
    sel2 = runtime.wrap_sel(cand_ptr, cnt)
    cand_dc = _gather_table(runtime, inp, sel2.data, cnt)
    # sort the candidates on their RAW columns (day-ints, codes) and
    # convert only the k winners — to_pandas on the full candidate set
    # (datetime/dict conversion of thousands of rows) measured ~1 ms/step
    # on the Q3 headline. Raw order == converted order for numeric and
    # DATE keys (monotone day-ints); dictionary sort keys bail out.
    ccc = cand_dc.column_container
    raws = []
    valids = []
    srcs = []
    for frontend in ccc.columns:
        col = cand_dc.table.col(ccc.get_backend_by_frontend_name(frontend))
        arr, valid = col.to_numpy()
        raws.append(arr)
        valids.append(valid)
        srcs.append(col)
    pdf = _topk_raw_frame(raws, valids, srcs, ccc.columns, below, keys, k)
    if pdf is not None:
        return pdf
    from dask_sql_amd.materialize import to_pandas
    pdf = to_pandas(cand_dc, context, below.getRowType())
    kcol = pdf.iloc[:, idx0]
    if kcol.isna().to_numpy().any():
        return None  # NULL/NaN keys present: exact NULLS ordering on host
    return _topk(pdf, keys, k)


def _topk_select_device(runtime, inp, keys, k, n):
    """The candidate rows through dsx_topk_rows (one host wait): exactly the
    rows whose primary key sorts at or before the k-th row's, in row order —
    the order the threshold filter of _device_topk_impl emits its candidates
    in, so ties break the same way. Returns (raws, valids, srcs) or None
    when the shape is not routed there (k > 1024, more than 16 columns, a
    dtype the call does not carry, a dictionary ORDER BY key,
    DSX_DISABLE_TOPK=1) or the call answers "not applicable"."""
    import os as _os
    if k > 1024 or _os.environ.get("DSX_DISABLE_TOPK", "0") == "1":
        return None
    cc = inp.column_container
    srcs = [inp.table.col(cc.get_backend_by_frontend_name(f))
            for f in cc.columns]
    if len(srcs) > rt.MAX_COLS or any(
            s.dtype not in (rt.I8, rt.I32, rt.I64, rt.F32, rt.F64)
            for s in srcs):
        return None
    if any(getattr(srcs[i], "dictionary", None) is not None
           for i, _a, _nf in keys):
        return None
    idx0, asc0, _ = keys[0]
    res = runtime.topk_rows(srcs, idx0, not asc0, n, k,
                            min(4096, max(4 * k, 1024)))
    if res is None:
        return None
    rowids, cols = res
    order = np.argsort(rowids, kind="stable")
    raws = [vals[order] for vals, _v in cols]
    valids = [v[order] if v is not None else None for _vals, v in cols]
    return raws, valids, srcs


def _topk_raw_frame(raws, valids, srcs, fronts, below, keys, k):
    """Top k of the candidate rows, ordered on their RAW columns (day-ints,
    codes), converting only the k winners. Returns None when raw order is
    not the converted order or NULLS placement matters: a dictionary key, a
    NULL or a NaN in a key column."""
    for i, _a, _nf in keys:
        if getattr(srcs[i], "dictionary", None) is not None:
            return None  # dict key: code order != string order
        if valids[i] is not None and not valids[i].all():
            return None
        if np.asarray(raws[i]).dtype.kind == "f" and \
                np.isnan(raws[i]).any():
            return None
    import pandas as pd

    # np.lexsort: last key = primary; DESC via exact negation (f64 and
    # sub-64-bit ints negate exactly in i64/f64; i64 at INT64_MIN bails)
    lex = []
    ok = True
    for i, a, _nf in keys:
        arr = np.asarray(raws[i])
        if a:
            lex.append(arr)
        elif arr.dtype.kind == "f":
            lex.append(-arr)
        else:
            a64 = arr.astype(np.int64)
            if a64.size and a64.min() == np.iinfo(np.int64).min:
                ok = False
                break
            lex.append(-a64)
    if ok:
        top = np.lexsort(tuple(reversed(lex)))[:k]
    else:
        raw_pdf = pd.DataFrame({j: raws[j] for j in range(len(raws))})
        by = [i for i, _a, _nf in keys]
        asc = [a for _i, a, _nf in keys]
        top = raw_pdf.sort_values(by, ascending=asc,
                                  kind="stable").index[:k].to_numpy()
    from dask_sql_amd.materialize import _convert
    fields = below.getRowType().getFieldList()
    data = {}
    for j, frontend in enumerate(fronts):
        sql_t = fields[j].getType().getSqlType() if j < len(fields) \
            else None
        v = valids[j][top] if valids[j] is not None else None
        data[frontend] = _convert(raws[j][top], v, srcs[j],
                                  sql_t).reset_index(drop=True)
    return pd.DataFrame(data)


def _topk(pdf, keys, k):
    """Exact multi-key top-k: candidates by primary key via argpartition
    (+ boundary ties), then the full mergesort ordering on candidates only."""
    n = len(pdf)
    if n > k:
        idx0, asc0, _ = keys[0]
        col0 = pdf.iloc[:, idx0].to_numpy()
        import numpy as _np
        v = col0 if asc0 else -_np.asarray(col0, dtype=_np.float64) \
            if col0.dtype.kind == "f" else (col0 if asc0 else -col0)
        v = _np.asarray(v)
        if _np.isnan(_np.asarray(v, dtype=float)).any() if v.dtype.kind == "f" \
                else False:
            cand = pdf  # NaN keys: fall back to full sort
        else:
            part = _np.argpartition(v, min(k - 1, n - 1))[:k]
            thresh = v[part].max()
            cand_mask = v <= thresh  # includes boundary ties
            if cand_mask.sum() > max(10 * k, 1000):
                cand = pdf  # degenerate ties: full sort
            else:
                cand = pdf[cand_mask]
    else:
        cand = pdf
    for idx, asc, nulls_first in reversed(keys):
        col = cand.columns[idx]
        cand = cand.sort_values(
            col, ascending=asc,
            na_position="first" if nulls_first else "last",
            kind="mergesort")
    return cand.iloc[:k]


class DaskWindowPlugin(BaseRelPlugin):
    """reference rel/logical/window.py:212-428 (OverOperation dispatch +
    map_on_each_group over sorted partitions). _one routes each window
    column to one of four device paths:

    - unordered partition aggregates (SUM/COUNT/AVG/MIN/MAX OVER
      (PARTITION BY …)), _device_agg: fused groupby, hash join-back of the
      per-group value, and a row scatter into original order;
    - ranking, LAG/LEAD/FIRST_VALUE and ordered (running, RANGE-peers
      default frame) aggregates, _device_ordered: the sort front half,
      then dsx_window_ordered (binary-search ranks / shifts,
      per-partition running scans with peer broadcast);
    - explicit ROWS frames (SUM/COUNT/AVG/MIN/MAX/FIRST_VALUE/LAST_VALUE
      over ROWS BETWEEN … AND … / ROWS k PRECEDING), _device_rows: the
      sort front half, then dsx_window_rows (LDS tile pass for narrow
      bounded frames, per-partition scans + prefix differences
      otherwise);
    - RANGE frames with value offsets (the same seven functions over
      RANGE BETWEEN … AND … with numeric or INTERVAL offsets),
      _device_range: the sort front half with peer ids, then
      dsx_window_range (frame bounds by binary search over the sorted
      order key, the same scans, a sparse table for MIN/MAX bounded on
      both sides). What it declines runs on the numpy model of the same
      SQL semantics (_host_range, physical/window_range.py), never on
      _frame_apply, which knows row offsets only.

    What the others decline runs as the reference computes it, in pandas
    per partition on the host (_host_ordered, _frame_apply;
    window.py:266-427 map_on_each_group), and the one result column is
    uploaded:
    DSX_DISABLE_DEVWINDOW set, a key dtype that is not device-sortable, a
    single integer key spanning more than 2^62, a dictionary-encoded
    value column, OVER () aggregates, or a bounded MIN/MAX frame wider
    than window_frames.WIN_ROWS_TILE_MAXW.

    The sort front half is _device_sort_keys. It resolves the
    (partition, order) keys once into key records — physical/keys.py owns
    a key's range, its rank column and the dtypes the device sorts — and
    feeds either the bucket sort + keypack codes (_bucket_ids; integer-kind
    keys that pack) or the sort_word chain + boundary marks + segment ids
    (_word_ids; float keys, explicit NULLS FIRST, skew, more than 4 keys,
    key spaces above 2^62, tables wider than 16 columns) from them. Knobs,
    read per call: DSX_DISABLE_DEVWINDOW (ordered and framed windows on
    the host), DSX_DISABLE_WINWORDS=1 (no word front half: those shapes
    run on the host as they did before it existed), DSX_WIN_WORDS=1 (every
    device window through the word front half; for A/B runs)."""

    class_name = "Window"

    def convert(self, rel, context):
        runtime = context._get_runtime()
        (dc,) = self.assert_inputs(rel, 1, context)
        cols = dc.backend_cols()
        cc_in = dc.column_container
        n = dc.table.num_rows
        out_cols = dict(dc.table.columns)
        order_names = [(f, cc_in.get_backend_by_frontend_name(f))
                       for f in cc_in.columns]
        for spec in rel.window().getWindowSpecs():
            col = self._one(runtime, cols, n, spec)
            bname = f"win__{spec.out_name}"
            out_cols[bname] = col
            order_names.append((spec.out_name, bname))
        cc = ColumnContainer([nm for nm, _ in order_names],
                             dict(order_names))
        cc = self.fix_column_to_row_type(cc, rel.getRowType())
        return DataContainer(DeviceTable(out_cols, num_rows=n), cc)

    _AGGS = {"sum", "count", "avg", "min", "max"}

    def _one(self, runtime, cols, n, spec):
        import os as _os
        if getattr(spec, "frame", None) is not None \
                and spec.frame[0] == "range":
            # RANGE frames with value offsets: dsx_window_range, or the
            # numpy model of the same semantics. Never _frame_apply, which
            # ignores the frame kind and would answer with row semantics:
            # tested before every route that ends in _host_ordered. An
            # explicit NULLS FIRST with the word front half off is declined
            # by _device_sort_keys and honoured by the host model
            col = self._device_range(runtime, cols, n, spec)
            if col is not None:
                return col
            return self._host_range(runtime, cols, n, spec)
        if any(nf is True for nf in getattr(spec, "order_nf", [])) \
                and _os.environ.get("DSX_DISABLE_WINWORDS", "0") == "1":
            # explicit NULLS FIRST on a window order key is sorted by the
            # word chain only (_device_sort_keys); with that off, the host
            # sort path honors per-key placement
            return self._host_ordered(runtime, cols, n, spec)
        if getattr(spec, "frame", None) is None \
                and spec.func == "last_value" and spec.order_idx \
                and spec.arg_idx is not None:
            # ordered default frame ends AT the current row, and the
            # reference's row-based expanding window makes LAST_VALUE the
            # current row's value (window.py LastValueOperation over
            # expanding) — a straight copy of the operand
            src = cols[spec.arg_idx]
            out = runtime.concat_columns([src], src.dtype)
            if getattr(src, "dictionary", None) is not None:
                out.dictionary = src.dictionary
            return out
        if getattr(spec, "frame", None) is not None:
            # explicit ROWS frames: device tile / scan kernels
            # (dsx_window_rows); shapes they do not cover run the
            # reference's own rolling pandas computation host-side
            # (window.py:145-198 map_on_each_group)
            col = self._device_rows(runtime, cols, n, spec)
            if col is not None:
                return col
            return self._host_ordered(runtime, cols, n, spec)
        device_ok = (spec.func in self._AGGS and not spec.order_idx
                     and spec.part_idx  # OVER () = whole-table agg → host
                     and all(cols[i].dtype in _INT_KINDS
                             for i in spec.part_idx))
        if device_ok:
            return self._device_agg(runtime, cols, n, spec)
        col = self._device_ordered(runtime, cols, n, spec)
        if col is not None:
            return col
        return self._host_ordered(runtime, cols, n, spec)

    def _frame_apply(self, df, grp, pnames, spec):
        """Explicit ROWS frame over sorted partitions — the reference's
        map_on_each_group expanding/rolling/Indexer chain restated
        (window.py:145-198)."""
        import pandas as pd
        fk, lo, hi = spec.frame
        if fk != "rows":
            # row offsets only: a RANGE frame answered here would be wrong
            # without an error (_one sends those to _host_range)
            raise RexCompileError(f"{fk.upper()} frame on the ROWS host path")
        f = spec.func
        src = "v" if spec.arg_idx is not None else "_one_"
        if src == "_one_":
            df["_one_"] = 1.0
            grp = df.groupby(pnames, dropna=False, sort=False)
        if lo[0] == "unbounded_preceding" and hi[0] == "current":
            roll = grp[src].expanding(min_periods=1)
        elif lo[0] == "preceding" and hi[0] == "current":
            roll = grp[src].rolling(window=lo[1] + 1, min_periods=1)
        else:
            from pandas.api.indexers import BaseIndexer

            lo_off = {"unbounded_preceding": None, "current": 0,
                      "preceding": -lo[1] if lo[1] is not None else None,
                      "following": lo[1]}[lo[0]]
            hi_off = {"unbounded_following": None, "current": 0,
                      "preceding": -hi[1] if hi[1] is not None else None,
                      "following": hi[1]}[hi[0]]

            class _Ix(BaseIndexer):
                def get_window_bounds(self, num_values=0, min_periods=None,
                                      center=None, closed=None, step=None):
                    i = np.arange(num_values, dtype=np.int64)
                    start = np.zeros(num_values, dtype=np.int64)                         if lo_off is None                         else np.clip(i + lo_off, 0, num_values)
                    end = np.full(num_values, num_values, dtype=np.int64)                         if hi_off is None                         else np.clip(i + hi_off + 1, 0, num_values)
                    return start, np.maximum(start, end)

            roll = grp[src].rolling(window=_Ix(), min_periods=1)
        if f == "sum":
            res = roll.sum()
        elif f == "count":
            res = roll.count()
        elif f == "avg":
            res = roll.mean()
        elif f == "min":
            res = roll.min()
        elif f == "max":
            res = roll.max()
        elif f == "first_value":
            res = roll.apply(lambda x: x.iloc[0], raw=False)
        elif f == "last_value":
            res = roll.apply(lambda x: x.iloc[-1], raw=False)
        else:
            raise RexCompileError(
                f"window function {f} with an explicit frame")
        # rolling output is ordered group-by-group exactly like the sorted
        # frame — realign positionally
        return pd.Series(res.to_numpy(), index=df.index)

    def _device_sort_keys(self, runtime, cols, n, spec, need_full=True):
        """Shared front half of the device window paths: the sort
        permutation over (partition, order) keys plus, in sorted order,
        per-row partition ids and (with need_full) partition+order peer
        ids — any u64 arrays whose adjacent values differ exactly at a
        boundary. The keys are resolved once (keys.key_record; dictionary
        ORDER BY keys through their rank column, PARTITION BY keys by raw
        code) and the records feed either engine:

        - _bucket_ids: sort_perm + keypack codes, for integer-kind keys
          that pack into one code;
        - _word_ids: the sort_word chain + boundary marks, for whatever
          the first declines (float keys, skew, more than 4 keys, key
          spaces above 2^62, tables wider than 16 columns) and for an
          explicit NULLS FIRST order key.

        DSX_DISABLE_WINWORDS=1 turns the second off (those shapes run on
        the host again); DSX_WIN_WORDS=1 sends every shape through it.
        Both are read per call. None → host fallback."""
        import os as _os
        from dask_sql_amd.physical.sort_words import window_order_mode
        words_on = _os.environ.get("DSX_DISABLE_WINWORDS", "0") != "1"
        force_words = words_on and \
            _os.environ.get("DSX_WIN_WORDS", "0") == "1"
        nfs = list(getattr(spec, "order_nf", [])) or \
            [None] * len(spec.order_idx)
        try_bucket = not force_words and not any(nf is True for nf in nfs)
        if not try_bucket and not words_on:
            return None
        # partition keys carry mode 0, which is the bucket route's;
        # plan_window_words gives them PARTITION_MODE itself. Order keys:
        # the host sorts them na_position="last" for BOTH directions
        # (_host_ordered) unless the query says NULLS FIRST, which only
        # the word route takes
        wanted = [(i, 0, False) for i in spec.part_idx] + \
            [(i, window_order_mode(desc, nf), True)
             for (i, desc), nf in zip(spec.order_idx, nfs)]
        work = list(cols)  # + rank columns of dictionary order keys
        recs = []
        for i, mode, rank in wanted:
            rec = keys.key_record(runtime, work, n, i, mode, rank)
            if rec is None or (rec[1] and not words_on):
                return None
            recs.append(rec)
        part, order = recs[:len(spec.part_idx)], recs[len(spec.part_idx):]
        want_fs = bool(order) and need_full
        if try_bucket and not any(rec[1] for rec in recs):
            out = self._bucket_ids(runtime, work, n, part, order, want_fs)
            if out is not None:
                return out
        if not words_on or not recs:
            return None
        return self._word_ids(runtime, work, n, part, order, want_fs)

    @staticmethod
    def _zero_ids(runtime, n):
        """Constant zero ids for "no partition key": an eval of literal 0
        over n rows."""
        from dask_sql_amd.physical.rex import OP_LIT_I64
        z = runtime.upload_column(np.zeros(1, dtype=np.int64))
        return runtime.eval(runtime.make_prog([(OP_LIT_I64, 0, 0)]), [z], n,
                            rt.I64, with_validity=False)

    def _word_ids(self, runtime, work, n, part, order, want_fs):
        """Word front half: plan_window_words cuts the (partition, order)
        key records into 64-bit words, keys.run_words sorts by them,
        window_mark_word ORs each word's boundary marks over the sorted
        sequence and window_seg_ids turns marks into ids — the partition
        words' marks give the partition ids, the order words' marks on top
        of them the peer ids. Each word brings only its own columns. None
        (→ host) when a word is refused (one integer key spanning more
        than 2^62)."""
        from dask_sql_amd.physical.sort_words import plan_window_words
        words = plan_window_words(part, order)
        perm = keys.run_words(runtime, words, work, n)
        if perm is None:
            return None

        def mark(side, marks):
            for w in words:
                if w.is_partition == side:
                    marks = runtime.window_mark_word(
                        [work[i] for i in w.cols], list(w.specs), n, perm,
                        marks)
                    if marks is None:
                        # validated exactly like the sort_word call above
                        raise rt.DsxError("window_mark_word refused a word "
                                          "that sort_word accepted")
            return marks

        marks = mark(True, None)
        ps = runtime.window_seg_ids(marks, n)[0] if part \
            else self._zero_ids(runtime, n)
        fs = ps
        if want_fs:
            # ORed into the same buffer: ps is already computed from it
            fs = runtime.window_seg_ids(mark(False, marks), n)[0]
        return perm, ps, fs

    def _bucket_ids(self, runtime, work, n, part, order, want_fs):
        """Bucket front half: sort_perm over the packed (partition, order)
        key records, keypack codes gathered into sorted order as the ids.
        None when the key space does not pack or sort_perm refuses."""
        recs = part + order
        perm = runtime.sort_perm(
            work, [keys.bucket_spec(rec) for rec in reversed(recs)], n)
        if perm is None:
            return None

        def packed(recs):
            if not recs:
                return self._zero_ids(runtime, n)
            return runtime.keypack(
                work, [(ki, mn, rng, nullable) for
                       (ki, _f, mn, rng, nullable, _m) in recs], n)[0]

        try:
            pcodes = packed(part)
            fcodes = packed(recs) if want_fs else pcodes
        except Exception:
            return None  # key space overflow etc → next route
        ps = runtime.gather(pcodes, perm.data, n)
        fs = runtime.gather(fcodes, perm.data, n) if want_fs else ps
        return perm, ps, fs

    def _device_ordered(self, runtime, cols, n, spec):
        """Device ordered window frames: sort permutation
        over (partition, order) keys → boundary starts → dsx_window_ordered
        (binary-search ranks / shifts; per-partition running scans with
        peer broadcast). Mirrors _host_ordered's pandas semantics exactly
        (na_position="last" on order keys, partitions keep NULL groups).
        Returns None on unsupported shapes → host fallback."""
        import os as _os
        if _os.environ.get("DSX_DISABLE_DEVWINDOW") or n == 0:
            return None
        if spec.func not in runtime.WIN_FUNCS:
            return None
        keys = self._device_sort_keys(runtime, cols, n, spec)
        if keys is None:
            return None
        perm, ps, fs = keys

        v_col = cols[spec.arg_idx] if spec.arg_idx is not None else None
        func = spec.func
        ranking = func in ("row_number", "rank", "dense_rank")
        if ranking:
            out_dtype, want_valid = rt.I64, False
            default_bits, has_def = 0, False
        elif func in ("lag", "lead", "first_value"):
            if v_col is None or getattr(v_col, "dictionary",
                                        None) is not None:
                return None  # dict value shift: host (string payload)
            out_dtype = v_col.dtype
            want_valid = True
            has_def = spec.default is not None and func != "first_value"
            default_bits = 0
            if has_def:
                d = spec.default
                if out_dtype in (rt.F64,):
                    default_bits = int(np.float64(d).view(np.int64))
                elif out_dtype == rt.F32:
                    default_bits = int(np.float32(d).view(np.int32))
                else:
                    default_bits = int(d)
        else:
            if func != "count" and v_col is None:
                return None
            if v_col is not None and getattr(v_col, "dictionary",
                                             None) is not None:
                return None
            # host emits int64 when the plan type is BIGINT and nothing is
            # NULL; float64 (+validity) otherwise (_host_ordered tail)
            is_big = spec.out_type is not None and                 spec.out_type.getSqlType() == "BIGINT"
            nonnull_v = v_col is None or not v_col.validity
            if func == "count":
                out_dtype, want_valid = rt.I64, False
            elif is_big and nonnull_v and func in ("sum", "min", "max"):
                out_dtype, want_valid = rt.I64, False
            else:
                out_dtype, want_valid = rt.F64, True
            default_bits, has_def = 0, False
        col = runtime.window_ordered(perm, n, ps, fs, func, v_col,
                                     spec.offset, default_bits, has_def,
                                     out_dtype, want_valid)
        col._keep_alive = (perm, ps, fs, v_col)
        return col

    def _device_rows(self, runtime, cols, n, spec):
        """Device explicit ROWS frames (dsx_window_rows): the sort front
        half of _device_ordered, then window_frames.lower_rows_frame picks
        the LDS tile pass or the per-partition scans. Reproduces
        _frame_apply: an empty frame is NULL for every function (COUNT
        too), FIRST/LAST return the boundary row as is. Returns None on
        unsupported shapes → host fallback."""
        import os as _os
        from dask_sql_amd.physical import window_frames as wf
        if _os.environ.get("DSX_DISABLE_DEVWINDOW") or n == 0:
            return None
        func = spec.func
        if func not in runtime.WIN_ROWS_FUNCS:
            return None
        lo_off, hi_off, strategy = wf.lower_rows_frame(func, spec.frame)
        if strategy == "host":
            return None
        v_col = cols[spec.arg_idx] if spec.arg_idx is not None else None
        if v_col is None and func != "count":
            return None
        if v_col is not None and getattr(v_col, "dictionary",
                                         None) is not None:
            return None  # string payload: host
        keys = self._device_sort_keys(runtime, cols, n, spec,
                                      need_full=False)
        if keys is None:
            return None
        perm, ps, _fs = keys
        is_big = spec.out_type is not None and \
            spec.out_type.getSqlType() == "BIGINT"
        kind, want_valid = wf.frame_out_dtype(
            func, lo_off, hi_off, is_big,
            v_col is not None and bool(v_col.validity))
        out_dtype = {"i64": rt.I64, "f64": rt.F64}.get(kind)
        if out_dtype is None:
            out_dtype = v_col.dtype
        col = runtime.window_rows(perm, n, ps, func, v_col, lo_off, hi_off,
                                  out_dtype, want_valid)
        col._keep_alive = (perm, ps, v_col)
        return col

    @staticmethod
    def _range_out(spec, v_col, lo, hi):
        """(kind, with_validity) of a RANGE-framed column, shared by the
        device and host routes so both produce the same dtype."""
        from dask_sql_amd.physical import window_range as wrg
        is_big = spec.out_type is not None and \
            spec.out_type.getSqlType() == "BIGINT"
        return wrg.range_out_dtype(
            spec.func, lo, hi, is_big,
            v_col is not None and bool(v_col.validity))

    def _device_range(self, runtime, cols, n, spec):
        """Device RANGE frames with value offsets (dsx_window_range): the
        sort front half with peer ids, then per-row frame bounds by binary
        search over the sorted order key, the per-partition scans and, for
        a MIN/MAX bounded on both sides, the sparse table. Returns None →
        window_range.range_frames_host: DSX_DISABLE_DEVWINDOW, an empty
        table, a dictionary-encoded value column, a key the device does not
        sort, OVER () without any key, or a table above
        DSX_WIN_RANGE_RMQ_MAX_BYTES."""
        import os as _os
        from dask_sql_amd.physical import window_range as wrg
        if _os.environ.get("DSX_DISABLE_DEVWINDOW") or n == 0:
            return None
        func = spec.func
        if func not in runtime.WIN_ROWS_FUNCS:
            return None
        v_col = cols[spec.arg_idx] if spec.arg_idx is not None else None
        if v_col is None and func != "count":
            return None
        if v_col is not None and getattr(v_col, "dictionary",
                                         None) is not None:
            return None  # string payload: host
        lo, hi = wrg.frame_bounds(spec.frame)
        k_col, desc = None, False
        if wrg.OFFSET in (lo.kind, hi.kind):
            ki, desc = spec.order_idx[0]
            k_col = cols[ki]
            if k_col.dtype not in (rt.I64, rt.I32, rt.I8, rt.F64, rt.F32) \
                    or getattr(k_col, "dictionary", None) is not None:
                return None
        if wrg.needs_rmq(func, lo, hi) \
                and wrg.rmq_table_bytes(n) > wrg.rmq_max_bytes():
            # the library would answer -7; decline before the sort
            return None
        sort = self._device_sort_keys(runtime, cols, n, spec, need_full=True)
        if sort is None:
            return None
        perm, ps, fs = sort
        kind, want_valid = self._range_out(spec, v_col, lo, hi)
        out_dtype = {"i64": rt.I64, "f64": rt.F64}.get(kind)
        if out_dtype is None:
            out_dtype = v_col.dtype
        col = runtime.window_range(perm, n, ps, fs, func, v_col, k_col, desc,
                                   lo, hi, out_dtype, want_valid)
        if col is None:
            return None
        col._keep_alive = (perm, ps, fs, v_col, k_col)
        return col

    def _host_range(self, runtime, cols, n, spec):
        """RANGE frames on the host: download the key and value columns
        like _host_ordered and run the numpy model of the same semantics
        (window_range.range_frames_host)."""
        from dask_sql_amd.physical import window_range as wrg

        def key_of(i):
            arr, valid = cols[i].to_numpy()
            dic = getattr(cols[i], "dictionary", None)
            if dic is not None:
                # dictionary codes → ranks in string order
                order = np.argsort(np.asarray(list(dic), dtype=object),
                                   kind="mergesort")
                rank = np.empty(len(order), dtype=np.int64)
                rank[order] = np.arange(len(order))
                ok = valid if valid is not None else \
                    np.ones(len(arr), dtype=bool)
                arr = np.where(ok, rank[np.where(ok, arr, 0)], 0)
            return arr, valid

        func = spec.func
        if func not in wrg.RANGE_FUNCS:
            raise RexCompileError(
                f"window function {func} with a RANGE frame")
        v_col = cols[spec.arg_idx] if spec.arg_idx is not None else None
        if v_col is None and func != "count":
            raise RexCompileError(f"{func} with a RANGE frame needs an "
                                  "operand")
        dic = getattr(v_col, "dictionary", None) if v_col is not None \
            else None
        if dic is not None and func not in wrg.RANGE_POSITIONAL:
            raise RexCompileError(
                f"{func} over a string column with a RANGE frame")
        lo, hi = wrg.frame_bounds(spec.frame)
        pid = wrg.dense_ids([key_of(i) for i in spec.part_idx]) \
            if spec.part_idx else np.zeros(n, dtype=np.int64)
        nfs = list(getattr(spec, "order_nf", [])) or \
            [None] * len(spec.order_idx)
        order = [key_of(i) + (bool(desc), nf is True)
                 for (i, desc), nf in zip(spec.order_idx, nfs)]
        value, value_valid = v_col.to_numpy() if v_col is not None \
            else (None, None)
        kind, _want_valid = self._range_out(spec, v_col, lo, hi)
        out, ok = wrg.range_frames_host(func, pid, order, value, value_valid,
                                        lo, hi, kind)
        col = runtime.upload_column(
            out, validity=ok,
            dtype=v_col.dtype if kind == "value" else None)
        if dic is not None:
            col.dictionary = dic
        return col

    def _device_agg(self, runtime, cols, n, spec):
        """groupby → per-group value → hash join-back → row scatter."""
        keyspecs = []
        for gi in spec.part_idx:
            mn, rng = keys.key_range(runtime, cols[gi])
            keyspecs.append((gi, mn, rng, bool(cols[gi].validity)))
        arg = InputRef(spec.arg_idx, None) if spec.arg_idx is not None \
            else None
        speclist, fin = DaskAggregatePlugin()._agg_spec_expr(
            spec.func, arg, cols, _dicts_of(cols))
        specs = [(op, runtime.make_prog(p)) for op, p in speclist]
        oc, ov, on, G = runtime.hash_groupby(cols, n, keyspecs, None, specs)

        class _H:
            def __init__(s, ptrs):
                s.ptrs = ptrs

            def __del__(s):
                for p in s.ptrs:
                    try:
                        runtime._free(p)
                    except Exception:
                        pass

        h = _H([oc, ov, on])
        from dask_sql_amd.physical.rex import (OP_DIV_F64, OP_GT_I64,
                                               OP_I64_TO_F64, OP_LIT_I64,
                                               OP_LIT_NULL, OP_SELECT)
        val_col = rt.DeviceColumn(runtime, ov, None, G,
                                  rt.F64 if fin in ("avg", "sum_f", "min_f",
                                                    "max_f") else rt.I64,
                                  owner=False, keep_alive=h)
        cnt_col = rt.DeviceColumn(runtime, on, None, G, rt.I64, owner=False,
                                  keep_alive=h)
        if fin == "count":
            gval = cnt_col
        elif fin == "avg":
            prog = [(OP_COL, 1, 0), (OP_LIT_I64, 0, 0), (OP_GT_I64, 0, 0),
                    (OP_COL, 0, 0), (OP_COL, 1, 0), (OP_I64_TO_F64, 0, 0),
                    (OP_DIV_F64, 0, 0), (OP_LIT_NULL, 0, 0),
                    (OP_SELECT, 0, 0)]
            gval = runtime.eval(runtime.make_prog(prog), [val_col, cnt_col],
                                G, rt.F64)
        else:
            prog = [(OP_COL, 1, 0), (OP_LIT_I64, 0, 0), (OP_GT_I64, 0, 0),
                    (OP_COL, 0, 0), (OP_LIT_NULL, 0, 0), (OP_SELECT, 0, 0)]
            gval = runtime.eval(runtime.make_prog(prog), [val_col, cnt_col],
                                G, val_col.dtype)
        # join-back: every row's partition code is in the group table
        bcodes = rt.DeviceColumn(runtime, oc, None, G, rt.I64, owner=False,
                                 keep_alive=h)
        pcodes, space = runtime.keypack(cols, keyspecs, n)
        table = runtime.hash_build(bcodes, None, code_max=space - 1)
        try:
            p_ptr, b_ptr, count = runtime.hash_probe(table, pcodes,
                                                     rt.JOIN_INNER, None)
            p_sel = runtime.wrap_sel(p_ptr, count)
            b_sel = runtime.wrap_sel(b_ptr, count)
            assert count == n, (count, n)
            pair_val = runtime.gather(gval, b_sel.data, count,
                                      bool(gval.validity))
            out = runtime.scatter_rows(pair_val, p_sel.data, count, n,
                                       with_validity=bool(pair_val.validity))
        finally:
            runtime.hash_table_free(table)
        return out

    def _host_ordered(self, runtime, cols, n, spec):
        import pandas as pd

        def np_col(i):
            arr, valid = cols[i].to_numpy()
            if valid is not None and not valid.all():
                arr = arr.astype(np.float64)
                arr[~valid] = np.nan
            return arr

        df = pd.DataFrame({f"p{j}": np_col(i)
                           for j, i in enumerate(spec.part_idx)})
        pnames = list(df.columns)
        onames = []
        asc = []
        for j, (i, desc) in enumerate(spec.order_idx):
            df[f"o{j}"] = np_col(i)
            onames.append(f"o{j}")
            asc.append(not desc)
        if spec.arg_idx is not None:
            df["v"] = np_col(spec.arg_idx)
        if not pnames:
            df["p0"] = 0
            pnames = ["p0"]
        if onames:
            nfs = list(getattr(spec, "order_nf", [])) or [None] * len(
                onames)
            if any(nf is True for nf in nfs):
                # mixed per-key NULL placement: successive stable sorts,
                # last key first
                for name_, a_, nf in reversed(list(zip(onames, asc, nfs))):
                    df = df.sort_values(
                        name_, ascending=a_, kind="mergesort",
                        na_position="first" if nf else "last")
            else:
                df = df.sort_values(onames, ascending=asc,
                                    na_position="last", kind="mergesort")
        df = df.sort_values(pnames, na_position="last", kind="mergesort")
        grp = df.groupby(pnames, dropna=False, sort=False)
        f = spec.func
        if getattr(spec, "frame", None) is not None:
            res = self._frame_apply(df, grp, pnames, spec)
        elif f == "row_number":
            res = grp.cumcount() + 1
        elif f == "last_value":
            # default frame: ordered → the current row (reference expanding
            # tail); unordered → whole partition → partition tail
            res = df["v"] if onames else grp["v"].transform("last")
        elif f == "first_value":
            # default frame starts at the partition head (test_over.py:90)
            res = grp["v"].transform("first")
        elif f in ("lag", "lead"):
            # row-based shift within the partition; boundary rows get the
            # default (NULL unless given) — reference window.py lag/lead
            off = spec.offset if f == "lag" else -spec.offset
            res = grp["v"].shift(off)
            if spec.default is not None:
                pos = grp.cumcount()
                size = grp["v"].transform("size")
                bm = pos < spec.offset if f == "lag" \
                    else pos >= size - spec.offset
                res = res.where(~bm, spec.default)
        elif f in ("rank", "dense_rank"):
            rn = grp.cumcount() + 1
            df["_rn"] = rn
            tie = df.groupby(pnames + onames, dropna=False, sort=False)
            if f == "rank":
                res = tie["_rn"].transform("first")
            else:
                tid = tie.ngroup()
                df["_tid"] = tid
                res = tid - grp["_tid"].transform("first") + 1
        elif not onames and f in ("sum", "count", "avg", "min", "max"):
            # no ORDER BY: the default frame is the WHOLE partition
            # (reference window.py:280-300 unbounded..unbounded)
            if f == "count" and spec.arg_idx is None:
                res = grp["p0" if "p0" in df.columns else pnames[0]] \
                    .transform("size")
            elif f == "count":
                res = grp["v"].transform("count")
            elif f == "sum":
                # SUM over a partition with no non-NULL value is NULL
                res = grp["v"].transform("sum", min_count=1)
            else:
                res = grp["v"].transform(
                    {"avg": "mean", "min": "min", "max": "max"}[f])
        else:
            # running aggregates, default RANGE UNBOUNDED..CURRENT frame:
            # cumulative then broadcast the tie-group's last value (peers)
            if f == "count" and spec.arg_idx is None:
                cum = grp.cumcount() + 1
            elif f == "count":
                df["_nn"] = df["v"].notna().astype(np.int64)
                cum = grp["_nn"].cumsum()
            elif f == "sum":
                cum = grp["v"].cumsum()
                cum = cum.groupby(
                    [df[c] for c in pnames], dropna=False).ffill()
            elif f == "min":
                cum = grp["v"].cummin()
                cum = cum.groupby(
                    [df[c] for c in pnames], dropna=False).ffill()
            elif f == "max":
                cum = grp["v"].cummax()
                cum = cum.groupby(
                    [df[c] for c in pnames], dropna=False).ffill()
            elif f == "avg":
                df["_nn"] = df["v"].notna().astype(np.int64)
                s = grp["v"].cumsum().groupby(
                    [df[c] for c in pnames], dropna=False).ffill()
                c = grp["_nn"].cumsum()
                cum = s / c.replace(0, np.nan)
            else:
                raise RexCompileError(f"window function {f}")
            if onames:
                df["_cum"] = cum
                res = df.groupby(pnames + onames, dropna=False,
                                 sort=False)["_cum"].transform("last")
            else:
                res = cum
        vals = np.asarray(res, dtype=np.float64)
        out = np.empty(n, dtype=np.float64)
        out[df.index.to_numpy()] = vals
        nanmask = np.isnan(out)
        if not nanmask.any() and spec.func in ("row_number", "rank",
                                               "dense_rank", "count") \
                or (not nanmask.any()
                    and spec.out_type.getSqlType() == "BIGINT"):
            return runtime.upload_column(out.astype(np.int64))
        return runtime.upload_column(
            out, validity=(~nanmask).astype(np.uint8)
            if nanmask.any() else None)


class DaskUnionPlugin(BaseRelPlugin):
    """Positional UNION ALL: device concatenation of the branch columns
    (reference Union rel → dd.concat of the branch frames). Dict string
    columns merge dictionaries (rhs codes remapped on device); mixed
    numeric positions promote to f64."""

    class_name = "Union"

    def convert(self, rel, context):
        runtime = context._get_runtime()
        dcs = self.assert_inputs(rel, 2, context)
        fields = rel.getRowType().getFieldList()
        per_input = []
        for dc in dcs:
            cc = dc.column_container
            per_input.append([dc.table.col(cc.get_backend_by_frontend_name(f))
                              for f in cc.columns])
        n_total = sum(dc.table.num_rows for dc in dcs)
        out_cols = {}
        order_names = []
        for i, f in enumerate(fields):
            col = self._concat(runtime, [cols[i] for cols in per_input])
            bname = f"u{i}__{f.getName()}"
            out_cols[bname] = col
            order_names.append((f.getName(), bname))
        cc = ColumnContainer([nm for nm, _ in order_names],
                             dict(order_names))
        cc = self.fix_column_to_row_type(cc, rel.getRowType())
        return DataContainer(DeviceTable(out_cols, num_rows=n_total), cc)

    def _concat(self, runtime, cols):
        dicts = [getattr(c, "dictionary", None) for c in cols]
        if any(d is not None for d in dicts):
            if not all(d is not None for d in dicts):
                raise RexCompileError(
                    "UNION position mixes string and non-string")
            base = list(dicts[0])
            index = {s: j for j, s in enumerate(base)}
            parts = [cols[0]]
            for c, d in zip(cols[1:], dicts[1:]):
                if d is dicts[0] or list(d) == base[:len(d)]:
                    parts.append(c)
                    continue
                m = []
                for s in d:
                    if s is not None and s not in index:
                        index[s] = len(base)
                        base.append(s)
                    m.append(index.get(s, 0))
                map_col = runtime.upload_column(np.array(m, dtype=np.int32),
                                                dtype=rt.I32)
                g = runtime.gather(map_col, _codes_i32(runtime, c).data,
                                   c.len)
                parts.append(rt.DeviceColumn(runtime, g.data, c.validity,
                                             c.len, rt.I32, owner=False,
                                             keep_alive=(g, c, map_col)))
            code_dt = rt.I32
            if any(p.dtype != rt.I32 for p in parts):
                # a branch that went through a groupby (UNION's Distinct)
                # carries wider codes: widen every part the same way
                code_dt = rt.I64
                prog = runtime.make_prog([(OP_COL, 0, 0)])
                parts = [p if p.dtype == rt.I64 else runtime.eval(
                    prog, [p], p.len, rt.I64,
                    with_validity=bool(p.validity)) for p in parts]
            out = runtime.concat_columns(parts, code_dt)
            out.dictionary = base
            return out
        target = cols[0].dtype
        if any(c.dtype != target for c in cols):
            target = rt.F64 if any(c.dtype in (rt.F64, rt.F32)
                                   for c in cols) else rt.I64
        parts = []
        for c in cols:
            if c.dtype == target:
                parts.append(c)
            else:
                prog = [(OP_COL, 0, 0)]
                if target == rt.F64 and c.dtype not in (rt.F64, rt.F32):
                    prog.append((50, 0, 0))  # I64_TO_F64
                parts.append(runtime.eval(runtime.make_prog(prog), [c],
                                          c.len, target,
                                          with_validity=bool(c.validity)))
        return runtime.concat_columns(parts, target)


class DaskValuesPlugin(BaseRelPlugin):
    """One-row empty relation for FROM-less SELECTs (SELECT 1 + 1)."""

    class_name = "Values"

    def convert(self, rel, context):
        context._get_runtime()  # GPU required like everything else
        return DataContainer(DeviceTable({}, num_rows=1), ColumnContainer([]))


def register_defaults():
    for cls in (DaskTableScanPlugin, DaskFilterPlugin, DaskProjectPlugin,
                DaskJoinPlugin, DaskAggregatePlugin, DaskSortPlugin,
                DaskLimitPlugin, DaskWindowPlugin, DaskUnionPlugin,
                DaskValuesPlugin):
        RelConverter.add_plugin_class(cls, replace=False)
