"""The join plugin: gathers what the plan and the inputs say about a join
(join_plan.JoinFacts), asks join_plan.route for the one decision, and runs the
executor it names. Two declines depend on the device and stay run-time
fallbacks here: dsx_radix_join not applicable (the route's fallback runs) and
dsx_filter_probe_cols finding duplicate build keys (the probe side runs its
WHERE and probes the same table the two-pass way). The aggregate's group-join
uses the public surface: prepare, route, settle, fused_setup, build_table,
key_columns, key_dtype and source_col."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from dask_sql_amd import runtime as rt
from dask_sql_amd.datacontainer import (ColumnContainer, DataContainer,
                                        DeferredFilter, DeviceTable,
                                        pending_filter)
from dask_sql_amd.physical import join_plan as jp
from dask_sql_amd.physical import keys
from dask_sql_amd.physical.convert import BaseRelPlugin
from dask_sql_amd.physical.rex import (OP_AND, OP_COL, OP_IS_NOT_NULL,
                                       RexCompileError, compile_expr,
                                       scalar_literal)
from dask_sql_amd.planner.plan import Call
from dask_sql_amd.planner.prune import _expr_refs, _remap

_INT_KINDS = keys.INT_KINDS
_dicts_of = keys.dicts_of


# What the plan says about a join, over its two converted inputs. join_type:
# lower-case (inner / left / right / outer / leftanti); lhs_on / rhs_on: equi
# keys, side-local column positions; residual: the rest of the condition, over
# the combined row; combined: (side, frontend name) per column of the joined
# row; out_idx: the columns of it that the plan consumes; mat_idx: those, once
PreparedJoin = namedtuple(
    "PreparedJoin", "join dc_lhs dc_rhs cc_lhs cc_rhs n_lhs_cols join_type "
    "lhs_on rhs_on residual combined out_idx mat_idx null_eq")
# Sides, key ranges and column lists of the hash paths' entries. pending /
# pending_b: the filter-probe / filter-build side. dc_lhs / dc_rhs: the inputs,
# a side that stays pending as its UNFILTERED base rows; probe_kdc / build_kdc:
# the same with a dictionary key of the rhs remapped into the lhs dictionary.
# fp_cols / fp_keys (pending probe side only): its program plus key columns in
# ONE list and the key specs indexing it; fb_cols / fb_keys: the same for the
# build side, with the program columns of a pending build side or none
FusedSetup = namedtuple(
    "FusedSetup", "pending pending_b dc_lhs dc_rhs swap ktype ranges "
    "probe_kdc build_kdc probe_on build_on fp_cols fp_keys fb_cols fb_keys "
    "fb_space")


def source_col(J, i, dc_lhs=None, dc_rhs=None):
    """The input column behind J.combined[i], of the given containers."""
    side, frontend = J.combined[i]
    if side == "l":
        dc, cc = J.dc_lhs if dc_lhs is None else dc_lhs, J.cc_lhs
    else:
        dc, cc = J.dc_rhs if dc_rhs is None else dc_rhs, J.cc_rhs
    return dc.table.col(cc.get_backend_by_frontend_name(frontend))


def tag_output(col, src):
    """An output column of rows of `src`: its dictionary and its statistics."""
    if getattr(src, "dictionary", None) is not None:
        col.dictionary = src.dictionary
    col._stats_src = src
    return col


def fold_residual(residual, index_map):
    """The residual conjuncts as one expression over the columns that
    index_map (joined-row column → position) lists."""
    cond = residual[0]
    for r in residual[1:]:
        cond = Call("AND", [cond, r])
    return _remap(cond, index_map)


def dict_rewrites(lkeys, rkeys):
    """Per key pair: would the string-key reconciliation rewrite the rhs key?
    Yes when both are dictionaries, neither the same object nor equal lists.
    Pure; a string column paired with a non-string one is an error."""
    out = []
    for lc, rc in zip(lkeys, rkeys):
        dl = getattr(lc, "dictionary", None)
        dr = getattr(rc, "dictionary", None)
        if (dl is None) != (dr is None):
            raise RexCompileError(
                "join key pairs a string column with a non-string column")
        out.append(dl is not None and dl is not dr and list(dl) != list(dr))
    return out


def _n_cols(prog_cols, key_cols):
    """Length of prog_cols with the key columns added by identity; a None
    key stands for a column made for this join (a remapped key)."""
    ids = {id(c) for c in prog_cols}
    return len(ids) + key_cols.count(None) + len(
        {id(c) for c in key_cols if c is not None} - ids)


class DaskJoinPlugin(BaseRelPlugin):
    """reference rel/logical/join.py:23-322.

    Equi/residual split mirrors _split_join_condition (:250-322); NULL-key
    drop (:202-213) is the kernels' validity skip; dd.merge (:241-246)
    becomes CAS-claim hash build + probe-compaction (k_hash_build/probe);
    LEFTSEMI falls back to INNER like the reference CPU path (:78-79);
    residual applied via filter_or_scalar (:169-181); FULL OUTER composed
    from LEFT + unmatched-build sweep, NaN-filled (test_join.py:55-65)."""

    class_name = "Join"

    JOIN_TYPE_MAPPING = {
        "INNER": "inner", "LEFT": "left", "RIGHT": "right", "FULL": "outer",
        "LEFTSEMI": "inner",  # reference join.py:78-79 (CPU)
        "LEFTANTI": "leftanti", "CROSS": "cross",
    }

    def convert(self, rel, context, inputs=None, table=None):
        """inputs: the converted inputs or the prepared join, when the
        aggregate's group-join attempt made them already; table: the hash
        table it built over this join's build side (build_table with the key
        filter), for the fused filter-probe join to use and free."""
        runtime = context._get_runtime()
        J = inputs if isinstance(inputs, PreparedJoin) else self.prepare(
            rel, *(inputs or self.assert_inputs(rel, 2, context)))
        join_type, residual = J.join_type, J.residual

        if (join_type == "leftanti" and getattr(J.join, "null_aware", False)
                and J.rhs_on):
            # NOT IN three-valued logic: any NULL in the subquery output
            # makes `x NOT IN (...)` non-TRUE for every row → empty result
            rcols0 = J.dc_rhs.backend_cols()
            for ri in J.rhs_on:
                col = rcols0[ri]
                if col.validity:
                    _, _, nn = keys.minmax_cached(runtime, col)
                    if nn < J.dc_rhs.table.num_rows:
                        return self._empty_output(rel, runtime, J.dc_lhs)

        R = self.settle(J, self.route(J))
        if table is not None and not (R.path == "fused" and R.fprobe):
            # a group-join attempt built it for this very route
            runtime.hash_table_free(table)
            raise AssertionError(R)
        mat_idx = J.mat_idx
        gathered = pairs = None
        if R.path in ("radix", "fused"):
            S = self.fused_setup(runtime, J, R)
            if R.path == "radix":
                gathered = self._run_radix(runtime, J, S)
            if gathered is None and R.fallback != "pairs":
                gathered = self._run_fused(runtime, J, R, S, table)
        else:
            if R.path == "anti_residual":
                # ANTI with extra condition: keep lhs rows with NO rhs match
                # satisfying key AND residual (join.py:169-181 composed with
                # the anti semantics of :78-90)
                pairs = self._anti_residual(runtime, J)
                residual = []
            res_refs = set()
            for r in residual:
                _expr_refs(r, res_refs)
            mat_idx = sorted(set(J.out_idx) | res_refs)
        if gathered is None:
            gathered = self._run_pairs(runtime, J, R, mat_idx, pairs)
        gathered, n_out = gathered

        # residual filter (join.py:169-181) over the combined row, with
        # InputRefs densified to the materialized set
        if residual:
            cond = fold_residual(
                residual, {i: pos for pos, i in enumerate(mat_idx)})
            cols_list = [gathered[i] for i in mat_idx]
            s = scalar_literal(cond)
            if s is not None:
                if not s:
                    empty = runtime.empty_column(0, rt.I32)
                    gathered = {i: runtime.gather(gathered[i], empty.data, 0)
                                for i in mat_idx}
                    n_out = 0
            else:
                prog, _ = compile_expr(cond, cols_list, _dicts_of(cols_list))
                sel_ptr, n_out = runtime.filter(runtime.make_prog(prog),
                                                cols_list, n_out)
                sel = runtime.wrap_sel(sel_ptr, n_out)
                gathered = {
                    i: tag_output(runtime.gather(
                        gathered[i], sel.data, n_out,
                        bool(gathered[i].validity)), gathered[i])
                    for i in J.out_idx}

        field_names = [str(f) for f in rel.getRowType().getFieldNames()]
        assert len(field_names) == len(J.out_idx), (field_names, J.out_idx)
        out_cols = {f"j{i}__{name}": gathered[i]
                    for name, i in zip(field_names, J.out_idx)}
        cc = ColumnContainer(field_names, dict(zip(field_names, out_cols)))
        return DataContainer(DeviceTable(out_cols, num_rows=n_out), cc)

    # -- the surface the aggregate's group-join shares -----------------------
    def prepare(self, rel, dc_lhs, dc_rhs) -> PreparedJoin:
        """Unique names, join type, split condition, columns to materialize."""
        join = rel.join()
        cc_lhs = dc_lhs.column_container.make_unique("lhs")
        cc_rhs = dc_rhs.column_container.make_unique("rhs")
        dc_lhs = dc_lhs.with_columns(cc_lhs)
        dc_rhs = dc_rhs.with_columns(cc_rhs)
        n_lhs_cols = len(cc_lhs.columns)
        join_type = self.JOIN_TYPE_MAPPING[str(join.getJoinType())]
        lhs_on, rhs_on, residual = [], [], []
        if join.getCondition() is not None:
            lhs_on, rhs_on, residual = self._split_join_condition(
                join.getCondition(), n_lhs_cols)
        # materialize only columns the plan consumes (output_indices from the
        # pruning pass) plus residual-referenced temporaries
        combined = [("l", f) for f in cc_lhs.columns]
        if join_type != "leftanti":
            combined += [("r", f) for f in cc_rhs.columns]
        out_idx = getattr(join, "output_indices", None)
        if out_idx is None:
            # unpruned SEMI join (e.g. below a UNION): lhs columns only
            out_idx = list(range(
                n_lhs_cols if str(join.getJoinType()) == "LEFTSEMI"
                else len(combined)))
        return PreparedJoin(
            join, dc_lhs, dc_rhs, cc_lhs, cc_rhs, n_lhs_cols, join_type,
            lhs_on, rhs_on, residual, combined, out_idx,
            sorted(set(out_idx)),
            bool(getattr(join, "null_equal", False)))

    @staticmethod
    def key_columns(J):
        """([lhs key columns], [rhs key columns]); a DeferredFilter's are its
        base table's, which have the dtypes and dictionaries of its rows."""
        return [[(dc.base if isinstance(dc, DeferredFilter) else dc).table.col(
            dc.column_container.get_backend_by_frontend_index(i)) for i in on]
            for dc, on in ((J.dc_lhs, J.lhs_on), (J.dc_rhs, J.rhs_on))]

    def route(self, J, group_join=False, ran=()) -> jp.JoinRoute:
        """join_plan.route over this join's facts; no device work. Its path
        is None while a side has to run its WHERE first (settle). ran: the
        sides whose WHERE has run since the first answer."""
        kcols = self.key_columns(J)
        rew = dict_rewrites(*kcols)
        sides = []
        for s, dc, kc in (("l", J.dc_lhs, kcols[0]), ("r", J.dc_rhs, [
                None if w else c for c, w in zip(kcols[1], rew)])):
            pend = s in ran or pending_filter(dc)
            sides.append(jp.Side(
                dc.max_rows if pend else dc.table.num_rows,
                isinstance(dc, DeferredFilter), pend,
                dc.table.num_rows if s in ran else None,
                _n_cols(dc.prog_cols, kc) if pend else 0))
        return jp.route(jp.JoinFacts(
            J.join_type, tuple((lc.dtype, rc.dtype, w)
                               for lc, rc, w in zip(*kcols, rew)),
            *sides, bool(J.residual),
            J.null_eq, bool(getattr(J.join, "null_aware", False)),
            len(J.mat_idx)), jp.knobs(), group_join)

    def settle(self, J, route, group_join=False) -> jp.JoinRoute:
        """The final route: runs the WHEREs `route` wants first, asks again."""
        if route.path is not None:
            return route
        for s in route.materialize:
            (J.dc_lhs if s == "l" else J.dc_rhs).table  # runs the filter
        final = self.route(J, group_join, route.materialize)
        assert (final.fprobe, final.fbuild) == (route.fprobe, route.fbuild)
        return final

    def fused_setup(self, runtime, J, route) -> FusedSetup:
        """Sides, key ranges and the entries' column lists of a radix or
        fused route (integer-kind keys). Applies the dictionary remap over the
        rows the route uses: a pending side's are its unfiltered base rows."""
        kept = (route.fprobe, route.fbuild)
        dcs = {"l": J.dc_lhs, "r": J.dc_rhs}
        pending, pending_b = dcs.get(kept[0]), dcs.get(kept[1])
        dc_lhs = J.dc_lhs.unfiltered() if "l" in kept else J.dc_lhs
        dc_rhs = J.dc_rhs.unfiltered() if "r" in kept else J.dc_rhs
        lhs_on, rhs_on = J.lhs_on, J.rhs_on
        def key_cols(dc, on):  # position → column, the key columns alone
            return {i: dc.table.col(
                dc.column_container.get_backend_by_frontend_index(i)) for i in on}
        lcols = key_cols(dc_lhs, lhs_on)
        kdc_rhs, krcols = self._reconcile_dict_keys(
            runtime, lcols, dc_rhs, key_cols(dc_rhs, rhs_on), lhs_on, rhs_on)
        ranges = [keys.joint_range(runtime, lcols[li], krcols[ri])
                  for li, ri in zip(lhs_on, rhs_on)]
        if route.swap:
            probe_kdc, build_kdc, pk, bk = kdc_rhs, dc_lhs, krcols, lcols
            probe_on, build_on = rhs_on, lhs_on
        else:
            probe_kdc, build_kdc, pk, bk = dc_lhs, kdc_rhs, lcols, krcols
            probe_on, build_on = lhs_on, rhs_on

        def with_keys(cols, kcols, on):
            specs = []
            for i, (mn, rng) in zip(on, ranges):
                ci = next((k for k, c in enumerate(cols) if c is kcols[i]),
                          None)
                if ci is None:
                    cols.append(kcols[i])
                    ci = len(cols) - 1
                specs.append((ci, mn, rng, False))
            return cols, specs

        fp_cols = fp_keys = None
        if pending is not None:
            fp_cols, fp_keys = with_keys(list(pending.prog_cols), pk,
                                         probe_on)
        fb_cols, fb_keys = with_keys(
            list(pending_b.prog_cols) if pending_b is not None else [], bk,
            build_on)
        space = 1
        for _, rng in ranges:
            space *= rng
        return FusedSetup(pending, pending_b, dc_lhs, dc_rhs, route.swap,
                          route.ktype, ranges, probe_kdc, build_kdc, probe_on,
                          build_on, fp_cols, fp_keys, fb_cols, fb_keys, space)

    def build_table(self, runtime, S, route, key_filter):
        """The hash table over S's build side: straight from its columns
        (dsx_hash_build_cols, a pending build side's WHERE inside) where the
        route says so, else keypack + hash_build. key_filter: also build the
        key-membership filter (for the fused filter-probe and group-join)."""
        if route.build_from_cols:
            return runtime.hash_build_cols(
                runtime.make_prog(S.pending_b.prog)
                if S.pending_b is not None else None,
                S.fb_cols, S.fb_keys, S.build_kdc.table.num_rows,
                code_max=S.fb_space - 1, key_filter=key_filter)
        assert S.pending_b is None, route
        bcodes, bval, bkeep, space = self._key_codes(
            runtime, S.build_kdc, S.build_on, S.ranges)
        return runtime.hash_build(bcodes, bval, code_max=space - 1,
                                  key_filter=key_filter)

    @staticmethod
    def key_dtype(col, side):
        """A key's dtype for group_join.verdict: strings never compare equal
        across sides (per-side codes)."""
        if getattr(col, "dictionary", None) is not None:
            return ("dict", side)
        return col.dtype

    # -- helpers ------------------------------------------------------------
    def _empty_output(self, rel, runtime, dc_lhs):
        field_names = [str(f) for f in rel.getRowType().getFieldNames()]
        out_idx = getattr(rel.join(), "output_indices", None)
        if out_idx is None:
            out_idx = list(range(len(field_names)))
        empty = runtime.empty_column(0, rt.I32)
        out_cols = {}
        lcols = dc_lhs.backend_cols()
        for name, oi in zip(field_names, out_idx):
            src = lcols[oi] if oi < len(lcols) else lcols[0]
            g = runtime.gather(src, empty.data, 0)
            if getattr(src, "dictionary", None) is not None:
                g.dictionary = src.dictionary
            out_cols[f"j{oi}__{name}"] = g
        cc = ColumnContainer(field_names, dict(zip(field_names, out_cols)))
        return DataContainer(DeviceTable(out_cols, num_rows=0), cc)

    def _run_pairs(self, runtime, J, route, mat_idx, pairs=None):
        """PAIR / CROSS path: selection vectors, then one gather per
        materialized column."""
        if pairs is None and route.path == "cross":
            pairs = self._cross_join(runtime, J.dc_lhs, J.dc_rhs)
        elif pairs is None:
            pairs = self._equi_join(runtime, J.dc_lhs, J.dc_rhs, J.lhs_on,
                                    J.rhs_on, J.join_type, J.null_eq)
        (probe_sel, build_sel), n_out = pairs
        force = {"l": J.join_type in ("outer", "right"),
                 "r": J.join_type in ("left", "outer")}
        sel = {"l": probe_sel, "r": build_sel}
        gathered = {}
        for i in mat_idx:
            side = J.combined[i][0]
            col = source_col(J, i)
            gathered[i] = tag_output(
                runtime.gather(col, sel[side].data, n_out, force[side]), col)
        return gathered, n_out

    def _anti_residual(self, runtime, J):
        """LEFT ANTI with a residual: inner pairs, residual filter on them,
        then the host complement of the surviving probe ids (a rare shape)."""
        (pi, bi), n_i = self._equi_join(runtime, J.dc_lhs, J.dc_rhs, J.lhs_on,
                                        J.rhs_on, "inner")
        n_l = J.dc_lhs.table.num_rows
        matched = np.empty(0, dtype=np.uint32)
        if n_i:
            refs = set()
            for r in J.residual:
                _expr_refs(r, refs)
            refs = sorted(refs)
            cols_list = []
            for i in refs:
                # the residual sees lhs ++ rhs, an ANTI join's row only lhs
                dc, sel, k = (J.dc_lhs, pi, i) if i < J.n_lhs_cols \
                    else (J.dc_rhs, bi, i - J.n_lhs_cols)
                col = dc.table.col(
                    dc.column_container.get_backend_by_frontend_index(k))
                cols_list.append(tag_output(
                    runtime.gather(col, sel.data, n_i), col))
            cond = fold_residual(J.residual,
                                 {i: pos for pos, i in enumerate(refs)})
            s = scalar_literal(cond)
            if s is None:
                prog, _ = compile_expr(cond, cols_list, _dicts_of(cols_list))
                sel_ptr, cnt = runtime.filter(runtime.make_prog(prog),
                                              cols_list, n_i)
                surv = runtime.wrap_sel(sel_ptr, cnt)
                if cnt:
                    pid = runtime.gather(pi, surv.data, cnt)
                    matched = np.empty(cnt, dtype=np.uint32)
                    runtime._download(pid.data, matched)
            elif s:
                matched = np.empty(n_i, dtype=np.uint32)
                runtime._download(pi.data, matched)
        mask = np.ones(n_l, dtype=bool)
        if len(matched):
            mask[matched.astype(np.int64)] = False
        anti = np.flatnonzero(mask).astype(np.uint32)
        sel = runtime.upload_column(anti, dtype=rt.I32)
        return (sel, sel), len(anti)

    def _reconcile_dict_keys(self, runtime, lcols, dc_rhs, rcols, lhs_on,
                             rhs_on):
        """String join keys: the reference merges on the STRINGS
        (join.py:241-246); per-table dictionary codes are incomparable across
        tables, so where dict_rewrites says so the rhs key codes are remapped
        into the lhs dictionary on device (a small host-built code→code map,
        one gather; a string absent from the lhs gets a code that never
        matches). lcols / rcols: the sides' columns by position. Returns a shadow
        (dc_rhs, rcols) for key building only — materialization keeps the
        original codes + dictionary."""
        sub = {}
        for (li, ri), rewrite in zip(
                zip(lhs_on, rhs_on),
                dict_rewrites([lcols[i] for i in lhs_on],
                              [rcols[i] for i in rhs_on])):
            if not rewrite:
                continue  # no strings, or codes already comparable
            dl, dr = lcols[li].dictionary, rcols[ri].dictionary
            index = {s: c for c, s in enumerate(dl)}
            miss = len(dl)  # sentinel: never present on the lhs side
            m = np.array([index.get(s, miss) for s in dr], dtype=np.int64)
            map_col = runtime.upload_column(m)
            codes = keys.codes_i32(runtime, rcols[ri])
            g = runtime.gather(map_col, codes.data,
                               dc_rhs.table.num_rows)
            rem = rt.DeviceColumn(runtime, g.data, rcols[ri].validity,
                                  g.len, rt.I64, owner=False,
                                  keep_alive=(g, rcols[ri], map_col, codes))
            rem.dictionary = dl
            sub[ri] = rem
        if not sub:
            return dc_rhs, rcols
        cc = dc_rhs.column_container
        cols2 = dict(dc_rhs.table.columns)
        for ri, col in sub.items():
            cols2[cc.get_backend_by_frontend_name(cc.columns[ri])] = col
        dc2 = DataContainer(DeviceTable(cols2), cc)
        return dc2, dc2.backend_cols()

    def _key_codes(self, runtime, dc, on, ranges, null_flags=None):
        """Build i64 code column + optional validity for join keys.
        null_flags (FULL OUTER, null-equal): per-key bools — NULL packs as
        its own code slot so NULL keys MATCH each other (pandas merge
        how="outer" matches NA keys; join.py:202-213 drops them only for
        inner/left/right/semi). Returns (codes, validity_ptr, keep, space)."""
        cols = dc.backend_cols()
        keyspecs = [(idx, mn, rng, nf) for idx, (mn, rng), nf
                    in zip(on, ranges, null_flags or [False] * len(on))]
        codes, space = runtime.keypack(cols, keyspecs, dc.table.num_rows)
        vcol = None
        if null_flags is None and any(cols[i].validity for i in on):
            # combined key validity (NULL-key semantics, join.py:202-213)
            expr_prog = []
            for i in on:
                expr_prog += [(OP_COL, i, 0), (OP_IS_NOT_NULL, 0, 0)]
                if len(expr_prog) > 2:
                    expr_prog.append((OP_AND, 0, 0))
            vcol = runtime.eval(runtime.make_prog(expr_prog), cols,
                                dc.table.num_rows, rt.BOOL8,
                                with_validity=False)
        return codes, vcol and vcol.data, vcol, space

    def _densify_join_float_key(self, runtime, lcol, rcol):
        """Float equi-join keys: every distinct f64 bit-pattern gets ONE dense
        integer id, consistent across BOTH sides (bits-mode groupby over the
        concatenation, ids joined back per row, as _densify_float_keys). NaN
        keys share an id — pandas merge matches NaN with NaN; NULL rows keep
        their validity and drop as usual. Returns (lid, rid, n_distinct)."""
        n_l, n_r = lcol.len, rcol.len
        cat = runtime.concat_columns([lcol, rcol], rt.F64)
        oc, ov, on_, G = runtime.hash_groupby(
            [cat], n_l + n_r, [(0, 0, 0, True, 1)], None, [])
        runtime._free(ov)
        runtime._free(on_)
        bcol = rt.DeviceColumn(runtime, oc, None, max(G, 1), rt.I64,
                               owner=True)
        pcodes, _ = runtime.keypack([cat], [(0, 0, 0, True, 1)], n_l + n_r)
        table = runtime.hash_build(bcol, None, code_max=0)
        try:
            p, b, cnt = runtime.hash_probe(table, pcodes, rt.JOIN_INNER,
                                           None)
            psel = runtime.wrap_sel(p, cnt)
            bsel = runtime.wrap_sel(b, cnt)
            assert cnt == n_l + n_r, (cnt, n_l + n_r)
            fid = runtime.scatter_rows(bsel, psel.data, cnt, n_l + n_r,
                                       with_validity=False)
        finally:
            runtime.hash_table_free(table)
        keep = (fid, lcol, rcol)
        # fid holds the scattered build positions: 4-byte ids like bsel
        assert fid.dtype == rt.I32, fid.dtype
        lid = rt.DeviceColumn(runtime, fid.data, lcol.validity, n_l,
                              rt.I32, owner=False, keep_alive=keep)
        rid = rt.DeviceColumn(runtime, fid.data + 4 * n_l, rcol.validity,
                              n_r, rt.I32, owner=False, keep_alive=keep)
        return lid, rid, G

    def _equi_join(self, runtime, dc_lhs, dc_rhs, lhs_on, rhs_on, join_type,
                   null_equal=False):
        """PAIR path: (probe_sel, build_sel) in (lhs, rhs) order, count."""
        lcols = dc_lhs.backend_cols()
        rcols = dc_rhs.backend_cols()
        for li, ri in zip(lhs_on, rhs_on):
            lk, rk = lcols[li].dtype, rcols[ri].dtype
            if (lk in _INT_KINDS) != (rk in _INT_KINDS):
                raise RexCompileError("join key type mismatch (int vs "
                                      "float) — cast one side first")
            if lk == rt.F32 or rk == rt.F32:
                raise RexCompileError("float32 join keys: cast to DOUBLE")
            if lk not in _INT_KINDS and lk != rt.F64:
                raise RexCompileError("unsupported join key dtype")
        n_l, n_r = dc_lhs.table.num_rows, dc_rhs.table.num_rows
        dc_rhs, rcols = self._reconcile_dict_keys(runtime, lcols, dc_rhs,
                                                  rcols, lhs_on, rhs_on)
        # f64 keys densify to consistent integer ids (single OR composite)
        float_pairs = [j for j, li in enumerate(lhs_on)
                       if lcols[li].dtype == rt.F64]
        dense_ranges = {}
        if float_pairs:
            lcols, rcols = list(lcols), list(rcols)
            lhs_on, rhs_on = list(lhs_on), list(rhs_on)
            for j in float_pairs:
                lid, rid, G = self._densify_join_float_key(
                    runtime, lcols[lhs_on[j]], rcols[rhs_on[j]])
                lcols.append(lid)
                rcols.append(rid)
                lhs_on[j] = len(lcols) - 1
                rhs_on[j] = len(rcols) - 1
                dense_ranges[j] = (0, max(G, 1))
            # the inputs' columns with this join's ids beside them
            dc_lhs, dc_rhs = (
                DataContainer(DeviceTable(dict(enumerate(c)), n),
                              ColumnContainer(range(len(c))))
                for c, n in ((lcols, n_l), (rcols, n_r)))
        # combined ranges over both sides so codes are comparable
        ranges = [dense_ranges[j] if j in dense_ranges
                  else keys.joint_range(runtime, lcols[li], rcols[ri])
                  for j, (li, ri) in enumerate(zip(lhs_on, rhs_on))]

        # build on the smaller side for INNER (what the reference gets from
        # dask's merge internals + JoinReorder,
        # src/sql/optimizer/join_reorder.rs)
        swap, ktype = jp.sides(join_type, n_l, n_r)
        if swap:
            probe_dc, build_dc = dc_rhs, dc_lhs
            probe_on, build_on = rhs_on, lhs_on
        else:
            probe_dc, build_dc = dc_lhs, dc_rhs
            probe_on, build_on = lhs_on, rhs_on

        # FULL OUTER: NULL keys get their own code slot so they MATCH each
        # other — the reference keeps both sides' NULL-key rows and pandas
        # merge how="outer" matches NA keys (join.py:202-213 drops NULL keys
        # only for inner/left/right/semi). ADVICE r1 (medium).
        null_flags = None
        if join_type == "outer" or null_equal:
            # null_equal: INTERSECT/EXCEPT semi/anti joins use DataFusion's
            # null_equals_null — NULL keys pack into their own slot and
            # match each other instead of being dropped
            pkc, bkc = probe_dc.backend_cols(), build_dc.backend_cols()
            null_flags = [
                bool(pkc[pi].validity) or bool(bkc[bi].validity)
                for pi, bi in zip(probe_on, build_on)]
        bcodes, bval, bkeep, bspace = self._key_codes(
            runtime, build_dc, build_on, ranges, null_flags)
        pcodes, pval, pkeep, _ = self._key_codes(
            runtime, probe_dc, probe_on, ranges, null_flags)
        table = runtime.hash_build(bcodes, bval, code_max=bspace - 1)
        try:
            p_ptr, b_ptr, count = runtime.hash_probe(
                table, pcodes, ktype, pval,
                mark_matched=(join_type == "outer"))
            probe_sel = runtime.wrap_sel(p_ptr, count)
            build_sel = runtime.wrap_sel(b_ptr, count)
            if join_type == "outer":
                # FULL = LEFT + unmatched build rows (test_join.py:46-66)
                ub_ptr, u_count = runtime.hash_unmatched(table)
                if u_count:
                    ub = runtime.wrap_sel(ub_ptr, u_count)
                    p_host = np.full(count + u_count, rt.NULL_IDX, np.uint32)
                    b_host = np.empty(count + u_count, dtype=np.uint32)
                    runtime._download(probe_sel.data, p_host[:count])
                    runtime._download(build_sel.data, b_host[:count])
                    runtime._download(ub.data, b_host[count:])
                    probe_sel = runtime.upload_column(p_host, dtype=rt.I32)
                    build_sel = runtime.upload_column(b_host, dtype=rt.I32)
                    count += u_count
                else:
                    runtime._free(ub_ptr)
        finally:
            runtime.hash_table_free(table)
        if swap:
            probe_sel, build_sel = build_sel, probe_sel
        return (probe_sel, build_sel), count

    def _run_radix(self, runtime, J, S):
        """Radix-partitioned equijoin (dsx_radix_join — VERDICT r1 #3, LDS-
        staged build/probe), which join_plan's size gates let through only
        when the flat probe table would spill the XCD L2. Returns
        ({combined_idx: DeviceColumn}, n_out), or None where the entry does
        not apply (over 16 columns on a side, or its own answer)."""
        bcols = S.build_kdc.backend_cols()
        pcols = S.probe_kdc.backend_cols()
        # NULL keys: pack them into their own code slot (nullable flag,
        # both sides identically) and DROP build-side NULL keys with a
        # predicate — code 0 then never matches, so INNER skips NULL-key
        # probe rows and LEFT null-extends them, exactly join.py:202-213
        null_flags = [bool(pcols[pi].validity) or bool(bcols[bi].validity)
                      for pi, bi in zip(S.probe_on, S.build_on)]
        keyspecs_b = [(bi, mn, rng, nf) for bi, (mn, rng), nf
                      in zip(S.build_on, S.ranges, null_flags)]
        keyspecs_p = [(pi, mn, rng, nf) for pi, (mn, rng), nf
                      in zip(S.probe_on, S.ranges, null_flags)]
        bpred = []
        for bi in S.build_on:
            if bcols[bi].validity:
                bpred += [(OP_COL, bi, 0), (OP_IS_NOT_NULL, 0, 0)]
                if len(bpred) > 2:
                    bpred.append((OP_AND, 0, 0))
        # output spec: mat_idx over `combined` → (side, col-in-side-array).
        # The arrays passed to C start as the (possibly dict-remapped) key
        # views; payloads whose original column was substituted by the
        # remap are APPENDED so outputs keep the original codes.
        b_arr = list(bcols)
        p_arr = list(pcols)
        out_specs = []
        srcs = []
        force_bv = S.ktype == rt.JOIN_LEFT
        for i in J.mat_idx:
            col = source_col(J, i)
            on_probe = (J.combined[i][0] == "l") != S.swap
            arr = p_arr if on_probe else b_arr
            ci = next((j for j, c in enumerate(arr) if c is col), None)
            if ci is None:
                arr.append(col)
                ci = len(arr) - 1
            need_valid = bool(col.validity) or (not on_probe and force_bv)
            out_specs.append((0 if on_probe else 1, ci, need_valid))
            srcs.append(col)
        if len(b_arr) > 16 or len(p_arr) > 16:
            return None  # DSX_MAX_COLS — flat path handles wide tables
        res = runtime.radix_join(
            b_arr, S.build_kdc.table.num_rows, keyspecs_b, keyspecs_p, bpred,
            p_arr, S.probe_kdc.table.num_rows, S.ktype, out_specs)
        if res is None:
            return None
        cols_out, n_out = res
        return {i: tag_output(col, src)
                for i, src, col in zip(J.mat_idx, srcs, cols_out)}, n_out

    def _run_fused(self, runtime, J, route, S, table=None):
        """Equi join with fused emit+materialization (dsx_hash_probe_cols):
        the probe's emit pass writes the output columns directly. Returns
        ({combined_idx: DeviceColumn}, n_out). Keys, ranges and sources of a
        side that stays pending come from its UNFILTERED base columns: a
        filter-probe side's predicate runs inside the probe
        (dsx_filter_probe_cols), and a filter-build side's table holds row
        ids that index the base columns. The ranges are the base columns'
        cached stats either way (_stats_src), so codes do not change."""
        pending = S.pending
        probe_kdc = S.probe_kdc
        # per-side materialization lists (sources: ORIGINAL tables)
        p_items, b_items = [], []
        for i in J.mat_idx:
            on_probe = (J.combined[i][0] == "l") != S.swap
            (p_items if on_probe else b_items).append(
                (i, source_col(J, i, S.dc_lhs, S.dc_rhs)))
        # only the fused filter-probe reads the key-membership filter; a
        # table handed in (a declined group-join's) is that same build
        if table is None:
            table = self.build_table(runtime, S, route,
                                     key_filter=pending is not None)
        try:
            res = None
            if pending is not None:
                res = runtime.filter_probe_cols(
                    table, runtime.make_prog(pending.prog), S.fp_cols,
                    S.fp_keys, pending.max_rows, [c for _, c in p_items],
                    [c for _, c in b_items])
                if res is None:
                    # duplicate build keys: run the filter after all and
                    # probe the same table the two-pass way
                    done = DataContainer(pending.table,
                                         pending.column_container)
                    if S.swap:
                        probe_kdc, _ = self._reconcile_dict_keys(
                            runtime, S.dc_lhs.backend_cols(), done,
                            done.backend_cols(), J.lhs_on, J.rhs_on)
                    else:
                        probe_kdc = done
                    p_items = [(i, source_col(J, i, *(
                        (S.dc_lhs, done) if S.swap else (done, S.dc_rhs))))
                        for i, _ in p_items]
            if res is None:
                pcodes, pval, pkeep, _ = self._key_codes(
                    runtime, probe_kdc, S.probe_on, S.ranges)
                res = runtime.hash_probe_cols(
                    table, pcodes, S.ktype, pval,
                    [c for _, c in p_items], [c for _, c in b_items],
                    force_build_validity=(S.ktype == rt.JOIN_LEFT))
            cols_out, n_out = res
        finally:
            runtime.hash_table_free(table)
        return {i: tag_output(col, src)
                for (i, src), col in zip(p_items + b_items, cols_out)}, n_out

    def _cross_join(self, runtime, dc_lhs, dc_rhs):
        # reference join.py:133-140 (merge on constant); tiny-only guard
        n_l, n_r = dc_lhs.table.num_rows, dc_rhs.table.num_rows
        if n_l * n_r > 50_000_000:
            raise NotImplementedError(
                f"cross join of {n_l}x{n_r} rows is unreasonable "
                "(reference warns ResourceWarning too, join.py:141-145)")
        p = np.repeat(np.arange(n_l, dtype=np.uint32), n_r)
        b = np.tile(np.arange(n_r, dtype=np.uint32), n_l)
        return (runtime.upload_column(p, dtype=rt.I32),
                runtime.upload_column(b, dtype=rt.I32)), int(n_l * n_r)

    def _split_join_condition(self, condition, n_lhs_cols):
        """reference join.py:250-322 — equi-keys + residual split."""
        rex_type = str(condition.getRexType())
        if rex_type in ("RexType.Literal", "RexType.Reference"):
            return [], [], [condition]
        if rex_type != "RexType.Call":
            raise NotImplementedError("Can not understand join condition.")
        try:
            lhs_on, rhs_on, residual = self._extract_lhs_rhs(condition,
                                                             n_lhs_cols)
        except AssertionError:
            return [], [], [condition]
        if lhs_on and rhs_on:
            return lhs_on, rhs_on, residual
        return [], [], [condition]

    def _extract_lhs_rhs(self, rex, n_lhs_cols):
        # reference join.py:274-322
        assert str(rex.getRexType()) == "RexType.Call"
        op = str(rex.getOperatorName())
        assert op in ("=", "AND")
        operands = rex.getOperands()
        assert len(operands) == 2
        if op == "=":
            a, b = operands
            if str(a.getRexType()) == "RexType.Reference" and \
                    str(b.getRexType()) == "RexType.Reference":
                ai, bi = a.getIndex(), b.getIndex()
                if ai > bi:
                    ai, bi = bi, ai
                assert ai < n_lhs_cols <= bi, "both refs on one side"
                return [ai], [bi - n_lhs_cols], []
            raise AssertionError("Invalid join condition")
        lhs_idx, rhs_idx, residual = [], [], []
        for operand in operands:
            try:
                li, ri, res = self._extract_lhs_rhs(operand, n_lhs_cols)
                lhs_idx.extend(li)
                rhs_idx.extend(ri)
                residual.extend(res)
            except AssertionError:
                residual.append(operand)
        return lhs_idx, rhs_idx, residual
