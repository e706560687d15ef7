"""Call-sequence characterisation of the sort front halves — test
infrastructure only. A fake runtime records what DaskSortPlugin._device_sort
and DaskWindowPlugin._device_sort_keys ask of the device (which engine, over
which columns, with which key specs, in which order) for a fixed list of
cases over fake columns with preset statistics; no GPU, no libdsxhip.so.

Run as a script it prints the traces as JSON:

    python tests/key_trace.py > tests/golden/key_trace.json

tests/test_key_trace.py replays the cases and compares with that file.

Per case the trace holds
  engine: every sort_perm / sort_word / keypack / window_mark_word /
          window_seg_ids / eval / upload / gather call in order, except
  rank:   the calls that build a dictionary's rank column (LUT upload, gather
          through the codes, min-max of the result), as a sorted set — how
          often a rank column is built is not part of the contract;
  result: what the entry point returned.
"""
import json
import os
import sys
import types
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from dask_sql_amd import runtime as rt  # noqa: E402
from dask_sql_amd.physical.rel_plugins import (DaskSortPlugin,  # noqa: E402
                                               DaskWindowPlugin)
from dask_sql_amd.planner.plan import WindowSpec  # noqa: E402

KNOBS = ("DSX_SORT_MIN", "DSX_DISABLE_RADIXSORT", "DSX_SORT_RADIX",
         "DSX_DISABLE_WINWORDS", "DSX_WIN_WORDS", "DSX_DISABLE_DEVWINDOW")
N = 100


class FakeCol:
    """Stands in for a DeviceColumn: dtype, validity, len, a distinct `data`
    handle and, for base columns, preset statistics."""
    _next = [1000]

    def __init__(self, name, dtype, minmax=None, nullable=False,
                 dictionary=None, n=N):
        self.name = name
        self.dtype = dtype
        self.len = n
        FakeCol._next[0] += 1
        self.data = FakeCol._next[0]
        self.validity = self.data + 500000 if nullable else None
        if minmax is not None:
            self._minmax = minmax
        if dictionary is not None:
            self.dictionary = dictionary


def base_columns():
    """The fixed table: index → column."""
    return [
        FakeCol("i", rt.I64, (5, 14, N)),
        FakeCol("f", rt.F64, nullable=True),
        FakeCol("d", rt.I32, (0, 2, N), nullable=True,
                dictionary=["b", None, "a"]),
        FakeCol("allnull", rt.I64, (0, 0, 0), nullable=True),
        FakeCol("big", rt.I64, (-(1 << 62), 1 << 62, N)),
        FakeCol("k0", rt.I64, (0, 9, N)),
        FakeCol("k1", rt.I32, (1, 100, N)),
        FakeCol("k2", rt.I64, (-3, 3, N), nullable=True),
        FakeCol("k3", rt.I8, (0, 1, N)),
        FakeCol("k4", rt.I64, (10, 1000, N)),
    ]


I, F, D, ALLNULL, BIG, K0, K1, K2, K3, K4 = range(10)


class FakeRuntime:
    lib = None
    ctx = None
    WIN_FUNCS = rt.Runtime.WIN_FUNCS
    WIN_ROWS_FUNCS = rt.Runtime.WIN_ROWS_FUNCS

    def __init__(self, cols, refuse_sort_perm=False, keypack_raises=False):
        self.calls = []
        self.refuse_sort_perm = refuse_sort_perm
        self.keypack_raises = keypack_raises
        self._by_data = {c.data: c for c in cols}
        self._uploads = {}   # data handle of an uploaded column → its record

    # ---- naming ----------------------------------------------------------
    def name(self, c):
        if c is None:
            return None
        nm = getattr(c, "name", None)
        if nm is not None:
            return nm
        ka = getattr(c, "_keep_alive", None)
        if isinstance(ka, tuple) and len(ka) == 3:
            # the ranked view of a dictionary column: (gather, source, lut)
            return f"rank({self.name(ka[1])})"
        return "?"

    def _new(self, name, n, dtype=rt.I64):
        c = FakeCol(name, dtype, n=n)
        self._by_data[c.data] = c
        return c

    def _sel(self, ptr):
        c = self._by_data.get(ptr)
        return self.name(c) if c is not None else "?"

    def _rec(self, **kw):
        self.calls.append(kw)
        return kw

    # ---- the Runtime surface the front halves use ------------------------
    def upload_column(self, arr, validity=None, dtype=None):
        arr = np.asarray(arr)
        rec = self._rec(call="upload", values=arr.tolist())
        c = self._new("upload", len(arr))
        self._uploads[c.data] = rec
        return c

    def gather(self, col, sel_ptr, n, force_validity=False):
        rec = self._rec(call="gather", col=self.name(col),
                        through=self._sel(sel_ptr), n=n,
                        force_validity=bool(force_validity))
        up = self._uploads.get(col.data)
        src = self._by_data.get(sel_ptr)
        if up is not None and getattr(src, "dictionary", None) is not None:
            # a LUT gathered through dictionary codes: the rank column
            up["rank_of"] = rec["rank_of"] = src.name
        return self._new(f"gather({self.name(col)})", n, col.dtype)

    def minmax_i64(self, col):
        nm = self.name(col)
        rec = self._rec(call="minmax", col=nm)
        if nm.startswith("rank("):
            rec["rank_of"] = nm[5:-1]
        return (0, 1, col.len)

    def sort_perm(self, cols, specs, n):
        self._rec(call="sort_perm", cols=[self.name(c) for c in cols],
                  specs=[list(s) for s in specs], n=n)
        if self.refuse_sort_perm:
            return None
        return self._new("perm", n, rt.I32)

    def sort_word(self, cols, specs, n, perm_in=None):
        self._rec(call="sort_word", cols=[self.name(c) for c in cols],
                  specs=[list(s) for s in specs], n=n,
                  perm_in=perm_in is not None)
        rng = [s[2] for s in specs if not s[4] & 8]
        if len(rng) == 1 and rng[0] > (1 << 62):
            return None  # dsx_sort_word answers -4 for such a key
        return self._new("perm", n, rt.I32)

    def keypack(self, cols, specs, n):
        self._rec(call="keypack", cols=[self.name(c) for c in cols],
                  specs=[list(s) for s in specs], n=n)
        if self.keypack_raises:
            raise rt.DsxError("key space overflow")
        return self._new(f"codes{len(specs)}", n), 1

    def window_mark_word(self, cols, specs, n, perm, marks=None):
        self._rec(call="window_mark_word",
                  cols=[self.name(c) for c in cols],
                  specs=[list(s) for s in specs], n=n,
                  perm=self.name(perm), marks_in=marks is not None)
        return marks if marks is not None else self._new("marks", n,
                                                         rt.BOOL8)

    def window_seg_ids(self, marks, n):
        self._rec(call="window_seg_ids", marks=self.name(marks), n=n)
        return self._new("ids", n), 3

    @staticmethod
    def make_prog(instrs):
        return tuple(instrs)

    def eval(self, prog, cols, n, out_dtype, with_validity=True):
        self._rec(call="eval", prog=[list(p) for p in prog],
                  cols=[self.name(c) for c in cols], n=n)
        return self._new("eval", n, out_dtype)

    # ---- the trace -------------------------------------------------------
    def trace(self):
        engine = [c for c in self.calls if "rank_of" not in c]
        rank = sorted({json.dumps(c, sort_keys=True)
                       for c in self.calls if "rank_of" in c})
        return engine, [json.loads(r) for r in rank]


def _wspec(part, order, nf=None):
    s = WindowSpec("rank", None, part, order, "o", None)
    if nf is not None:
        s.order_nf = nf
    return s


# (name, kind, args, options): kind "sort" takes a collation of
# (idx, ascending, nulls_first); kind "window" (part_idx, [(idx, desc)],
# order_nf | None). Options: env, refuse_sort_perm, keypack_raises,
# need_full.
CASES = [
    ("sort_int_asc", "sort", [(I, True, False)], {}),
    ("sort_int_desc_nulls_first", "sort", [(I, False, True)], {}),
    ("sort_int_dict", "sort", [(I, True, False), (D, False, True)], {}),
    ("sort_int_dict_refused", "sort", [(I, True, False), (D, False, True)],
     {"refuse_sort_perm": True}),
    ("sort_float_first", "sort", [(F, True, False), (I, False, False)], {}),
    ("sort_dict_float", "sort", [(D, True, True), (F, False, False)], {}),
    ("sort_allnull", "sort", [(ALLNULL, True, False), (I, True, True)], {}),
    ("sort_big", "sort", [(BIG, True, False)], {}),
    ("sort_big_refused", "sort", [(BIG, True, False)],
     {"refuse_sort_perm": True}),
    ("sort_five_keys_refused", "sort",
     [(K0, True, False), (K1, False, False), (K2, True, True),
      (K3, True, False), (K4, False, True)], {"refuse_sort_perm": True}),
    ("sort_sort_min_set", "sort", [(I, True, False)],
     {"env": {"DSX_SORT_MIN": "7"}}),
    ("sort_radix_off_float", "sort", [(I, True, False), (F, True, False)],
     {"env": {"DSX_DISABLE_RADIXSORT": "1"}}),
    ("sort_radix_off_refused", "sort", [(I, True, False)],
     {"env": {"DSX_DISABLE_RADIXSORT": "1"}, "refuse_sort_perm": True}),
    ("sort_radix_forced", "sort", [(I, True, False), (D, True, False)],
     {"env": {"DSX_SORT_RADIX": "1"}}),
    ("sort_radix_forced_but_off", "sort", [(I, True, False)],
     {"env": {"DSX_SORT_RADIX": "1", "DSX_DISABLE_RADIXSORT": "1"}}),
    ("win_part_dict_order_int_desc", "window",
     ([D], [(I, True)], None), {}),
    ("win_part_int_order_dict", "window", ([I], [(D, False)], None), {}),
    ("win_part_int_order_dict_refused", "window",
     ([I], [(D, False)], None), {"refuse_sort_perm": True}),
    ("win_part_int_order_dict_rows", "window",
     ([I], [(D, False)], None), {"need_full": False}),
    ("win_part_int_order_dict_refused_rows", "window",
     ([I], [(D, False)], None),
     {"refuse_sort_perm": True, "need_full": False}),
    ("win_order_dict_then_float", "window",
     ([I], [(D, False), (F, True)], None), {}),
    ("win_order_float_then_dict", "window",
     ([I], [(F, False), (D, True)], None), {}),
    ("win_part_float", "window", ([F], [(I, False)], None), {}),
    ("win_nulls_first", "window",
     ([I], [(K2, False), (D, True)], [True, None]), {}),
    ("win_nulls_last_explicit", "window",
     ([I], [(K2, True)], [False]), {}),
    ("win_no_partition", "window", ([], [(I, False)], None), {}),
    ("win_no_partition_refused", "window", ([], [(I, False)], None),
     {"refuse_sort_perm": True}),
    ("win_no_order", "window", ([I, D], [], None), {}),
    ("win_no_order_refused", "window", ([I, D], [], None),
     {"refuse_sort_perm": True}),
    ("win_no_keys", "window", ([], [], None), {}),
    ("win_allnull_part", "window", ([ALLNULL], [(I, False)], None), {}),
    ("win_allnull_part_refused", "window",
     ([ALLNULL], [(I, False)], None), {"refuse_sort_perm": True}),
    ("win_big_order", "window", ([I], [(BIG, False)], None),
     {"refuse_sort_perm": True}),
    ("win_five_keys_refused", "window",
     ([K0, K1], [(K2, False), (K3, True), (K4, False)], None),
     {"refuse_sort_perm": True}),
    ("win_keypack_raises", "window", ([I], [(K0, False)], None),
     {"keypack_raises": True}),
    ("win_words_off_refused", "window", ([I], [(D, False)], None),
     {"env": {"DSX_DISABLE_WINWORDS": "1"}, "refuse_sort_perm": True}),
    ("win_words_off_float", "window", ([I], [(F, False)], None),
     {"env": {"DSX_DISABLE_WINWORDS": "1"}}),
    ("win_words_off_nulls_first", "window",
     ([I], [(K0, False)], [True]),
     {"env": {"DSX_DISABLE_WINWORDS": "1"}}),
    ("win_words_forced", "window", ([I], [(D, True)], None),
     {"env": {"DSX_WIN_WORDS": "1"}}),
    ("win_words_forced_but_off", "window", ([I], [(K0, False)], None),
     {"env": {"DSX_WIN_WORDS": "1", "DSX_DISABLE_WINWORDS": "1"}}),
    ("win_devwindow_off", "ordered", ([I], [(K0, False)], None),
     {"env": {"DSX_DISABLE_DEVWINDOW": "1"}}),
]


def _run_sort(runtime, cols, collation):
    # the output table: four columns, one of them under two names
    names = [c.name for c in cols[:4]] + [cols[0].name]
    by_name = {c.name: c for c in cols}
    cc = types.SimpleNamespace(
        columns=names, get_backend_by_frontend_name=lambda f: f)
    table = types.SimpleNamespace(num_rows=N, col=lambda b: by_name[b])
    dc = types.SimpleNamespace(backend_cols=lambda: cols, table=table,
                               column_container=cc)
    ctx = types.SimpleNamespace(_get_runtime=lambda: runtime)
    out = DaskSortPlugin.__new__(DaskSortPlugin)._device_sort(
        ctx, dc, collation)
    if out is None:
        return None
    return {b: {"dictionary": getattr(g, "dictionary", None),
                "stats_src": runtime.name(getattr(g, "_stats_src", None))}
            for b, g in out.table.columns.items()}


def _run_window(runtime, cols, kind, part, order, nf, need_full):
    plug = DaskWindowPlugin.__new__(DaskWindowPlugin)
    spec = _wspec(part, order, nf)
    if kind == "ordered":
        out = plug._device_ordered(runtime, cols, N, spec)
        return None if out is None else "column"
    out = plug._device_sort_keys(runtime, cols, N, spec, need_full)
    if out is None:
        return None
    perm, ps, fs = out
    return {"perm": runtime.name(perm), "ps": runtime.name(ps),
            "fs": runtime.name(fs), "fs_is_ps": fs is ps}


def run_case(case):
    """Runs one case; returns (trace dict, the FakeRuntime)."""
    name, kind, args, opt = case
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(opt.get("env", {}))
    try:
        cols = base_columns()
        runtime = FakeRuntime(cols, opt.get("refuse_sort_perm", False),
                              opt.get("keypack_raises", False))
        if kind == "sort":
            result = _run_sort(runtime, cols, args)
        else:
            result = _run_window(runtime, cols, kind, *args,
                                 opt.get("need_full", True))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    engine, rank = runtime.trace()
    return {"engine": engine, "rank": rank, "result": result}, runtime


def run_all():
    return {case[0]: run_case(case)[0] for case in CASES}


if __name__ == "__main__":
    traces = run_all()
    sys.stdout.write("{\n" + ",\n".join(
        f"{json.dumps(k)}: {json.dumps(traces[k], sort_keys=True)}"
        for k in sorted(traces)) + "\n}\n")
