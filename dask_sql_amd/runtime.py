"""ctypes binding to libdsxhip.so — the C-ABI boundary (include/dsxhip.h).

This is the ONLY module that touches the HIP library. It fails LOUDLY when
the extension or a GPU is missing: there is no CPU fallback on the product
path.
"""
from __future__ import annotations

import ctypes as ct
from pathlib import Path

import numpy as np

# ---- dtype tags (include/dsxhip.h DsxType) --------------------------------
I64, F64, I32, F32, I8, BOOL8 = 0, 1, 2, 3, 4, 5

_NP_TO_DSX = {
    np.dtype("int64"): I64,
    np.dtype("float64"): F64,
    np.dtype("int32"): I32,
    np.dtype("float32"): F32,
    np.dtype("int8"): I8,
    np.dtype("uint8"): BOOL8,
    np.dtype("bool"): BOOL8,
}
_DSX_TO_NP = {
    I64: np.dtype("int64"),
    F64: np.dtype("float64"),
    I32: np.dtype("int32"),
    F32: np.dtype("float32"),
    I8: np.dtype("int8"),
    BOOL8: np.dtype("uint8"),
}
_DSX_SIZE = {I64: 8, F64: 8, I32: 4, F32: 4, I8: 1, BOOL8: 1}

MAX_PROG = 120
MAX_COLS = 16
MAX_AGGS = 16
MAX_KEYS = 4

# agg ops (include/dsxhip.h DsxAggOp)
AGG_SUM_F64, AGG_SUM_I64, AGG_COUNT = 0, 1, 2
AGG_MIN_F64, AGG_MAX_F64, AGG_MIN_I64, AGG_MAX_I64 = 3, 4, 5, 6

JOIN_INNER, JOIN_LEFT, JOIN_LEFTSEMI, JOIN_LEFTANTI = 0, 1, 2, 3
NULL_IDX = 0xFFFFFFFF
NOT_APPLICABLE = 1  # DSX_NOT_APPLICABLE (dsx_filter_probe_cols)
# 64-row words per wave iteration of the generated filter-probe mask kernel
# (DSX_FPROBE_JIT_WORDS, csrc/jit_kernels.inc)
FPROBE_JIT_WORDS = 1


class DsxError(RuntimeError):
    pass


class DsxUnavailable(DsxError):
    """Raised when libdsxhip.so / a GPU is not available. The product path
    must propagate this — never fall back to CPU."""


class _Instr(ct.Structure):
    _fields_ = [("op", ct.c_int32), ("arg0", ct.c_int32), ("imm", ct.c_int64)]


class _Column(ct.Structure):
    _fields_ = [
        ("data", ct.c_void_p),
        ("validity", ct.c_void_p),
        ("len", ct.c_int64),
        ("dtype", ct.c_int32),
    ]


class _KeySpec(ct.Structure):
    _fields_ = [
        ("col", ct.c_int32),
        ("min", ct.c_int64),
        ("range", ct.c_int64),
        ("nullable", ct.c_int32),
        ("mode", ct.c_int32),
    ]


class _AggSpec(ct.Structure):
    _fields_ = [
        ("op", ct.c_int32),
        ("prog_len", ct.c_int32),
        ("prog", _Instr * MAX_PROG),
    ]


class _WinBound(ct.Structure):
    _fields_ = [("kind", ct.c_int32), ("ival", ct.c_int64),
                ("fval", ct.c_double)]


class _GbFinishCall(ct.Structure):
    _fields_ = [("kind", ct.c_int32), ("agg", ct.c_int32)]


_LIB = None


def _load_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = Path(__file__).resolve().parent / "libdsxhip.so"
    if not so.exists():
        raise DsxUnavailable(
            f"HIP extension not built: {so} missing. Run `make -C "
            f"{so.parent / 'csrc'}` (hipcc --offload-arch=gfx950). "
            "The MI355X execution layer has NO CPU fallback."
        )
    lib = ct.CDLL(str(so))
    lib.dsx_last_error.restype = ct.c_char_p
    lib.dsx_ctx_create.argtypes = [ct.c_int, ct.POINTER(ct.c_void_p)]
    _LIB = lib
    return lib


def _check(lib, rc, what):
    if rc != 0:
        raise DsxError(f"{what} failed ({rc}): {lib.dsx_last_error().decode()}")


class DeviceColumn:
    """A device-resident column: data ptr + optional validity + dtype."""

    def __init__(self, rt, data, validity, length, dtype, owner=True,
                 keep_alive=None):
        self.rt = rt
        self.data = data
        self.validity = validity  # device ptr or None
        self.len = length
        self.dtype = dtype
        self._owner = owner
        self._keep_alive = keep_alive  # e.g. torch tensor backing the ptrs

    def c_struct(self):
        # cached: data/validity/len are immutable after construction and
        # ~40 ctypes struct builds per query step measured on the Q3 host
        # overhead profile
        c = getattr(self, "_c_struct", None)
        if c is None:
            c = _Column(self.data, self.validity or None, self.len,
                        self.dtype)
            self._c_struct = c
        return c

    def __del__(self):
        if getattr(self, "_owner", False) and self.rt and self.rt.lib:
            try:
                self.rt.lib.dsx_free(self.rt.ctx, ct.c_void_p(self.data))
                if self.validity:
                    self.rt.lib.dsx_free(self.rt.ctx, ct.c_void_p(self.validity))
            except Exception:
                pass

    def to_numpy(self):
        np_dtype = _DSX_TO_NP[self.dtype]
        out = np.empty(self.len, dtype=np_dtype)
        self.rt._download(self.data, out)
        if self.validity:
            v = np.empty(self.len, dtype=np.uint8)
            self.rt._download(self.validity, v)
            return out, v.astype(bool)
        return out, None


class Runtime:
    """One GPU, one HIP stream, one ctypes session (include/dsxhip.h)."""

    def __init__(self, device_id: int = 0):
        self.lib = _load_lib()
        ctx = ct.c_void_p()
        rc = self.lib.dsx_ctx_create(ct.c_int(device_id), ct.byref(ctx))
        if rc != 0:
            raise DsxUnavailable(
                f"dsx_ctx_create({device_id}) failed: "
                f"{self.lib.dsx_last_error().decode()} — is a GPU visible?"
            )
        self.ctx = ctx
        self.device_id = device_id

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.dsx_ctx_destroy(self.ctx)
            self.ctx = None

    # ---- memory ----------------------------------------------------------
    def _malloc(self, nbytes) -> int:
        p = ct.c_void_p()
        _check(self.lib, self.lib.dsx_malloc(self.ctx, ct.c_int64(max(nbytes, 1)),
                                             ct.byref(p)), "dsx_malloc")
        return p.value

    def _free(self, ptr):
        if ptr:
            self.lib.dsx_free(self.ctx, ct.c_void_p(ptr))

    def _upload_raw(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = ct.c_void_p()
        _check(
            self.lib,
            self.lib.dsx_upload(self.ctx, arr.ctypes.data_as(ct.c_void_p),
                                ct.c_int64(arr.nbytes), ct.byref(p)),
            "dsx_upload",
        )
        return p.value

    def copy_raw(self, dst_ptr: int, src_ptr: int, nbytes: int):
        """Device→device copy (dsx_copy / hipMemcpyAsync on the lib
        stream); staging into externally-owned buffers (e.g. torch tensors
        for RCCL collectives)."""
        if nbytes:
            _check(self.lib,
                   self.lib.dsx_copy(self.ctx, ct.c_void_p(dst_ptr),
                                     ct.c_void_p(src_ptr),
                                     ct.c_int64(nbytes)), "dsx_copy")

    def _download(self, dev_ptr, out: np.ndarray):
        _check(
            self.lib,
            self.lib.dsx_download(self.ctx, ct.c_void_p(dev_ptr),
                                  out.ctypes.data_as(ct.c_void_p),
                                  ct.c_int64(out.nbytes)),
            "dsx_download",
        )

    _PINNED_MIN = 8 << 20  # below this the pageable path is fine

    def upload_column(self, arr: np.ndarray, validity: np.ndarray | None = None,
                      dtype: int | None = None) -> DeviceColumn:
        if dtype is None:
            dtype = _NP_TO_DSX[arr.dtype]
        data = self._upload_raw_auto(arr)
        vptr = None
        if validity is not None:
            vptr = self._upload_raw_auto(validity.astype(np.uint8))
        return DeviceColumn(self, data, vptr, len(arr), dtype)

    def _upload_raw_auto(self, arr: np.ndarray) -> int:
        """Large buffers go through the pinned staging arena
        (dsx_upload_pinned — chunked memcpy + hipMemcpyAsync overlap);
        small ones take the plain path."""
        arr = np.ascontiguousarray(arr)
        if arr.nbytes < self._PINNED_MIN:
            return self._upload_raw(arr)
        p = ct.c_void_p()
        _check(
            self.lib,
            self.lib.dsx_upload_pinned(self.ctx,
                                       arr.ctypes.data_as(ct.c_void_p),
                                       ct.c_int64(arr.nbytes), ct.byref(p)),
            "dsx_upload_pinned",
        )
        return p.value

    def empty_column(self, n: int, dtype: int, with_validity=False) -> DeviceColumn:
        data = self._malloc(n * _DSX_SIZE[dtype])
        vptr = self._malloc(n) if with_validity else None
        return DeviceColumn(self, data, vptr, n, dtype)

    def synchronize(self):
        _check(self.lib, self.lib.dsx_synchronize(self.ctx), "dsx_synchronize")

    # ---- profiling -------------------------------------------------------
    def prof_enable(self, on=True):
        self.lib.dsx_prof_enable(self.ctx, 1 if on else 0)

    def prof_reset(self):
        self.lib.dsx_prof_reset(self.ctx)

    def prof_get(self) -> dict:
        cap = 64  # more than the library has kernel families
        names = ((ct.c_char * 32) * cap)()
        ms = (ct.c_double * cap)()
        launches = (ct.c_int64 * cap)()
        n = self.lib.dsx_prof_get(self.ctx, names, ms, launches, cap)
        return {
            names[i].value.decode(): {"ms": ms[i], "launches": launches[i]}
            for i in range(n)
        }

    # ---- helpers ---------------------------------------------------------
    # stack effect per opcode family (VM slots are 6 named registers —
    # dsxhip.hip VmStack; exceeding them would silently alias slot 5)
    _PUSH_OPS = {1, 2, 3, 4}          # COL, LIT_*
    # arith/cmp/AND/OR + POW(71), FLOORMOD(75), ATAN2(82): each pops two
    _BIN_OPS = set(range(10, 42)) | {71, 75, 82}
    _SELECT_OP = 60
    _MAX_DEPTH = 8

    @classmethod
    def _check_depth(cls, instrs):
        depth = 0
        peak = 0
        for op, _, _ in instrs:
            if op in cls._PUSH_OPS:
                depth += 1
            elif op in cls._BIN_OPS and op != 42:  # NOT(42) is unary
                depth -= 1
            elif op == cls._SELECT_OP:
                depth -= 2
            peak = max(peak, depth)
        if peak > cls._MAX_DEPTH:
            raise DsxError(
                f"expression too deep for the VM register stack "
                f"({peak} > {cls._MAX_DEPTH}); split the expression "
                "(e.g. nested CASE) into projection steps")

    @staticmethod
    def make_prog(instrs) -> tuple:
        """instrs: list of (op, arg0, imm) where imm may be float/int.
        Cached by content — the ctypes arrays are immutable after build and
        the C side copies them, so reuse across steps is safe."""
        return Runtime._make_prog_cached(tuple(instrs))

    @staticmethod
    def _make_prog_cached(instrs) -> tuple:
        cache = Runtime._prog_cache
        hit = cache.get(instrs)
        if hit is not None:
            return hit
        if len(instrs) > MAX_PROG:
            raise DsxError(f"program too long ({len(instrs)})")
        Runtime._check_depth(instrs)
        arr = (_Instr * max(len(instrs), 1))()
        for i, (op, arg0, imm) in enumerate(instrs):
            arr[i].op = op
            arr[i].arg0 = arg0
            if isinstance(imm, float):
                arr[i].imm = int.from_bytes(
                    np.float64(imm).tobytes(), "little", signed=True
                )
            else:
                arr[i].imm = int(imm)
        if len(cache) > 4096:
            cache.clear()
        cache[instrs] = (arr, len(instrs))
        return arr, len(instrs)

    _prog_cache: dict = {}

    @staticmethod
    def _cols_array(cols):
        arr = (_Column * max(len(cols), 1))()
        for i, c in enumerate(cols):
            arr[i] = c.c_struct()
        return arr

    @staticmethod
    def _keyspec_array(keyspecs):
        """DsxKeySpec array of (col, min, range, nullable[, mode]) tuples;
        a missing mode is 0. At least one element, so that an empty key
        list still passes a valid pointer."""
        ks = (_KeySpec * max(len(keyspecs), 1))()
        for k, spec in zip(ks, keyspecs):
            k.col = spec[0]
            k.min = spec[1]
            k.range = spec[2]
            k.nullable = 1 if spec[3] else 0
            if len(spec) > 4:
                k.mode = spec[4]
        return ks

    @staticmethod
    def _aggspec_array(agg_specs):
        """DsxAggSpec array of (agg_op, prog) pairs."""
        aggs = (_AggSpec * max(len(agg_specs), 1))()
        for a, (op, (parr, plen)) in zip(aggs, agg_specs):
            a.op = op
            a.prog_len = plen
            ct.memmove(a.prog, parr, plen * ct.sizeof(_Instr))
        return aggs

    @staticmethod
    def _hist_cache_unsafe(cols, keyspecs):
        """The C-side group-by hist cache keys on device pointers with
        pool-free eviction; externally-backed key columns (torch/RCCL
        staging) recycle pointers outside that hook — the cache is switched
        off around a call over them."""
        return any(
            getattr(cols[spec[0]], "_keep_alive", None) is not None
            and not getattr(cols[spec[0]], "_owner", True)
            for spec in keyspecs)

    # ---- ops -------------------------------------------------------------
    def eval(self, prog, cols, n, out_dtype, with_validity=True) -> DeviceColumn:
        parr, plen = prog
        out = self.empty_column(n, out_dtype, with_validity)
        _check(
            self.lib,
            self.lib.dsx_eval(self.ctx, parr, ct.c_int(plen),
                              self._cols_array(cols), ct.c_int(len(cols)),
                              ct.c_int64(n), ct.c_void_p(out.data),
                              ct.c_void_p(out.validity) if out.validity else None,
                              ct.c_int32(out_dtype)),
            "dsx_eval",
        )
        return out

    def filter(self, prog, cols, n):
        """Returns (sel_device_ptr, count) — ordered selection vector."""
        parr, plen = prog
        sel = ct.c_void_p()
        count = ct.c_int64()
        _check(
            self.lib,
            self.lib.dsx_filter(self.ctx, parr, ct.c_int(plen),
                                self._cols_array(cols), ct.c_int(len(cols)),
                                ct.c_int64(n), ct.byref(sel), ct.byref(count)),
            "dsx_filter",
        )
        return sel.value, count.value

    def gather_into(self, col: DeviceColumn, sel_ptr, n_sel, out_ptr: int):
        """Gather into a caller-owned device buffer (e.g. a torch tensor's
        storage, for the RCCL shuffle staging — SURVEY §8e)."""
        _check(
            self.lib,
            self.lib.dsx_gather(self.ctx, ct.byref(col.c_struct()),
                                ct.c_void_p(sel_ptr), ct.c_int64(n_sel),
                                ct.c_void_p(out_ptr), None),
            "dsx_gather",
        )

    def wrap_devptr(self, ptr: int, n: int, dtype: int,
                    keep_alive=None) -> DeviceColumn:
        """Wrap an externally-owned device buffer (e.g. torch tensor)."""
        return DeviceColumn(self, ptr, None, n, dtype, owner=False,
                            keep_alive=keep_alive)

    def concat_columns(self, cols, dtype) -> DeviceColumn:
        """Concatenate device columns of one dtype (UNION ALL — reference
        dd.concat). Validity kept if any input has one (absent = all-1)."""
        total = sum(c.len for c in cols)
        need_valid = any(c.validity for c in cols)
        out = self.empty_column(total, dtype, need_valid)
        sz = _DSX_SIZE[dtype]
        off = 0
        for c in cols:
            assert c.dtype == dtype
            if c.len:
                _check(self.lib,
                       self.lib.dsx_copy(self.ctx,
                                         ct.c_void_p(out.data + off * sz),
                                         ct.c_void_p(c.data),
                                         ct.c_int64(c.len * sz)), "dsx_copy")
                if need_valid:
                    if c.validity:
                        _check(self.lib, self.lib.dsx_copy(
                            self.ctx, ct.c_void_p(out.validity + off),
                            ct.c_void_p(c.validity), ct.c_int64(c.len)),
                            "dsx_copy")
                    else:
                        _check(self.lib, self.lib.dsx_memset(
                            self.ctx, ct.c_void_p(out.validity + off),
                            ct.c_int(1), ct.c_int64(c.len)), "dsx_memset")
            off += c.len
        return out

    def scatter_rows(self, col: DeviceColumn, sel_ptr, n_sel, n_out,
                     with_validity=True) -> DeviceColumn:
        """out[sel[i]] = col[i] (inverse of gather; window/join-back
        placement). Rows not covered by sel come out NULL."""
        out = self.empty_column(n_out, col.dtype, with_validity)
        if out.validity:
            _check(self.lib,
                   self.lib.dsx_memset(self.ctx, ct.c_void_p(out.validity),
                                       ct.c_int(0), ct.c_int64(n_out)),
                   "dsx_memset")
        _check(
            self.lib,
            self.lib.dsx_scatter_rows(self.ctx, ct.byref(col.c_struct()),
                                      ct.c_void_p(sel_ptr),
                                      ct.c_int64(n_sel), ct.c_int64(n_out),
                                      ct.c_void_p(out.data),
                                      ct.c_void_p(out.validity)
                                      if out.validity else None),
            "dsx_scatter_rows",
        )
        return out

    def gather(self, col: DeviceColumn, sel_ptr, n_sel,
               force_validity=False) -> DeviceColumn:
        need_valid = force_validity or bool(col.validity)
        out = self.empty_column(n_sel, col.dtype, need_valid)
        _check(
            self.lib,
            self.lib.dsx_gather(self.ctx, ct.byref(col.c_struct()),
                                ct.c_void_p(sel_ptr), ct.c_int64(n_sel),
                                ct.c_void_p(out.data),
                                ct.c_void_p(out.validity) if out.validity else None),
            "dsx_gather",
        )
        return out

    def minmax_i64(self, col: DeviceColumn):
        mn = ct.c_int64()
        mx = ct.c_int64()
        nn = ct.c_int64()
        _check(
            self.lib,
            self.lib.dsx_minmax_i64(self.ctx, ct.byref(col.c_struct()),
                                    ct.byref(mn), ct.byref(mx), ct.byref(nn)),
            "dsx_minmax_i64",
        )
        return mn.value, mx.value, nn.value

    def keypack(self, cols, keyspecs, n) -> tuple:
        """keyspecs: list of (col_idx, min, range, nullable).
        Returns (codes DeviceColumn(u64-as-i64), key_space)."""
        ks = self._keyspec_array(keyspecs)
        space = 1
        for spec in keyspecs:
            space *= spec[2] + (1 if spec[3] else 0)
        out = self.empty_column(n, I64, False)
        _check(
            self.lib,
            self.lib.dsx_keypack(self.ctx, self._cols_array(cols),
                                 ct.c_int(len(cols)), ks, ct.c_int(len(keyspecs)),
                                 ct.c_int64(n), ct.c_void_p(out.data)),
            "dsx_keypack",
        )
        return out, space

    def hash_build(self, codes: DeviceColumn, validity_ptr=None, code_max=0,
                   key_filter=False):
        """key_filter: also build the key-membership filter that
        filter_probe_cols consults (dsx_hash_build_filtered); only a table
        that goes to filter_probe_cols asks for it."""
        t = ct.c_void_p()
        vptr = ct.c_void_p(validity_ptr) if validity_ptr else None
        if key_filter:
            _check(
                self.lib,
                self.lib.dsx_hash_build_filtered(
                    self.ctx, ct.c_void_p(codes.data), vptr,
                    ct.c_int64(codes.len), ct.c_uint64(code_max), ct.c_int(1),
                    ct.byref(t)),
                "dsx_hash_build_filtered",
            )
            return t
        _check(
            self.lib,
            self.lib.dsx_hash_build(self.ctx, ct.c_void_p(codes.data), vptr,
                                    ct.c_int64(codes.len),
                                    ct.c_uint64(code_max), ct.byref(t)),
            "dsx_hash_build",
        )
        return t

    def hash_build_cols(self, prog, cols, keyspecs, n, code_max=0,
                        key_filter=False):
        """hash_build straight from source columns (dsx_hash_build_cols):
        predicate `prog` over `cols` (None or an empty program keeps every
        row), NULL-key drop, key pack (keyspecs as for keypack, indexing
        `cols`) and insert in one sweep, without a wait. Row ids in the table
        index `cols`; the table is sized by n."""
        parr, plen = prog if prog is not None else (None, 0)
        t = ct.c_void_p()
        _check(
            self.lib,
            self.lib.dsx_hash_build_cols(
                self.ctx, parr, ct.c_int(plen), self._cols_array(cols),
                ct.c_int(len(cols)), self._keyspec_array(keyspecs),
                ct.c_int(len(keyspecs)), ct.c_int64(n), ct.c_uint64(code_max),
                ct.c_int(1 if key_filter else 0), ct.byref(t)),
            "dsx_hash_build_cols",
        )
        return t

    def hash_table_filter(self, table):
        """(mode, bytes) of the table's key-membership filter: mode 0 none,
        1 exact bitmap, 2 hashed (csrc/join_filter.h)."""
        self.lib.dsx_hash_table_filter_mode.restype = ct.c_int
        self.lib.dsx_hash_table_filter_bytes.restype = ct.c_int64
        return (int(self.lib.dsx_hash_table_filter_mode(table)),
                int(self.lib.dsx_hash_table_filter_bytes(table)))

    def join_filter_builds(self):
        """(none, exact, hashed): how many hash_build(key_filter=True) calls
        on this runtime ended in each filter mode so far."""
        self.lib.dsx_join_filter_builds.restype = ct.c_int64
        return tuple(int(self.lib.dsx_join_filter_builds(self.ctx, ct.c_int(m)))
                     for m in range(3))

    def hash_probe(self, table, codes: DeviceColumn, join_type,
                   validity_ptr=None, mark_matched=False):
        p = ct.c_void_p()
        b = ct.c_void_p()
        count = ct.c_int64()
        _check(
            self.lib,
            self.lib.dsx_hash_probe(self.ctx, table, ct.c_void_p(codes.data),
                                    ct.c_void_p(validity_ptr) if validity_ptr else None,
                                    ct.c_int64(codes.len), ct.c_int(join_type),
                                    ct.c_int(1 if mark_matched else 0),
                                    ct.byref(p), ct.byref(b), ct.byref(count)),
            "dsx_hash_probe",
        )
        return p.value, b.value, count.value

    def hash_unmatched(self, table):
        b = ct.c_void_p()
        count = ct.c_int64()
        _check(
            self.lib,
            self.lib.dsx_hash_unmatched(self.ctx, table, ct.byref(b),
                                        ct.byref(count)),
            "dsx_hash_unmatched",
        )
        return b.value, count.value

    def topk_rows(self, cols, key_idx, desc, n, k, cap):
        """Candidate rows of ORDER BY ... LIMIT k (dsx_topk_rows): the rows
        whose primary key cols[key_idx] sorts at or before the k-th row's,
        selected on the device and fetched with one wait. Returns
        (row_ids u32[count], [(values, valid-bool-or-None) per column]) as
        host arrays in no particular order, or None when the call is not
        applicable (NULL / NaN primary key, ties past `cap`)."""
        nc = len(cols)
        host = ct.c_void_p()
        offs = (ct.c_int64 * (1 + 2 * nc))()
        count = ct.c_int64()
        rc = self.lib.dsx_topk_rows(
            self.ctx, self._cols_array(cols), ct.c_int(nc),
            ct.c_int(key_idx), ct.c_int(1 if desc else 0), ct.c_int64(n),
            ct.c_int64(k), ct.c_int64(cap), ct.byref(host), offs,
            ct.byref(count))
        if rc == NOT_APPLICABLE:
            return None
        _check(self.lib, rc, "dsx_topk_rows")
        cnt = count.value

        def view(off, np_dtype):
            # copy out of the context's pinned buffer: the next call reuses it
            buf = (ct.c_char * (cnt * np_dtype.itemsize)).from_address(
                host.value + off)
            return np.frombuffer(buf, dtype=np_dtype, count=cnt).copy()

        rowids = view(offs[0], np.dtype("uint32"))
        out = []
        for i, c in enumerate(cols):
            vals = view(offs[1 + 2 * i], _DSX_TO_NP[c.dtype])
            voff = offs[2 + 2 * i]
            valid = view(voff, np.dtype("uint8")).astype(bool) \
                if voff >= 0 else None
            out.append((vals, valid))
        return rowids, out

    def filter_cols(self, prog, cols, n, mats):
        """Fused filter + materialization (dsx_filter_cols): returns
        ([DeviceColumn per mat], n_out)."""
        parr, plen = prog
        nm = len(mats)
        datas = (ct.c_void_p * max(nm, 1))()
        valids = (ct.c_void_p * max(nm, 1))()
        count = ct.c_int64()
        _check(
            self.lib,
            self.lib.dsx_filter_cols(
                self.ctx, parr, ct.c_int(plen), self._cols_array(cols),
                ct.c_int(len(cols)), ct.c_int64(n),
                self._cols_array(mats), ct.c_int(nm), datas, valids,
                ct.byref(count)),
            "dsx_filter_cols",
        )
        nr = count.value
        return [DeviceColumn(self, datas[i], valids[i] or None, nr,
                             m.dtype, owner=True)
                for i, m in enumerate(mats)], nr

    def hash_probe_cols(self, table, codes: DeviceColumn, join_type,
                        validity_ptr, pcols, bcols, force_build_validity):
        """Fused probe-emit + materialization (dsx_hash_probe_cols): returns
        ([DeviceColumn] ordered pcols then bcols, n_out)."""
        ncols = len(pcols) + len(bcols)
        datas = (ct.c_void_p * max(ncols, 1))()
        valids = (ct.c_void_p * max(ncols, 1))()
        count = ct.c_int64()
        _check(
            self.lib,
            self.lib.dsx_hash_probe_cols(
                self.ctx, table, ct.c_void_p(codes.data),
                ct.c_void_p(validity_ptr) if validity_ptr else None,
                ct.c_int64(codes.len), ct.c_int(join_type),
                self._cols_array(pcols), ct.c_int(len(pcols)),
                self._cols_array(bcols), ct.c_int(len(bcols)),
                ct.c_int(1 if force_build_validity else 0),
                datas, valids, ct.byref(count)),
            "dsx_hash_probe_cols",
        )
        n = count.value
        out = []
        for i, src in enumerate(list(pcols) + list(bcols)):
            out.append(DeviceColumn(self, datas[i], valids[i] or None, n,
                                    src.dtype, owner=True))
        return out, n

    def filter_probe_cols(self, table, prog, cols, keyspecs, n, pcols,
                          bcols):
        """Fused scan filter + key pack + probe + materialization
        (dsx_filter_probe_cols) over the unfiltered probe columns `cols`;
        keyspecs as for keypack, indexing `cols`. Returns ([DeviceColumn]
        ordered pcols then bcols, n_out), or None when the build keys are
        not unique (nothing was allocated)."""
        parr, plen = prog
        ks = self._keyspec_array(keyspecs)
        ncols = len(pcols) + len(bcols)
        datas = (ct.c_void_p * max(ncols, 1))()
        valids = (ct.c_void_p * max(ncols, 1))()
        count = ct.c_int64()
        rc = self.lib.dsx_filter_probe_cols(
            self.ctx, table, parr, ct.c_int(plen), self._cols_array(cols),
            ct.c_int(len(cols)), ks, ct.c_int(len(keyspecs)), ct.c_int64(n),
            self._cols_array(pcols), ct.c_int(len(pcols)),
            self._cols_array(bcols), ct.c_int(len(bcols)),
            datas, valids, ct.byref(count))
        if rc == NOT_APPLICABLE:
            return None
        _check(self.lib, rc, "dsx_filter_probe_cols")
        nr = count.value
        return [DeviceColumn(self, datas[i], valids[i] or None, nr,
                             src.dtype, owner=True)
                for i, src in enumerate(list(pcols) + list(bcols))], nr

    def fprobe_jit_launches(self) -> int:
        """Launches so far of the per-shape generated mask kernel of
        filter_probe_cols (dsx_fprobe_jit_launches). A call that leaves the
        count unchanged ran the interpreter kernel (DSX_DISABLE_JIT,
        DSX_DISABLE_JIT_FPROBE=1, a rejected predicate, a hipRTC failure) or
        had no rows."""
        self.lib.dsx_fprobe_jit_launches.restype = ct.c_int64
        return int(self.lib.dsx_fprobe_jit_launches(self.ctx))

    def radix_join(self, bcols, n_build, keyspecs_b, keyspecs_p, bpred_prog,
                   pcols, n_probe, join_type, out_specs):
        """Radix-partitioned equijoin (dsx_radix_join): out_specs =
        [(side, col_idx, need_valid)] with side 0=probe/1=build and col_idx
        into that side's cols array. Returns ([DeviceColumn], n) or None on
        bucket overflow / unsupported shape (caller falls back to the
        flat-table join)."""
        nk = len(keyspecs_b)
        kb = self._keyspec_array(keyspecs_b)
        kp = self._keyspec_array(keyspecs_p)
        n_out = len(out_specs)
        side_a = (ct.c_int32 * n_out)(*[s[0] for s in out_specs])
        col_a = (ct.c_int32 * n_out)(*[s[1] for s in out_specs])
        nv_a = (ct.c_int32 * n_out)(*[1 if s[2] else 0 for s in out_specs])
        datas = (ct.c_void_p * n_out)()
        valids = (ct.c_void_p * n_out)()
        count = ct.c_int64()
        bp = None
        bl = 0
        if bpred_prog:
            bp, bl = self.make_prog(bpred_prog)
        rc = self.lib.dsx_radix_join(
            self.ctx, self._cols_array(bcols), ct.c_int(len(bcols)),
            ct.c_int64(n_build), kb, kp, ct.c_int(nk),
            bp, ct.c_int(bl),
            self._cols_array(pcols), ct.c_int(len(pcols)),
            ct.c_int64(n_probe), ct.c_int(join_type),
            side_a, col_a, nv_a, ct.c_int(n_out),
            datas, valids, ct.byref(count))
        if rc in (-5, -6):
            return None  # skew overflow / degenerate: flat-table fallback
        _check(self.lib, rc, "dsx_radix_join")
        n = count.value
        out = []
        for i, (side, ci, _) in enumerate(out_specs):
            src = bcols[ci] if side else pcols[ci]
            out.append(DeviceColumn(self, datas[i], valids[i] or None, n,
                                    src.dtype, owner=True))
        return out, n

    def sort_perm(self, cols, keyspecs, n):
        """Device ORDER BY permutation (dsx_sort_perm): keyspecs =
        (col, min, range, nullable, mode) with mode bit1=DESC,
        bit2=NULLS LAST, passed in REVERSED significance order. Returns a
        DeviceColumn of u32 row ids or None (unsupported/skew → host)."""
        nk = len(keyspecs)
        ks = self._keyspec_array(keyspecs)
        perm = ct.c_void_p()
        rc = self.lib.dsx_sort_perm(self.ctx, self._cols_array(cols),
                                    ct.c_int(len(cols)), ks, ct.c_int(nk),
                                    ct.c_int64(n), ct.byref(perm))
        if rc in (-3, -4, -6):
            return None
        _check(self.lib, rc, "dsx_sort_perm")
        return DeviceColumn(self, perm.value, None, n, I32, owner=True)

    def sort_word(self, cols, keyspecs, n, perm_in=None):
        """Stable device sort of a row-id sequence by ONE 64-bit order word
        (dsx_sort_word, LSD radix). `cols` are the word's own key columns,
        keyspecs = (col, min, range, nullable, mode) as for sort_perm, or a
        single float key with mode bit 8. perm_in: DeviceColumn of u32 row
        ids to reorder (None = identity). Chained least significant word
        first it sorts composite keys of any width. Returns a DeviceColumn
        of u32 row ids or None (-3/-4: unsupported → host)."""
        nk = len(keyspecs)
        ks = self._keyspec_array(keyspecs)
        if perm_in is not None and perm_in.len != n:
            raise DsxError(f"sort_word: perm_in has {perm_in.len} ids, "
                           f"expected {n}")
        perm = ct.c_void_p()
        rc = self.lib.dsx_sort_word(
            self.ctx, self._cols_array(cols), ct.c_int(len(cols)), ks,
            ct.c_int(nk), ct.c_int64(n),
            ct.c_void_p(perm_in.data) if perm_in is not None else None,
            ct.byref(perm))
        if rc in (-3, -4):
            return None
        _check(self.lib, rc, "dsx_sort_word")
        return DeviceColumn(self, perm.value, None, n, I32, owner=True)

    def window_mark_word(self, cols, keyspecs, n, perm, marks=None):
        """Boundary marks of one order word over sorted positions
        (dsx_window_mark_word): mark[i] = i == 0 or the word's code of row
        perm[i] differs from that of row perm[i-1]. cols / keyspecs as for
        sort_word; perm: DeviceColumn of u32 row ids (None = identity).
        marks=None returns a new u8 DeviceColumn; a given one is ORed into
        and returned. None on -3/-4 (unsupported → host)."""
        nk = len(keyspecs)
        ks = self._keyspec_array(keyspecs)
        for what, col in (("perm", perm), ("marks", marks)):
            if col is not None and col.len != n:
                raise DsxError(f"window_mark_word: {what} has {col.len} "
                               f"entries, expected {n}")
        m = ct.c_void_p(marks.data if marks is not None else None)
        rc = self.lib.dsx_window_mark_word(
            self.ctx, self._cols_array(cols), ct.c_int(len(cols)), ks,
            ct.c_int(nk), ct.c_int64(n),
            ct.c_void_p(perm.data) if perm is not None else None,
            ct.byref(m))
        if rc in (-3, -4):
            return None
        _check(self.lib, rc, "dsx_window_mark_word")
        if marks is not None:
            return marks
        return DeviceColumn(self, m.value, None, n, BOOL8, owner=True)

    def window_seg_ids(self, marks, n):
        """Segment ids of sorted positions from boundary marks
        (dsx_window_seg_ids): ids[i] = marks set in [0, i], minus one — a
        drop-in for the sorted key codes window_ordered / window_rows take.
        Returns (DeviceColumn of n u64 ids, number of segments)."""
        if marks.len != n:
            raise DsxError(f"window_seg_ids: marks has {marks.len} "
                           f"entries, expected {n}")
        ids = ct.c_void_p()
        nseg = ct.c_int64()
        _check(self.lib,
               self.lib.dsx_window_seg_ids(
                   self.ctx, ct.c_void_p(marks.data), ct.c_int64(n),
                   ct.byref(ids), ct.byref(nseg)),
               "dsx_window_seg_ids")
        return (DeviceColumn(self, ids.value, None, n, I64, owner=True),
                nseg.value)

    WIN_FUNCS = {"row_number": 0, "rank": 1, "dense_rank": 2, "lag": 3,
                 "lead": 4, "first_value": 5, "sum": 6, "count": 7,
                 "min": 8, "max": 9, "avg": 10}

    def window_ordered(self, perm, n, pcode_sorted, fcode_sorted, func,
                       v_col, offset, default_bits, has_default, out_dtype,
                       want_valid):
        """Device ordered window frame (dsx_window_ordered)."""
        d = ct.c_void_p()
        vv = ct.c_void_p()
        vstruct = None
        if v_col is not None:
            vstruct = v_col.c_struct()
        _check(
            self.lib,
            self.lib.dsx_window_ordered(
                self.ctx, ct.c_void_p(perm.data), ct.c_int64(n),
                ct.c_void_p(pcode_sorted.data),
                ct.c_void_p(fcode_sorted.data) if fcode_sorted is not None
                else None,
                ct.c_int(self.WIN_FUNCS[func]),
                ct.byref(vstruct) if vstruct is not None else None,
                ct.c_int64(offset), ct.c_int64(default_bits),
                ct.c_int(1 if has_default else 0), ct.c_int(out_dtype),
                ct.byref(d), ct.byref(vv),
                ct.c_int(1 if want_valid else 0)),
            "dsx_window_ordered",
        )
        return DeviceColumn(self, d.value, vv.value or None, n, out_dtype,
                            owner=True)

    # dsx_window_rows func ids: the aggregate ids above + FIRST and LAST
    WIN_ROWS_FUNCS = {"sum": 6, "count": 7, "min": 8, "max": 9, "avg": 10,
                      "first_value": 5, "last_value": 11}

    def window_rows(self, perm, n, pcode_sorted, func, v_col, lo_off, hi_off,
                    out_dtype, want_valid):
        """Device explicit ROWS frame (dsx_window_rows). lo_off / hi_off are
        row offsets relative to the current sorted row (PRECEDING negative),
        None = unbounded side."""
        d = ct.c_void_p()
        vv = ct.c_void_p()
        vstruct = v_col.c_struct() if v_col is not None else None
        _check(
            self.lib,
            self.lib.dsx_window_rows(
                self.ctx, ct.c_void_p(perm.data), ct.c_int64(n),
                ct.c_void_p(pcode_sorted.data),
                ct.c_int(self.WIN_ROWS_FUNCS[func]),
                ct.byref(vstruct) if vstruct is not None else None,
                ct.c_int(1 if lo_off is None else 0),
                ct.c_int64(0 if lo_off is None else lo_off),
                ct.c_int(1 if hi_off is None else 0),
                ct.c_int64(0 if hi_off is None else hi_off),
                ct.c_int(out_dtype), ct.byref(d), ct.byref(vv),
                ct.c_int(1 if want_valid else 0)),
            "dsx_window_rows",
        )
        return DeviceColumn(self, d.value, vv.value or None, n, out_dtype,
                            owner=True)

    def window_range(self, perm, n, pcode_sorted, fcode_sorted, func, v_col,
                     key_col, desc, lo, hi, out_dtype, want_valid):
        """Device RANGE frame with value offsets (dsx_window_range). lo / hi
        are ``(kind, value)`` with kind 0 unbounded, 1 current row, 2 signed
        offset in the order key's unit; key_col (original row order) may be
        None when no bound is an offset. None when the library declines the
        frame (-7: the MIN/MAX table would exceed
        DSX_WIN_RANGE_RMQ_MAX_BYTES)."""
        d = ct.c_void_p()
        vv = ct.c_void_p()
        vstruct = v_col.c_struct() if v_col is not None else None
        kstruct = key_col.c_struct() if key_col is not None else None

        def bound(b):
            kind, value = b
            if kind != 2:
                return _WinBound(kind, 0, 0.0)
            return _WinBound(kind, int(value) if not isinstance(value, float)
                             else 0, float(value))

        blo, bhi = bound(lo), bound(hi)
        rc = self.lib.dsx_window_range(
            self.ctx, ct.c_void_p(perm.data), ct.c_int64(n),
            ct.c_void_p(pcode_sorted.data), ct.c_void_p(fcode_sorted.data),
            ct.c_int(self.WIN_ROWS_FUNCS[func]),
            ct.byref(vstruct) if vstruct is not None else None,
            ct.byref(kstruct) if kstruct is not None else None,
            ct.c_int(1 if desc else 0), ct.byref(blo), ct.byref(bhi),
            ct.c_int(out_dtype), ct.byref(d), ct.byref(vv),
            ct.c_int(1 if want_valid else 0))
        if rc == -7:
            return None
        _check(self.lib, rc, "dsx_window_range")
        return DeviceColumn(self, d.value, vv.value or None, n, out_dtype,
                            owner=True)

    def hash_table_free(self, table):
        self.lib.dsx_hash_table_free(table)

    def hash_groupby(self, cols, n, keyspecs, pred_prog, agg_specs):
        unsafe = self._hist_cache_unsafe(cols, keyspecs)
        if unsafe:
            self.lib.dsx_gb_hist_cache_enable(self.ctx, 0)
        try:
            return self._hash_groupby(cols, n, keyspecs, pred_prog,
                                      agg_specs)
        finally:
            if unsafe:
                self.lib.dsx_gb_hist_cache_enable(self.ctx, 1)

    def _hash_groupby(self, cols, n, keyspecs, pred_prog, agg_specs):
        """keyspecs: list of (col_idx, min, range, nullable) — key pack fused
        in-kernel. agg_specs: list of (agg_op, prog). Returns device pointers
        (out_codes, out_vals [naggs][G], out_counts [naggs][G], n_groups)."""
        ks = self._keyspec_array(keyspecs)
        aggs = self._aggspec_array(agg_specs)
        if pred_prog is not None:
            pparr, pplen = pred_prog
        else:
            pparr, pplen = (_Instr * 1)(), 0
        oc = ct.c_void_p()
        ov = ct.c_void_p()
        on = ct.c_void_p()
        og = ct.c_int64()
        _check(
            self.lib,
            self.lib.dsx_hash_groupby(
                self.ctx, self._cols_array(cols), ct.c_int(len(cols)),
                ct.c_int64(n), ks, ct.c_int(len(keyspecs)), pparr,
                ct.c_int(pplen), aggs, ct.c_int(len(agg_specs)),
                ct.byref(oc), ct.byref(ov), ct.byref(on), ct.byref(og)),
            "dsx_hash_groupby",
        )
        return oc.value, ov.value, on.value, og.value

    # finalize kinds of hash_groupby_cols (DsxGbFinishKind)
    GB_FIN_KINDS = {"count": 0, "sum_i": 1, "sum_f": 2, "min_i": 3,
                    "max_i": 4, "min_f": 5, "max_f": 6, "avg": 7}

    def hash_groupby_cols(self, cols, n, keyspecs, pred_prog, agg_specs,
                          calls):
        """hash_groupby with the output columns finished in the same call
        (dsx_hash_groupby_cols): calls = [(finalize kind name, index into
        agg_specs)]. Returns ([key DeviceColumn], [call DeviceColumn],
        n_groups); the columns own their buffers. Integer keys come back as
        I64 with a validity buffer only when nullable, a float (mode 1) key
        as F64 with one; COUNT as I64 without, every other call with."""
        unsafe = self._hist_cache_unsafe(cols, keyspecs)
        ks = self._keyspec_array(keyspecs)
        aggs = self._aggspec_array(agg_specs)
        fc = (_GbFinishCall * max(len(calls), 1))()
        for i, (kind, agg) in enumerate(calls):
            fc[i].kind = self.GB_FIN_KINDS[kind]
            fc[i].agg = agg
        if pred_prog is not None:
            pparr, pplen = pred_prog
        else:
            pparr, pplen = (_Instr * 1)(), 0
        nout = len(keyspecs) + len(calls)
        datas = (ct.c_void_p * max(nout, 1))()
        valids = (ct.c_void_p * max(nout, 1))()
        og = ct.c_int64()
        if unsafe:
            self.lib.dsx_gb_hist_cache_enable(self.ctx, 0)
        try:
            _check(
                self.lib,
                self.lib.dsx_hash_groupby_cols(
                    self.ctx, self._cols_array(cols), ct.c_int(len(cols)),
                    ct.c_int64(n), ks, ct.c_int(len(keyspecs)), pparr,
                    ct.c_int(pplen), aggs, ct.c_int(len(agg_specs)), fc,
                    ct.c_int(len(calls)), datas, valids, ct.byref(og)),
                "dsx_hash_groupby_cols",
            )
        finally:
            if unsafe:
                self.lib.dsx_gb_hist_cache_enable(self.ctx, 1)
        G = og.value
        out = []
        for i in range(nout):
            if i < len(keyspecs):
                spec = keyspecs[i]
                dtype = F64 if (len(spec) > 4 and spec[4] == 1) else I64
            else:
                dtype = F64 if calls[i - len(keyspecs)][0] in (
                    "sum_f", "min_f", "max_f", "avg") else I64
            out.append(DeviceColumn(self, datas[i], valids[i] or None, G,
                                    dtype, owner=True))
        return out[:len(keyspecs)], out[len(keyspecs):], G

    def filter_probe_groupby(self, table, prog, cols, keyspecs, n, agg_specs,
                             calls, kcols):
        """Group-join (dsx_filter_probe_groupby): filter_probe_cols' sweep
        over the unfiltered probe columns `cols`, grouped by build row
        instead of materialized. agg_specs and calls as for
        hash_groupby_cols, the programs reading `cols`; kcols are the
        build-side sources of the output key columns. Returns ([key
        DeviceColumn], [call DeviceColumn], n_groups) typed as
        hash_groupby_cols types them, rows in build row order, or None when
        the entry declines (duplicate build keys, accumulators too large;
        nothing was allocated)."""
        parr, plen = prog
        ks = self._keyspec_array(keyspecs)
        aggs = self._aggspec_array(agg_specs)
        fc = (_GbFinishCall * max(len(calls), 1))()
        for i, (kind, agg) in enumerate(calls):
            fc[i].kind = self.GB_FIN_KINDS[kind]
            fc[i].agg = agg
        nout = len(kcols) + len(calls)
        datas = (ct.c_void_p * max(nout, 1))()
        valids = (ct.c_void_p * max(nout, 1))()
        og = ct.c_int64()
        rc = self.lib.dsx_filter_probe_groupby(
            self.ctx, table, parr, ct.c_int(plen), self._cols_array(cols),
            ct.c_int(len(cols)), ks, ct.c_int(len(keyspecs)), ct.c_int64(n),
            aggs, ct.c_int(len(agg_specs)), fc, ct.c_int(len(calls)),
            self._cols_array(kcols), ct.c_int(len(kcols)), datas, valids,
            ct.byref(og))
        if rc == NOT_APPLICABLE:
            return None
        _check(self.lib, rc, "dsx_filter_probe_groupby")
        G = og.value
        out = []
        for i in range(nout):
            if i < len(kcols):
                dtype = F64 if kcols[i].dtype in (F64, F32) else I64
            else:
                dtype = F64 if calls[i - len(kcols)][0] in (
                    "sum_f", "min_f", "max_f", "avg") else I64
            out.append(DeviceColumn(self, datas[i], valids[i] or None, G,
                                    dtype, owner=True))
        return out[:len(kcols)], out[len(kcols):], G

    def fprobe_agg_jit_launches(self) -> int:
        """Launches so far of the per-shape generated accumulate kernel of
        filter_probe_groupby; a call that leaves the count unchanged ran the
        interpreter kernel (as fprobe_jit_launches) or had no rows."""
        self.lib.dsx_fprobe_agg_jit_launches.restype = ct.c_int64
        return int(self.lib.dsx_fprobe_agg_jit_launches(self.ctx))

    def partition(self, codes: DeviceColumn, nbuckets, validity_ptr=None):
        """Returns (sel DeviceColumn-like ptr wrapped, offsets np.ndarray)."""
        sel = self.empty_column(codes.len, I32, False)  # u32 indices
        offsets = np.zeros(nbuckets + 1, dtype=np.int64)
        _check(
            self.lib,
            self.lib.dsx_partition(self.ctx, ct.c_void_p(codes.data),
                                   ct.c_void_p(validity_ptr) if validity_ptr else None,
                                   ct.c_int64(codes.len), ct.c_int(nbuckets),
                                   ct.c_void_p(sel.data),
                                   offsets.ctypes.data_as(ct.POINTER(ct.c_int64))),
            "dsx_partition",
        )
        return sel, offsets

    def wrap_sel(self, sel_ptr, count) -> DeviceColumn:
        """Wrap a library-allocated u32 selection vector."""
        return DeviceColumn(self, sel_ptr, None, count, I32, owner=True)
