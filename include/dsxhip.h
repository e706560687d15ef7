/* dsxhip — C ABI of the MI355X-native physical execution layer for dask-sql's
 * hot path.
 *
 * Each entry point cites the reference interface it replaces
 * (paths relative to /root/reference). The reference's own execution layer is
 * pandas/Dask called from dask_sql/physical/; this library is the
 * HIP/CDNA4 (gfx950) replacement for exactly those calls. Host bindings:
 * ctypes (dask_sql_amd/runtime.py); a cgo/JNI/N-API-style stub is shown in
 * INTEGRATION.md.
 *
 * Conventions:
 *  - plain pointers + lengths; no torch/Arrow types in signatures. Device
 *    pointers are HIP device memory on the context's device.
 *  - validity masks are uint8[n] (1 = valid); NULL pointer = all valid.
 *    (Arrow bitmaps are converted at the Python boundary.)
 *  - outputs with data-dependent size are library-allocated (hipMalloc);
 *    release with dsx_free. Fixed-size outputs are caller-allocated.
 *  - return: 0 = OK, <0 = error; dsx_last_error() has the message.
 *  - thread-safety: one DsxCtx per thread/GPU; calls on one ctx serialize on
 *    its HIP stream. Multi-GPU collectives are the host's job (RCCL via
 *    torch.distributed, one process per GPU) — this library is single-device.
 */
#ifndef DSXHIP_H
#define DSXHIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DsxCtx DsxCtx;

/* dtype tags (subset per SURVEY.md §2 "Type mappings" row) */
enum DsxType {
  DSX_I64 = 0,
  DSX_F64 = 1,
  DSX_I32 = 2,    /* also DATE32 (days since epoch) */
  DSX_F32 = 3,
  DSX_I8  = 4,    /* also dictionary codes */
  DSX_BOOL8 = 5,
};

/* expression VM opcodes — the device-compiled form of the reference's Rex
 * operator subset (dask_sql/physical/rex/core/call.py:1047-1156: comparisons,
 * AND/OR/NOT, +,-,*,/, IS [NOT] NULL, CASE-as-select, CAST). Programs are
 * typed postfix; built by dask_sql_amd/physical/rex compiler. */
enum DsxOp {
  DSX_OP_COL = 1,       /* arg0 = column index; pushes typed value+validity  */
  DSX_OP_LIT_F64 = 2,   /* imm = f64 bits                                    */
  DSX_OP_LIT_I64 = 3,   /* imm = i64                                         */
  DSX_OP_LIT_NULL = 4,
  DSX_OP_ADD_F64 = 10, DSX_OP_SUB_F64 = 11, DSX_OP_MUL_F64 = 12, DSX_OP_DIV_F64 = 13,
  DSX_OP_ADD_I64 = 14, DSX_OP_SUB_I64 = 15, DSX_OP_MUL_I64 = 16,
  DSX_OP_DIV_I64 = 17, DSX_OP_MOD_I64 = 18,
  DSX_OP_LT_F64 = 20, DSX_OP_LE_F64 = 21, DSX_OP_GT_F64 = 22, DSX_OP_GE_F64 = 23,
  DSX_OP_EQ_F64 = 24, DSX_OP_NE_F64 = 25,
  DSX_OP_LT_I64 = 30, DSX_OP_LE_I64 = 31, DSX_OP_GT_I64 = 32, DSX_OP_GE_I64 = 33,
  DSX_OP_EQ_I64 = 34, DSX_OP_NE_I64 = 35,
  DSX_OP_AND = 40, DSX_OP_OR = 41, DSX_OP_NOT = 42,   /* SQL 3-valued logic   */
  DSX_OP_IS_NULL = 43, DSX_OP_IS_NOT_NULL = 44,
  DSX_OP_I64_TO_F64 = 50, DSX_OP_F64_TO_I64 = 51,  /* CAST (trunc,
                                                      mappings.py:346-353) */
  DSX_OP_BITS_F64 = 52,  /* reinterpret i64 bits as f64 (float key unpack) */
  DSX_OP_SELECT = 60,   /* (cond, a, b) -> cond ? a : b — CASE WHEN           */
  DSX_OP_NEG_F64 = 61, DSX_OP_NEG_I64 = 62, DSX_OP_SQRT_F64 = 63,
  /* scalar math + date extraction (rex/core/call.py scalar operations) */
  DSX_OP_ABS_I64 = 64, DSX_OP_ABS_F64 = 65,
  DSX_OP_FLOOR_F64 = 66, DSX_OP_CEIL_F64 = 67,
  DSX_OP_RINT_F64 = 68,  /* ties-to-even like numpy round */
  DSX_OP_EXP_F64 = 69, DSX_OP_LN_F64 = 70, DSX_OP_POW_F64 = 71,
  DSX_OP_YEAR = 72, DSX_OP_MONTH = 73, DSX_OP_DAY = 74, /* date32 day-int */
  DSX_OP_FLOORMOD_I64 = 75, /* Python/pandas floor-mod: MOD(-5,3) = 1
                               (reference evaluates operator.mod on pandas,
                               rex/core/call.py:1047-1156) */
  /* trigonometry (rex/core/call.py TrigonometricOperations — da.sin etc.);
     unary ops take/return f64, ATAN2 is binary */
  DSX_OP_SIN_F64 = 76, DSX_OP_COS_F64 = 77, DSX_OP_TAN_F64 = 78,
  DSX_OP_ASIN_F64 = 79, DSX_OP_ACOS_F64 = 80, DSX_OP_ATAN_F64 = 81,
  DSX_OP_ATAN2_F64 = 82,
};

typedef struct DsxInstr {
  int32_t op;       /* DsxOp */
  int32_t arg0;     /* column index for OP_COL */
  int64_t imm;      /* literal bits */
} DsxInstr;

#define DSX_MAX_PROG 120
#define DSX_MAX_COLS 16
#define DSX_MAX_AGGS 16
#define DSX_MAX_KEYS 4

typedef struct DsxColumn {
  void* data;               /* device pointer */
  const uint8_t* validity;  /* device pointer or NULL (all valid) */
  int64_t len;
  int32_t dtype;            /* DsxType */
} DsxColumn;

/* ---- context / memory -------------------------------------------------- */

/* replaces: process/worker setup the reference delegates to dask.distributed
 * (SURVEY.md §5 "Distributed communication backend"). One ctx per GPU. */
int dsx_ctx_create(int device_id, DsxCtx** out);
void dsx_ctx_destroy(DsxCtx* ctx);
const char* dsx_last_error(void);
int dsx_synchronize(DsxCtx* ctx);

int dsx_malloc(DsxCtx* ctx, int64_t bytes, void** out);
int dsx_free(DsxCtx* ctx, void* ptr);
/* replaces the host→worker data movement of dask's task shuffle for table
 * registration (dask_sql/context.py:168 create_table / persist):
 * pinned-host→HBM hipMemcpyAsync. */
int dsx_upload(DsxCtx* ctx, const void* host, int64_t bytes, void** out_dev);
/* host→HBM through a persistent pinned staging arena (chunked, overlapped
 * memcpy + hipMemcpyAsync) — the parquet-ingest fast path (reference reads
 * via dask IO, physical/utils/filter.py:17; here: pyarrow column buffers →
 * pinned → HBM with no pandas round-trip). */
int dsx_upload_pinned(DsxCtx* ctx, const void* host_data, int64_t nbytes,
                      void** out_device_ptr);

int dsx_download(DsxCtx* ctx, const void* dev, void* host, int64_t bytes);
int dsx_memset(DsxCtx* ctx, void* dev, int value, int64_t bytes);
/* device-to-device copy (UNION ALL concatenation — the reference's
 * dd.concat of the union branches) */
int dsx_copy(DsxCtx* ctx, void* dst, const void* src, int64_t bytes);

/* per-kernel HIP-event timing (for bench.py roofline accounting) */
int dsx_prof_enable(DsxCtx* ctx, int enable);
/* fills (name, total_ms, launches) for up to cap kernels; returns count */
int dsx_prof_get(DsxCtx* ctx, char names[][32], double* total_ms,
                 int64_t* launches, int cap);
int dsx_prof_reset(DsxCtx* ctx);

/* ---- scan / expression / filter ---------------------------------------- */

/* replaces Projection `df.assign(RexConverter result)`
 * (dask_sql/physical/rel/logical/project.py:56-65 and rex/core/call.py ops):
 * out = program(cols) per row. out_dtype in {DSX_I64, DSX_F64, DSX_BOOL8}.
 * out_data caller-allocated (n * sizeof), out_validity caller-allocated u8[n]
 * or NULL to discard. */
int dsx_eval(DsxCtx* ctx, const DsxInstr* prog, int prog_len,
             const DsxColumn* cols, int ncols, int64_t n,
             void* out_data, uint8_t* out_validity, int32_t out_dtype);

/* replaces Filter `cond.fillna(False); df[cond]`
 * (dask_sql/physical/rel/logical/filter.py:20-45): evaluates the predicate
 * program, NULL→False, and emits the ORDER-PRESERVING selection vector of
 * matching row ids (library-allocated u32; free with dsx_free). */
int dsx_filter(DsxCtx* ctx, const DsxInstr* prog, int prog_len,
               const DsxColumn* cols, int ncols, int64_t n,
               uint32_t** out_sel, int64_t* out_count);

/* fused filter + materialization: evaluate the predicate and write the
 * selected rows of `mats` directly, order-preserving — `df[cond]`
 * (filter.py:40) in one pass, with no selection vector and no per-column
 * gathers. out_datas/out_valids are caller arrays of nmats slots, filled
 * with pool allocations (free with dsx_free). */
int dsx_filter_cols(DsxCtx* ctx, const DsxInstr* prog, int prog_len,
                    const DsxColumn* cols, int ncols, int64_t n,
                    const DsxColumn* mats, int nmats, void** out_datas,
                    uint8_t** out_valids, int64_t* out_count);

/* boolean-mask take / merge materialization: out[i] = col[sel[i]].
 * out caller-allocated. Gathers validity too when both non-NULL. */
int dsx_gather(DsxCtx* ctx, const DsxColumn* col, const uint32_t* sel,
               int64_t n_sel, void* out_data, uint8_t* out_validity);

/* inverse of dsx_gather: out[sel[i]] = col[i] — places join-back / window
 * columns into original row order (reference window.py:212-428 assigns the
 * computed window column back onto the frame's index). out caller-allocated
 * and pre-initialized (untouched rows keep their init). */
int dsx_scatter_rows(DsxCtx* ctx, const DsxColumn* col, const uint32_t* sel,
                     int64_t n_sel, int64_t n_out, void* out_data,
                     uint8_t* out_validity);

/* min/max of an i64/i32/i8/date32 column ignoring NULLs (key-range probe for
 * packing; also MIN/MAX aggregate support). */
int dsx_minmax_i64(DsxCtx* ctx, const DsxColumn* col, int64_t* out_min,
                   int64_t* out_max, int64_t* out_nonnull);

/* pack up to 4 key columns into one u64 code column:
 * code = Σ_k (col_k - min_k + nullable_k) * stride_k, NULL → 0 slot.
 * Implements composite GROUP BY / join keys; NULL gets its own code, which
 * is what gives groupby(dropna=False) (aggregate.py:575-577) for free.
 * out caller-allocated u64[n]. */
typedef struct DsxKeySpec {
  int32_t col;        /* index into cols */
  int64_t min;        /* from dsx_minmax */
  int64_t range;      /* max-min+1 (+1 more reserved internally if nullable) */
  int32_t nullable;   /* 0/1 */
  int32_t mode;       /* 0 = radix pack; 1 = f64 bit-pattern (must be the
                         ONLY key): code = canonical_bits(x)+1, NaN and NULL
                         share code 0 — pandas groups NaN keys together under
                         dropna=False (aggregate.py:575-577).
                         ORDER BY entries (dsx_sort_perm, dsx_sort_word):
                         bit1 (2) = DESC, bit2 (4) = NULLS LAST, bit3 (8) =
                         float key, a word of its own (dsx_sort_word only) */
} DsxKeySpec;
int dsx_keypack(DsxCtx* ctx, const DsxColumn* cols, int ncols,
                const DsxKeySpec* keys, int nkeys, int64_t n,
                uint64_t* out_codes);

/* ---- hash join ---------------------------------------------------------- */

/* replaces the per-partition pandas hash join inside
 * `dd.merge(on=..., how=...)` (dask_sql/physical/rel/logical/join.py:241-246).
 * Build: open-addressing multimap over u64 key codes (from dsx_keypack, or
 * raw non-negative i64 keys). NULL keys (code with validity 0) are NOT
 * inserted — the NULL-key drop of join.py:202-213 for the build side.
 * Table is library-allocated; free with dsx_hash_table_free. */
typedef struct DsxHashTable DsxHashTable;
/* code_max: max possible key code (0 = unknown). codes below 2^32-1 pack
 * (code,rowid) into one 8-byte slot — one random read per probe. */
int dsx_hash_build(DsxCtx* ctx, const uint64_t* codes, const uint8_t* validity,
                   int64_t n, uint64_t code_max, DsxHashTable** out);
/* dsx_hash_build plus, with key_filter != 0, a key-membership filter over the
 * build keys that dsx_filter_probe_cols consults before (or instead of) the
 * table: mode 1 is an exact bitmap over codes 0..code_max (packed tables whose
 * bitmap fits the byte cap), mode 2 a blocked two-bit Bloom filter, mode 0 no
 * filter. The cap is DSX_JOIN_FILTER_MAX_BYTES (csrc/join_filter.h; the env
 * variable of the same name overrides it per call); DSX_DISABLE_JOINFILTER=1,
 * read per call, builds and reads no filter. */
int dsx_hash_build_filtered(DsxCtx* ctx, const uint64_t* codes,
                            const uint8_t* validity, int64_t n,
                            uint64_t code_max, int key_filter,
                            DsxHashTable** out);
/* The same table built straight from source columns in one sweep: per row the
 * predicate program (prog_len == 0: every row; a row is kept only when the
 * predicate is TRUE), the NULL-key drop over the key columns' validity, the
 * key pack (keys[j].col indexes `cols`; mode 0 only; codes bit-identical to
 * dsx_keypack's) and the insert. The stored row id is the row's index in
 * `cols`, and the table is sized by n (the survivor count is never fetched:
 * the call copies nothing to the host and waits for nothing). It replaces
 * dsx_filter_cols -> dsx_keypack -> (dsx_eval for a nullable key) ->
 * dsx_hash_build_filtered on a build side with a pending WHERE, and
 * dsx_keypack -> dsx_hash_build_filtered on any other. Both build entries
 * combine the exact filter's bits per run of neighbouring lanes before the
 * atomic; DSX_DISABLE_BUILD_RUNCOMBINE=1 (read per call) issues one per row. */
int dsx_hash_build_cols(DsxCtx* ctx, const DsxInstr* prog, int prog_len,
                        const DsxColumn* cols, int ncols,
                        const DsxKeySpec* keys, int nkeys, int64_t n,
                        uint64_t code_max, int key_filter,
                        DsxHashTable** out);
int dsx_hash_table_filter_mode(const DsxHashTable* t);
int64_t dsx_hash_table_filter_bytes(const DsxHashTable* t);
/* filtered builds (key_filter != 0) on ctx so far that ended in `mode` */
int64_t dsx_join_filter_builds(DsxCtx* ctx, int mode);
void dsx_hash_table_free(DsxHashTable* t);

enum DsxJoinType {  /* reference join.py:41-48 JOIN_TYPE_MAPPING */
  DSX_JOIN_INNER = 0,
  DSX_JOIN_LEFT = 1,       /* left outer: unmatched probe → rhs NULL */
  DSX_JOIN_LEFTSEMI = 2,
  DSX_JOIN_LEFTANTI = 3,
};
#define DSX_NULL_IDX 0xFFFFFFFFu

/* Probe: emits (probe_rowid, build_rowid) pairs, library-allocated.
 * Unordered (normalize by sort for comparisons); FULL OUTER is composed by
 * the host from LEFT + unmatched-build sweep (dsx_hash_unmatched). */
/* mark_matched: record matched build slots (needed only when
 * dsx_hash_unmatched will run, i.e. FULL OUTER). The marks (slots x 4 B) are
 * allocated and cleared by the first mark_matched probe or
 * dsx_hash_unmatched on the table, not by the build; dsx_hash_unmatched on a
 * table never probed that way reports every build row. */
int dsx_hash_probe(DsxCtx* ctx, DsxHashTable* t, const uint64_t* codes,
                   const uint8_t* validity, int64_t n, int join_type,
                   int mark_matched,
                   uint32_t** out_probe_idx, uint32_t** out_build_idx,
                   int64_t* out_count);
/* build rows never matched by any probe since build (for FULL OUTER,
 * join.py JOIN_TYPE_MAPPING "FULL" → outer). */
/* fused probe-emit + materialization (INNER/LEFT/SEMI/ANTI, no residual):
 * the emit pass writes the join's output columns directly — one pass, no
 * (probe,build) pair vectors and no per-column gathers (the fusion of
 * join.py:241-246 dd.merge's column copy). out_datas/out_valids are caller
 * arrays of n_pcols+n_bcols slots, filled with pool allocations (free with
 * dsx_free); out_valids[i] NULL when the source has no validity and no
 * LEFT NULL-fill applies. */
int dsx_hash_probe_cols(DsxCtx* ctx, DsxHashTable* t, const uint64_t* codes,
                        const uint8_t* validity, int64_t n, int join_type,
                        const DsxColumn* pcols, int n_pcols,
                        const DsxColumn* bcols, int n_bcols,
                        int force_build_validity, void** out_datas,
                        uint8_t** out_valids, int64_t* out_count);

/* fused scan filter + key pack + probe + materialization for INNER joins
 * whose build keys are unique (PK-FK): the composition of dsx_filter_cols,
 * dsx_keypack and dsx_hash_probe_cols over the UNFILTERED probe-side columns,
 * without the compacted columns, the code column or the slot cache in
 * between (filter.py:20-45 + join.py:241-246 in one sweep). `cols` serves
 * both the predicate program (NULL→False) and the key specs (keys[j].col
 * indexes it; mode 0 only; codes are bit-identical to dsx_keypack's; a row
 * with a NULL key column never matches). Output rows are in increasing probe
 * row order; out_datas/out_valids as for dsx_hash_probe_cols.
 * Returns DSX_NOT_APPLICABLE, with nothing allocated, when the table holds a
 * duplicate build key — the caller then filters and probes separately. */
#define DSX_NOT_APPLICABLE 1
int dsx_filter_probe_cols(DsxCtx* ctx, DsxHashTable* t, const DsxInstr* prog,
                          int prog_len, const DsxColumn* cols, int ncols,
                          const DsxKeySpec* keys, int nkeys, int64_t n,
                          const DsxColumn* pcols, int n_pcols,
                          const DsxColumn* bcols, int n_bcols,
                          void** out_datas, uint8_t** out_valids,
                          int64_t* out_count);

/* The mask pass of dsx_filter_probe_cols runs a kernel generated per query
 * shape (hipRTC; predicate, key pack and table layout inlined, a word's
 * column loads in flight together) and falls
 * back to the interpreter kernel when DSX_DISABLE_JIT or
 * DSX_DISABLE_JIT_FPROBE=1 is set (the latter is read on every call), the
 * generator rejects the predicate, or hipRTC fails. Both fill the same mask.
 * This counts the launches of the generated kernel on `ctx` so far. */
int64_t dsx_fprobe_jit_launches(DsxCtx* ctx);

int dsx_hash_unmatched(DsxCtx* ctx, DsxHashTable* t, uint32_t** out_build_idx,
                       int64_t* out_count);

/* Radix-partitioned equijoin (INNER/LEFT/LEFTANTI): both sides hash-
 * partitioned into bucket-major records, per-bucket LDS build+probe, fused
 * column emit. Replaces dd.merge's per-partition hash join
 * (dask_sql/physical/rel/logical/join.py:241-246) at sizes where the flat
 * probe table spills the XCD L2. keys_b/keys_p: per-key specs (col index
 * into the side's column array; min/range/nullable MUST match pairwise).
 * bpred: build-side row predicate (e.g. key IS NOT NULL). out_side[i]:
 * 0 = probe column, 1 = build column; out_col[i]: column index in that
 * side's array; out_need_valid[i]: allocate a validity mask for output i.
 * Returns -6 on bucket overflow (key skew) — caller falls back to the
 * flat-table join. */
int dsx_radix_join(DsxCtx* ctx, const DsxColumn* build_cols, int n_build_cols,
                   int64_t n_build, const DsxKeySpec* keys_b,
                   const DsxKeySpec* keys_p, int nkeys,
                   const DsxInstr* bpred, int bpred_len,
                   const DsxColumn* probe_cols, int n_probe_cols,
                   int64_t n_probe, int join_type, const int32_t* out_side,
                   const int32_t* out_col, const int32_t* out_need_valid,
                   int n_out, void** out_datas, uint8_t** out_valids,
                   int64_t* out_count);

/* Device general sort for ORDER BY without LIMIT (reference
 * physical/utils/sort.py:9-60): order-preserving packed codes (DsxKeySpec
 * mode bit1 = DESC, bit2 = NULLS LAST; caller passes keys REVERSED so the
 * first ORDER BY key takes the highest stride) → range partition →
 * per-bucket LDS bitonic (stable via rowid tiebreak). Returns the sorted
 * row permutation; -6 on skew (caller sorts on host). */
int dsx_sort_perm(DsxCtx* ctx, const DsxColumn* cols, int ncols,
                  const DsxKeySpec* keys, int nkeys, int64_t n,
                  uint32_t** out_perm);

/* Stable LSD radix sort of a row-id sequence by ONE 64-bit order "word"
 * (reference physical/utils/sort.py:36-60 — `df.sort_values(kind=
 * "mergesort")` applied key by key from the last ORDER BY key to the
 * first). Sorts perm_in[0..n) (NULL = identity 0..n-1) stably by the word
 * code of the row each entry names and returns the new permutation
 * (library-allocated u32[n]; free with dsx_free). Stability makes a
 * composite key of any width a chain of calls, least significant word
 * first, each call taking the previous result as perm_in. A word is
 *  - up to DSX_MAX_KEYS integer-kind keys, packed exactly as dsx_sort_perm
 *    packs them (mode bit1 = DESC, bit2 = NULLS LAST, keys REVERSED, key
 *    space <= 2^62 else -4), or
 *  - ONE float key (F64 or F32 column), DsxKeySpec mode bit3 (value 8),
 *    optionally with bits 1 and 2; min/range/nullable are ignored. Its code
 *    is the inline function of csrc/sort_code.h: NULL and NaN share the null
 *    slot on the na_position side, -0.0 ties with +0.0.
 * `cols` holds only the word's own key columns (keys[j].col indexes it), so
 * the table's width does not matter. Digits (bytes) of the code that are
 * constant across all rows are skipped. Never returns -6: no input
 * distribution overloads it. -3 on a malformed spec or n > 0xFFFFFFFE. On
 * failure nothing stays allocated and *out_perm is NULL. DSX_RSORT_GRID=<g>
 * (read per call) caps the launch grid — test knob. */
int dsx_sort_word(DsxCtx* ctx, const DsxColumn* cols, int ncols,
                  const DsxKeySpec* keys, int nkeys, int64_t n,
                  const uint32_t* perm_in /* nullable = identity */,
                  uint32_t** out_perm);

/* Candidate rows of ORDER BY ... LIMIT k, selected on the device and brought
 * to the host with one wait (reference physical/utils/sort.py:9-34 topk_sort:
 * nsmallest / nlargest on the first key, then the full sort of what is left).
 * cols: 1..DSX_MAX_COLS fixed-width columns (I8/I32/I64/F32/F64, with or
 * without validity) of n rows; cols[key_col] is the PRIMARY sort key (I8/I32/
 * I64/F64), desc its direction. The candidates are exactly the rows whose
 * primary key sorts at or before the k-th row's primary key — the k-th order
 * statistic with all its ties (-0.0 ties with +0.0) — in no particular order.
 * An MSB-first radix select over the key's order code (csrc/topk_select.h)
 * finds them; every launch is queued without a host wait, and ONE D2H copy
 * into a pinned buffer owned by the context plus one stream synchronize
 * return the result:
 *   *out_host: the buffer, valid until the next dsx_topk_rows on ctx;
 *   out_offsets[1 + 2*ncols] (caller array), byte offsets into it:
 *     [0] row ids u32[count]; [1+2i] column i's values (its dtype)[count];
 *     [2+2i] column i's validity bytes u8[count], -1 when cols[i] has none;
 *   *out_count: k <= count <= cap.
 * Returns DSX_NOT_APPLICABLE (nothing to read) when the primary key holds a
 * NULL or a NaN, or when the candidates do not fit `cap` (ties across the
 * k-th position): the caller orders such frames another way. -3 on a
 * malformed call (n or k out of range, n > 0xFFFFFFFE, dtype). At most
 * 2 * DSX_TOPK_PASSES + 1 kernel launches and one memset; device work space
 * is the context's scratch arena. */
int dsx_topk_rows(DsxCtx* ctx, const DsxColumn* cols, int ncols, int key_col,
                  int desc, int64_t n, int64_t k, int64_t cap,
                  const void** out_host, int64_t* out_offsets,
                  int64_t* out_count);

/* Device ordered window frames (reference rel/logical/window.py:212-428):
 * caller provides the sort permutation over (partition, order) keys and the
 * partition / partition+order codes gathered into sorted order; computes
 * ROW_NUMBER/RANK/DENSE_RANK/LAG/LEAD/FIRST_VALUE and the running
 * SUM/COUNT/MIN/MAX (RANGE UNBOUNDED..CURRENT with peer broadcast),
 * scattered back to original row order. func = DsxWinFunc (0..9). */
int dsx_window_ordered(DsxCtx* ctx, const uint32_t* perm, int64_t n,
                       const uint64_t* pcode_sorted,
                       const uint64_t* fcode_sorted, int func,
                       const DsxColumn* value_or_null, int64_t offset,
                       int64_t default_bits, int has_default, int out_dtype,
                       void** out_data, uint8_t** out_valid, int want_valid);

/* Width thresholds of the ROWS-frame paths below (starting values, not
 * tuned): a bounded frame of W = hi_off - lo_off + 1 rows is reduced
 * directly out of an LDS tile when W <= DIRECT_MAXW (SUM/COUNT/AVG) or
 * W <= TILE_MAXW (MIN/MAX). dsx_window_rows_limits reports them to the
 * caller that picks the strategy. */
#define DSX_WIN_ROWS_DIRECT_MAXW 64
#define DSX_WIN_ROWS_TILE_MAXW 1024
int dsx_window_rows_limits(int* direct_maxw, int* tile_maxw);

/* Device explicit ROWS frames (reference rel/logical/window.py:145-198 —
 * map_on_each_group's expanding / rolling / BaseIndexer chain per sorted
 * partition). Same inputs as dsx_window_ordered minus the peer codes. The
 * frame of sorted row i in partition [p0, p1) is [max(p0, i + lo_off),
 * min(p1 - 1, i + hi_off)], a side dropping its offset when unbounded;
 * PRECEDING offsets are negative, CURRENT ROW is 0. An EMPTY frame yields
 * NULL for every function, COUNT included. func = DsxWinFunc SUM/COUNT/MIN/
 * MAX/AVG (6..10), FIRST_VALUE (5) or LAST_VALUE (11):
 *  - bounded frames up to the widths above: one LDS tile pass
 *    (k_win_rows_tile);
 *  - wider SUM/COUNT/AVG and any unbounded side: three-phase per-partition
 *    scan (k_win_segscan_tile/_carry/_apply; reverse for MIN/MAX with only
 *    the high side unbounded) + k_win_rows_prefix;
 *  - FIRST/LAST: positional bit copy in the value dtype (out_dtype must
 *    equal it), NULL when the boundary row is NULL;
 *  - bounded MIN/MAX wider than DSX_WIN_ROWS_TILE_MAXW: returns -7, the
 *    caller keeps those on the host.
 * Aggregates accumulate in f64 and write out_dtype I64 or F64 (COUNT(*) =
 * value_or_null NULL). Results land in original row order. On failure
 * nothing stays allocated and *out_data / *out_valid are NULL. */
int dsx_window_rows(DsxCtx* ctx, const uint32_t* perm, int64_t n,
                    const uint64_t* pcode_sorted, int func,
                    const DsxColumn* value_or_null, int lo_unbounded,
                    int64_t lo_off, int hi_unbounded, int64_t hi_off,
                    int out_dtype, void** out_data, uint8_t** out_valid,
                    int want_valid);

/* One bound of a RANGE frame: the partition edge, the edge of the current
 * row's peer group, or a signed offset in the order key's unit (PRECEDING
 * negative) — ival for integer, date and timestamp keys, fval for float
 * keys. */
enum DsxWinBoundKind {
  DSX_WIN_BOUND_UNBOUNDED = 0,
  DSX_WIN_BOUND_CURRENT = 1,
  DSX_WIN_BOUND_OFFSET = 2,
};
typedef struct DsxWinBound {
  int32_t kind; /* DsxWinBoundKind */
  int64_t ival;
  double fval;
} DsxWinBound;

/* Device RANGE frames with value offsets (SQL standard semantics, as sqlite
 * computes them). Inputs follow dsx_window_rows, plus the sorted peer codes
 * (partition + order keys; adjacent values differ exactly at a peer-group
 * boundary), the order-key column in ORIGINAL row order (I64/I32/I8 or
 * F64/F32; may be NULL when no bound is an OFFSET), its direction, and the
 * two bounds. With d = +1 (ASC) / -1 (DESC), a row of non-NULL key k frames
 * the non-NULL-key rows j of its partition with lo <= d * (key[j] - k) <=
 * hi; k + offset saturates at the int64 limits (a target whose exact
 * value lies beyond the limit no key can reach admits no row, also not a
 * key AT the limit); NaN keys count as NULL. A
 * NULL-key row's offset side ends at the edge of its peer group (the NULL
 * block). CURRENT is the peer group's first / last row, UNBOUNDED the
 * partition edge. An EMPTY frame is NULL for every function except COUNT,
 * which is 0. func as for dsx_window_rows:
 *  - SUM/COUNT/AVG: forward per-partition scan + prefix difference;
 *  - MIN/MAX with an unbounded side: forward / reverse scan lookup;
 *  - MIN/MAX with both sides bounded: a sparse table over 64-row blocks
 *    (8 * ceil(n / 64) * levels bytes from the pool, levels =
 *    floor(log2(blocks)) + 1). Above DSX_WIN_RANGE_RMQ_MAX_BYTES
 *    (environment, read per call, default 1 GiB) the call returns -7 and
 *    the caller keeps the frame on the host;
 *  - FIRST/LAST: positional bit copy in the value dtype.
 * n <= 2^32 - 1. Results land in original row order. On failure nothing
 * stays allocated and *out_data / *out_valid are NULL. */
int dsx_window_range(DsxCtx* ctx, const uint32_t* perm, int64_t n,
                     const uint64_t* pcode_sorted,
                     const uint64_t* fcode_sorted, int func,
                     const DsxColumn* value_or_null,
                     const DsxColumn* key_or_null, int desc,
                     const DsxWinBound* lo, const DsxWinBound* hi,
                     int out_dtype, void** out_data, uint8_t** out_valid,
                     int want_valid);

/* Boundary marks of ONE order word over a sorted row sequence — the window
 * front half for keys that do not pack into one code (float keys, more than
 * DSX_MAX_KEYS keys, key spaces above 2^62; reference rel/logical/
 * window.py:212-428 groups the sorted frame with groupby(dropna=False)).
 * The word is specified and validated exactly as dsx_sort_word takes it
 * (same -3 / -4 answers, same code: pack_key or csrc/sort_code.h, so NULL
 * and NaN share a slot and -0.0 ties with +0.0). For sorted position i,
 *   mark[i] = (i == 0) || code(perm[i]) != code(perm[i-1])
 * with perm NULL = identity. *marks_inout NULL: the library allocates u8[n]
 * (free with dsx_free) and writes the marks; otherwise the marks are ORed
 * into the given buffer, so the boundaries of a multi-word key are the OR
 * over its words. n == 0 is legal. On failure nothing stays allocated and
 * *marks_inout is NULL (a buffer the caller passed in stays the caller's).
 * DSX_RSORT_GRID caps the launch grid as for dsx_sort_word. */
int dsx_window_mark_word(DsxCtx* ctx, const DsxColumn* cols, int ncols,
                         const DsxKeySpec* keys, int nkeys, int64_t n,
                         const uint32_t* perm /* nullable = identity */,
                         uint8_t** marks_inout);

/* Segment ids from boundary marks: ids[i] = (number of non-zero marks in
 * [0, i]) - 1, library-allocated u64[n] (free with dsx_free) — adjacent
 * values differ exactly at a mark, so the ids serve as pcode_sorted /
 * fcode_sorted of dsx_window_ordered and dsx_window_rows. *out_segments
 * (nullable) receives the number of marks. Three bounded phases (per-block
 * counts, one-block scan, apply); no block waits on another. n == 0 is
 * legal. On failure nothing stays allocated and *out_ids is NULL.
 * DSX_RSORT_GRID caps the launch grid. */
int dsx_window_seg_ids(DsxCtx* ctx, const uint8_t* marks, int64_t n,
                       uint64_t** out_ids, int64_t* out_segments);

/* ---- hash groupby-aggregate --------------------------------------------- */

enum DsxAggOp {  /* reference AGGREGATION_MAPPING aggregate.py:117-231 subset:
                    sum (custom_sum min_count=1, :486-493), count, min, max;
                    avg finalized on host as sum/count. */
  DSX_AGG_SUM_F64 = 0,
  DSX_AGG_SUM_I64 = 1,
  DSX_AGG_COUNT = 2,     /* counts rows where input program is non-NULL */
  DSX_AGG_MIN_F64 = 3,
  DSX_AGG_MAX_F64 = 4,
  DSX_AGG_MIN_I64 = 5,
  DSX_AGG_MAX_I64 = 6,
};

typedef struct DsxAggSpec {
  int32_t op;                    /* DsxAggOp */
  int32_t prog_len;
  DsxInstr prog[DSX_MAX_PROG];   /* input expression, fused into the kernel */
} DsxAggSpec;

/* Toggle the per-table groupby histogram cache; the Python layer turns it
 * off for externally-backed (e.g. torch/RCCL staging) key columns. */
int dsx_gb_hist_cache_enable(DsxCtx* ctx, int enable);

/* replaces `df.groupby(by, dropna=False).agg(...)`
 * (dask_sql/physical/rel/logical/aggregate.py:575-581) with the WHERE
 * predicate fused in (filter.py:20-45 fused into the same scan — SURVEY §3
 * call stack (2)+(4)) and the key pack fused in (one fused scan kernel).
 *
 * keys: nkeys DsxKeySpec (ranges from dsx_minmax); the packed key space
 *       (Π(range+nullable)) must be ≤ 2^62. nkeys 0 = full-table aggregate.
 *       key_space ≤ LDS budget → per-CU LDS direct-indexed accumulation;
 *       else global CAS-claim table (SURVEY §7 step 4 two-level design).
 * pred: optional predicate program (NULL→False), pred_len 0 = no predicate.
 * Outputs (library-allocated, compacted, one row per non-empty group):
 *   out_codes u64[G], out_vals = one buffer laid out [naggs][G] (f64/i64 per
 *   agg op), out_counts = one buffer [naggs][G] of non-NULL input counts
 *   (for SUM NULL semantics and COUNT), G = *out_groups.
 *   For DSX_AGG_SUM_*: value is the sum over non-NULL inputs; nonnull count 0
 *   ⇒ SQL NULL (custom_sum min_count=1) — host finalizes.
 *   For MIN/MAX: same. For COUNT: value array unused, count is the result. */
int dsx_hash_groupby(DsxCtx* ctx,
                     const DsxColumn* cols, int ncols, int64_t n,
                     const DsxKeySpec* keys, int nkeys,
                     const DsxInstr* pred, int pred_len,
                     const DsxAggSpec* aggs, int naggs,
                     uint64_t** out_codes, void** out_vals /*[naggs][G]*/,
                     uint64_t** out_counts /*[naggs][G]*/, int64_t* out_groups);

/* dsx_hash_groupby plus the finish of its output columns in the same call:
 * the group keys unpacked from the packed code and every aggregate call
 * finalized, all written by ONE kernel launch once G is known (the reference
 * does this step on the grouped frame, aggregate.py:575-581 reset_index and
 * the per-call finalizers). Same three paths and fallbacks as
 * dsx_hash_groupby.
 *
 * Keys come back in `keys` order: mode 0 as i64 = (code / stride) % space
 * (− 1 when nullable, slot 0 = NULL) + min, with a validity buffer only when
 * the key is nullable; mode 1 as f64 = bitcast(code − 1), code 0 = NULL (cell
 * holds NaN), always with a validity buffer.
 * Calls: `agg` indexes `aggs` (one accumulator per call; the library maps it
 * to the partition path's value slot, which skips COUNT accumulators).
 * COUNT is i64 with no validity buffer. Every other kind has one and is NULL
 * when the non-NULL input count is 0 (f64 cells then hold NaN, i64 cells 0):
 * SUM_I/MIN_I/MAX_I are i64, SUM_F/MIN_F/MAX_F f64, AVG f64 = sum / count
 * over a DSX_AGG_SUM_F64 accumulator.
 * out_datas/out_valids: caller arrays of nkeys + ncalls slots (keys first),
 * filled with pool allocations (free with dsx_free); out_valids[i] is NULL
 * where no validity buffer is due. nkeys must be ≥ 1. The call returns with
 * the finish kernel queued on the context's stream, not completed. */
enum DsxGbFinishKind {
  DSX_GB_FIN_COUNT = 0,
  DSX_GB_FIN_SUM_I = 1,
  DSX_GB_FIN_SUM_F = 2,
  DSX_GB_FIN_MIN_I = 3,
  DSX_GB_FIN_MAX_I = 4,
  DSX_GB_FIN_MIN_F = 5,
  DSX_GB_FIN_MAX_F = 6,
  DSX_GB_FIN_AVG = 7,
};
typedef struct DsxGbFinishCall {
  int32_t kind;  /* DsxGbFinishKind */
  int32_t agg;   /* index into aggs */
} DsxGbFinishCall;
int dsx_hash_groupby_cols(DsxCtx* ctx,
                          const DsxColumn* cols, int ncols, int64_t n,
                          const DsxKeySpec* keys, int nkeys,
                          const DsxInstr* pred, int pred_len,
                          const DsxAggSpec* aggs, int naggs,
                          const DsxGbFinishCall* calls, int ncalls,
                          void** out_datas, uint8_t** out_valids,
                          int64_t* out_groups);

/* Group-join: the inner PK-FK join of dsx_filter_probe_cols grouped by the
 * build key (plus other columns of the build side), without materializing the
 * join rows. Build keys are unique on this path, so a matched probe row's
 * group is its build row: the sweep accumulates the aggregates per build row
 * and the finish writes one output row per build row that matched, in
 * ascending build row order (csrc/group_join.inc).
 *  - t, prog, cols, keys, n: as for dsx_filter_probe_cols.
 *  - aggs, calls: as for dsx_hash_groupby_cols; the aggregate programs read
 *    `cols` (the probe side) at the matched probe row.
 *  - kcols: 1..DSX_MAX_KEYS build-side columns (len = the table's build rows),
 *    gathered at the build row as the output key columns. Integer kinds come
 *    back as i64 and float kinds as f64, as dsx_hash_groupby_cols returns its
 *    keys, with a validity buffer iff the source has one.
 * out_datas/out_valids: n_kcols + ncalls slots (keys first), pool allocations
 * sized for every build row; *out_groups rows of each are written. One host
 * wait per call.
 * Returns DSX_NOT_APPLICABLE, with nothing allocated, when the table holds a
 * duplicate build key or the accumulators (build rows x 8..264 bytes) exceed
 * 4 GiB — the caller then joins and groups separately. */
int dsx_filter_probe_groupby(DsxCtx* ctx, DsxHashTable* t,
                             const DsxInstr* prog, int prog_len,
                             const DsxColumn* cols, int ncols,
                             const DsxKeySpec* keys, int nkeys, int64_t n,
                             const DsxAggSpec* aggs, int naggs,
                             const DsxGbFinishCall* calls, int ncalls,
                             const DsxColumn* kcols, int n_kcols,
                             void** out_datas, uint8_t** out_valids,
                             int64_t* out_groups);
/* The accumulate pass of dsx_filter_probe_groupby runs a kernel generated per
 * query shape (hipRTC; key pack, aggregate expressions and record layout
 * inlined) and falls back to the interpreter kernel under DSX_DISABLE_JIT,
 * DSX_DISABLE_JIT_FPROBE=1 (read per call), or a hipRTC failure. Launches of
 * the generated kernel on ctx so far: */
int64_t dsx_fprobe_agg_jit_launches(DsxCtx* ctx);

/* ---- shuffle support --------------------------------------- */

/* replaces dask's hash-repartition "tasks" shuffle split
 * (dask_sql/__init__.py:16, conftest.py:17; inside dd.merge/groupby):
 * bucket rows by mix64(code) % nbuckets, stable within bucket. Emits the
 * per-bucket-contiguous ORDERED selection vector into caller-allocated
 * out_sel u32[n] and bucket row offsets into out_offsets i64[nbuckets+1].
 * The host gathers each bucket's columns into torch-allocated staging
 * buffers and exchanges them with torch.distributed all_to_all (RCCL/xGMI). */
int dsx_partition(DsxCtx* ctx, const uint64_t* codes, const uint8_t* validity,
                  int64_t n, int nbuckets, uint32_t* out_sel,
                  int64_t* out_offsets);

/* TEST INFRASTRUCTURE: emit the hipRTC expression-evaluator source the
 * JIT generates for `prog` (host-only, no GPU) so CPU tests can compile it
 * with gcc and differential-test codegen semantics. Returns 1 when the
 * expression kind is double, 0 for i64, <0 on error. */
int dsx_jit_expr_source(const DsxInstr* prog, int prog_len,
                        const int32_t* dtypes, const uint8_t* has_validity,
                        int ncols, char* buf, int64_t cap);

/* TEST INFRASTRUCTURE: emit the JIT key-pack source for a key spec
 * (host-only, no GPU) for the CPU pack-semantics differential tests. */
int dsx_jit_pack_source(const DsxKeySpec* keys, int nkeys,
                        const int32_t* dtypes, const uint8_t* has_validity,
                        int ncols, char* buf, int64_t cap);

/* TEST INFRASTRUCTURE: the full source of the generated filter-probe mask
 * kernel for a shape (host-only, no GPU). has_validity gives only the
 * PRESENCE of validity buffers; pointers, n and the table mask are kernel
 * arguments and never enter the text. packed: table layout; words: 64-row
 * words per wave iteration (1..8, <= 0 for the shipped value). Returns 0;
 * -1 when the generator rejects the predicate (callers fall back to the
 * interpreter kernel), -2 when buf is too small, -3 on a malformed spec. */
int dsx_jit_fprobe_source_mode(const DsxInstr* prog, int prog_len,
                               const DsxKeySpec* keys, int nkeys,
                               const int32_t* dtypes,
                               const uint8_t* has_validity, int ncols,
                               int packed, int words, int jf_mode, char* buf,
                               int64_t cap);  /* jf_mode 0: the entry below */
int dsx_jit_fprobe_source(const DsxInstr* prog, int prog_len,
                          const DsxKeySpec* keys, int nkeys,
                          const int32_t* dtypes, const uint8_t* has_validity,
                          int ncols, int packed, int words, char* buf,
                          int64_t cap);

/* TEST INFRASTRUCTURE: hipRTC-compile `src` for gfx950 with the runtime's
 * options; needs no GPU. Returns 0, or 1 with the log on stderr. */
int dsx_jit_compile_check(const char* src);

/* TEST INFRASTRUCTURE: compile-check the generated filter-probe kernel for
 * representative shapes at every unroll factor; 0 on success. */
int dsx_jit_fprobe_selftest(void);

/* TEST INFRASTRUCTURE: compile-check the generated accumulate kernel of
 * dsx_filter_probe_groupby for two shapes; needs no GPU; 0 on success. */
int dsx_jit_fprobe_agg_selftest(void);

#ifdef __cplusplus
}
#endif
#endif /* DSXHIP_H */
