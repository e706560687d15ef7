// window_range.inc — device RANGE frames with value offsets
// (dsx_window_range). Included by dsxhip.hip after window_rows.inc, whose
// value staging, segmented scans and emit it shares unchanged.
//
// A bound is UNBOUNDED (partition edge), CURRENT (peer-group edge) or an
// OFFSET in the order key's unit. For sorted row i the frame [s, e] is found
// by search, not by position:
//   k_win_range_key     order key gathered into sorted space (i64 or f64)
//                       with a NULL byte (NaN counts as NULL)
//   k_win_range_bounds  s[i], e[i] (u32, inclusive; empty = 1, 0): partition
//                       and peer group by win_bsearch over the two starts
//                       arrays, the partition's non-NULL rows from the NULL
//                       bytes, an offset bound by lower/upper binary search
//                       over the staged key (csrc/win_range.h)
//   k_win_rmq_blocks    level 0 of the MIN/MAX sparse table: every 64 sorted
//                       rows reduced by one wave with shuffles
//   k_win_rmq_level     level j from level j - 1, one launch per level
//   k_win_range_apply   the result: prefix difference of the forward scans
//                       (SUM/COUNT/AVG), scan lookups (half-unbounded
//                       MIN/MAX), loose rows + two table entries (bounded
//                       MIN/MAX), or the positional FIRST/LAST copy
// An EMPTY frame is NULL for every function except COUNT, which is 0.
// Frames never cross a partition, so the table carries no partition marks.

#include "win_range.h"

enum { WIN_RANGE_MM_NONE = 0, WIN_RANGE_MM_FWD = 1, WIN_RANGE_MM_REV = 2,
       WIN_RANGE_MM_RMQ = 3 };

__global__ void k_win_range_key(const uint32_t* perm, int64_t n, DsxColumn k,
                                int is_f64, void* key_out, uint8_t* knull) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < n; i += stride) {
    int64_t r = (int64_t)perm[i];
    bool valid = !k.validity || k.validity[r];
    if (is_f64) {
      double x = k.dtype == DSX_F64 ? ((const double*)k.data)[r]
                                    : (double)((const float*)k.data)[r];
      if (x != x) valid = false;
      ((double*)key_out)[i] = valid ? x : 0.0;
    } else {
      int64_t x;
      switch (k.dtype) {
        case DSX_I64: x = ((const int64_t*)k.data)[r]; break;
        case DSX_I32: x = (int64_t)((const int32_t*)k.data)[r]; break;
        default: x = (int64_t)((const int8_t*)k.data)[r];
      }
      ((int64_t*)key_out)[i] = valid ? x : 0;
    }
    knull[i] = valid ? 0 : 1;
  }
}

struct WinRangeBounds {
  int lo_kind, hi_kind;  // DSX_WIN_BOUND_*
  int64_t lo_i, hi_i;    // signed offsets, integer keys
  double lo_f, hi_f;     // signed offsets, float keys
};

// [a, b): the rows of partition [p0, p1) whose key is not NULL. The NULL
// rows are one block at the partition's head (NULLS FIRST) or tail, so the
// NULL byte is monotone over the partition either way. The caller's row is
// not NULL, so the range is not empty.
__device__ __forceinline__ void win_range_nonnull(const uint8_t* knull,
                                                  int64_t p0, int64_t p1,
                                                  int64_t* a, int64_t* b) {
  bool head_null = knull[p0] != 0;
  int64_t lo = p0, hi = p1;  // first row whose NULL byte differs from p0's
  while (lo < hi) {
    int64_t mid = lo + ((hi - lo) >> 1);
    if ((knull[mid] != 0) == head_null) lo = mid + 1;
    else hi = mid;
  }
  if (head_null) {
    *a = lo;
    *b = p1;
  } else {
    *a = p0;
    *b = lo;
  }
}

__global__ void k_win_range_bounds(int64_t n, const uint32_t* starts_p,
                                   int64_t np_, const uint32_t* starts_f,
                                   int64_t nf, const void* key,
                                   const uint8_t* knull, int is_f64, int desc,
                                   WinRangeBounds bd, uint32_t* s_out,
                                   uint32_t* e_out) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  bool any_off = bd.lo_kind == DSX_WIN_BOUND_OFFSET ||
                 bd.hi_kind == DSX_WIN_BOUND_OFFSET;
  for (; i < n; i += stride) {
    int64_t sp = win_bsearch(starts_p, np_, i);
    int64_t p0 = (int64_t)starts_p[sp];
    int64_t p1 = sp + 1 < np_ ? (int64_t)starts_p[sp + 1] : n;
    int64_t sf = win_bsearch(starts_f, nf, i);
    int64_t f0 = (int64_t)starts_f[sf];
    int64_t f1 = sf + 1 < nf ? (int64_t)starts_f[sf + 1] : n;
    // CURRENT ROW, and an offset bound of a NULL-key row: the peer group
    int64_t s = bd.lo_kind == DSX_WIN_BOUND_UNBOUNDED ? p0 : f0;
    int64_t e = bd.hi_kind == DSX_WIN_BOUND_UNBOUNDED ? p1 - 1 : f1 - 1;
    if (any_off && !knull[i]) {
      int64_t a, b;
      win_range_nonnull(knull, p0, p1, &a, &b);
      if (is_f64) {
        const double* kd = (const double*)key;
        double k = kd[i];
        if (bd.lo_kind == DSX_WIN_BOUND_OFFSET)
          s = dsx_win_lower<double>(kd, a, b, k + (desc ? -bd.lo_f : bd.lo_f),
                                    desc);
        if (bd.hi_kind == DSX_WIN_BOUND_OFFSET)
          e = dsx_win_upper<double>(kd, a, b, k + (desc ? -bd.hi_f : bd.hi_f),
                                    desc) - 1;
      } else {
        const int64_t* ki = (const int64_t*)key;
        int64_t k = ki[i];
        // a target beyond an int64 limit admits every key (the saturated
        // value says so) or none (said here: a key AT the limit would tie
        // with the saturated value)
        int ovf;
        if (bd.lo_kind == DSX_WIN_BOUND_OFFSET) {
          int64_t t = dsx_win_sat_add_ovf(k, desc ? -bd.lo_i : bd.lo_i, &ovf);
          s = dsx_win_low_none(ovf, desc)
                  ? b
                  : dsx_win_lower<int64_t>(ki, a, b, t, desc);
        }
        if (bd.hi_kind == DSX_WIN_BOUND_OFFSET) {
          int64_t t = dsx_win_sat_add_ovf(k, desc ? -bd.hi_i : bd.hi_i, &ovf);
          e = dsx_win_high_none(ovf, desc)
                  ? a - 1
                  : dsx_win_upper<int64_t>(ki, a, b, t, desc) - 1;
        }
      }
    }
    if (s > e) {
      s = 1;
      e = 0;
    }
    s_out[i] = (uint32_t)s;
    e_out[i] = (uint32_t)e;
  }
}

// level 0: tab[b] = op over rows [64 b, 64 b + 63] clipped to n, NULLs as the
// identity. One wave per block; a 256-thread workgroup strides over four.
__global__ void __launch_bounds__(BLOCK) k_win_rmq_blocks(
    const double* vs, const uint8_t* ok, int64_t n, int64_t blocks, int op,
    double* tab) {
  int lane = threadIdx.x & 63;
  int64_t b = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
  int64_t stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
  for (; b < blocks; b += stride) {  // uniform per wave
    int64_t row = (b << DSX_WIN_RMQ_SHIFT) + lane;
    double x = win_ident(op);
    if (row < n && ok[row]) x = vs[row];
    for (int d = 32; d >= 1; d >>= 1)
      x = win_comb(op, x, __shfl_xor(x, d, 64));
    if (lane == 0) tab[b] = x;
  }
}

// level j: cur[i] = op(prev[i], prev[i + half]) where both exist, half =
// 2^(j-1); entries whose range would leave the table are never read and
// hold the identity
__global__ void k_win_rmq_level(const double* prev, double* cur,
                                int64_t blocks, int64_t half, int op) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < blocks; i += stride)
    cur[i] = i + 2 * half <= blocks ? win_comb(op, prev[i], prev[i + half])
                                    : win_ident(op);
}

__device__ __forceinline__ double win_range_loose(const double* vs,
                                                  const uint8_t* ok, int op,
                                                  int64_t from, int64_t to,
                                                  double acc) {
  for (int64_t j = from; j <= to; j++)
    if (ok[j]) acc = win_comb(op, acc, vs[j]);
  return acc;
}

// cum/cnt: the FORWARD per-partition scans (SUM/COUNT/AVG, MIN/MAX with the
// low side unbounded, and the non-NULL count of a bounded MIN/MAX) or the
// REVERSE scan (MIN/MAX with only the high side unbounded). marks[] tells
// whether s is its partition's head, i.e. whether a prefix precedes it.
__global__ void k_win_range_apply(
    const uint32_t* perm, int64_t n, const uint8_t* marks, int func, int mm,
    const uint32_t* s_in, const uint32_t* e_in, const double* cum,
    const int64_t* cnt, const double* vs, const uint8_t* ok,
    const double* tab, int64_t blocks, DsxColumn v, int out_f64, void* out,
    uint8_t* out_valid) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < n; i += stride) {
    int64_t s = (int64_t)s_in[i], e = (int64_t)e_in[i];
    bool empty = s > e;
    // bounds come from k_win_range_bounds inside [0, n); keep every access
    // below in range whatever they hold
    if (e >= n) empty = true;
    int64_t r = (int64_t)perm[i];
    if (func == DSX_WIN_FIRST || func == DSX_WIN_LAST) {
      uint64_t bits = 0;
      bool valid = false;
      if (!empty) {
        int64_t src = (int64_t)perm[func == DSX_WIN_FIRST ? s : e];
        valid = !v.validity || v.validity[src];
        switch (v.dtype) {
          case DSX_I64: case DSX_F64:
            bits = ((const uint64_t*)v.data)[src]; break;
          case DSX_I32: case DSX_F32:
            bits = ((const uint32_t*)v.data)[src]; break;
          default:
            bits = ((const uint8_t*)v.data)[src];
        }
      }
      switch (v.dtype) {
        case DSX_I64: case DSX_F64:
          ((uint64_t*)out)[r] = bits; break;
        case DSX_I32: case DSX_F32:
          ((uint32_t*)out)[r] = (uint32_t)bits; break;
        default:
          ((uint8_t*)out)[r] = (uint8_t)bits;
      }
      if (out_valid) out_valid[r] = valid ? 1 : 0;
      continue;
    }
    double acc = 0.0;
    int64_t c = 0;
    if (!empty) {
      if (mm == WIN_RANGE_MM_FWD) {
        acc = cum[e];
        c = cnt[e];
      } else if (mm == WIN_RANGE_MM_REV) {
        acc = cum[s];
        c = cnt[s];
      } else {
        bool head = marks[s] != 0;
        c = cnt[e] - (head ? 0 : cnt[s - 1]);
        if (mm == WIN_RANGE_MM_NONE) {
          acc = cum[e] - (head ? 0.0 : cum[s - 1]);
        } else if (c > 0) {
          int op = win_rows_op(func);
          acc = win_ident(op);
          if (e - s + 1 <= DSX_WIN_RMQ_DIRECT_MAXW) {
            acc = win_range_loose(vs, ok, op, s, e, acc);
          } else {
            DsxWinRmqSplit sp = dsx_win_rmq_split(s, e);
            acc = win_range_loose(vs, ok, op, s, sp.head_end, acc);
            acc = win_range_loose(vs, ok, op, sp.tail_begin, e, acc);
            if (sp.b1 >= sp.b0 && sp.b1 < blocks) {
              const double* lv = tab + (int64_t)sp.level * blocks;
              acc = win_comb(op, acc, win_comb(op, lv[sp.left], lv[sp.right]));
            }
          }
        }
      }
    }
    // COUNT over an empty frame is 0, not NULL: emit it as a non-empty frame
    // that counted nothing
    win_rows_emit(func, empty && func != DSX_WIN_RCOUNT, acc, c, out_f64, r,
                  out, out_valid);
  }
}

static int64_t win_range_rmq_max_bytes() {
  const char* s = getenv("DSX_WIN_RANGE_RMQ_MAX_BYTES");
  if (s && *s) {
    char* end = nullptr;
    long long v = strtoll(s, &end, 10);
    if (end != s && v >= 0) return (int64_t)v;
  }
  return (int64_t)1 << 30;
}

// boundary starts of a sorted code sequence (k_win_mark + dsx_filter); the
// marks stay in `marks` for the scans
static int win_range_starts(DsxCtx* c, WinRowsTemps& tmp, const uint64_t* codes,
                            int64_t n, int grid, uint8_t* marks,
                            uint32_t** starts, int64_t* ns) {
  DsxInstr prog[1] = {{DSX_OP_COL, 0, 0}};
  DsxColumn mc{marks, nullptr, n, DSX_BOOL8};
  hipLaunchKernelGGL(k_win_mark, dim3(grid), dim3(BLOCK), 0, c->stream, codes,
                     n, marks);
  int rc = dsx_filter(c, prog, 1, &mc, 1, n, starts, ns);
  if (rc) return rc;
  tmp.ptrs.push_back(*starts);
  return 0;
}

static int win_range_run(DsxCtx* c, const uint32_t* perm, int64_t n,
                         const uint64_t* pcode_sorted,
                         const uint64_t* fcode_sorted, int func,
                         const DsxColumn* v_or_null, const DsxColumn* key,
                         int desc, const WinRangeBounds& bd, int out_dtype,
                         void* out, uint8_t* out_valid) {
  WinRowsTemps tmp(c);
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  int64_t ntiles = (n + WIN_TILE - 1) / WIN_TILE;
  bool positional = func == DSX_WIN_FIRST || func == DSX_WIN_LAST;
  bool minmax = func == DSX_WIN_RMIN || func == DSX_WIN_RMAX;
  int mm = WIN_RANGE_MM_NONE;
  if (minmax)
    mm = bd.lo_kind == DSX_WIN_BOUND_UNBOUNDED   ? WIN_RANGE_MM_FWD
         : bd.hi_kind == DSX_WIN_BOUND_UNBOUNDED ? WIN_RANGE_MM_REV
                                                 : WIN_RANGE_MM_RMQ;
  int64_t blocks = (n + DSX_WIN_RMQ_BLOCK - 1) / DSX_WIN_RMQ_BLOCK;
  int levels = dsx_win_rmq_levels(blocks);
  if (mm == WIN_RANGE_MM_RMQ) {
    int64_t bytes = 8 * blocks * (int64_t)levels;
    int64_t cap = win_range_rmq_max_bytes();
    if (bytes > cap)
      FAIL(-7, "dsx_window_range: MIN/MAX table of %lld bytes exceeds "
               "DSX_WIN_RANGE_RMQ_MAX_BYTES=%lld",
           (long long)bytes, (long long)cap);
  }
  void *pm_p = nullptr, *fm_p = nullptr, *s_p = nullptr, *e_p = nullptr;
  int rc = tmp.alloc(n, &pm_p);
  if (!rc) rc = tmp.alloc(n, &fm_p);
  if (!rc) rc = tmp.alloc(n * 4, &s_p);
  if (!rc) rc = tmp.alloc(n * 4, &e_p);
  if (rc) return rc;
  uint8_t* marks = (uint8_t*)pm_p;
  uint32_t *starts_p = nullptr, *starts_f = nullptr;
  int64_t np_ = 0, nf = 0;
  rc = win_range_starts(c, tmp, pcode_sorted, n, grid, marks, &starts_p, &np_);
  if (!rc)
    rc = win_range_starts(c, tmp, fcode_sorted, n, grid, (uint8_t*)fm_p,
                          &starts_f, &nf);
  if (rc) return rc;
  if (np_ < 1 || nf < 1)
    FAIL(-2, "dsx_window_range: no boundary at row 0");
  // ---- order key into sorted space -----------------------------------------
  void *key_p = nullptr, *kn_p = nullptr;
  int is_f64 = 0;
  if (key) {
    is_f64 = key->dtype == DSX_F64 || key->dtype == DSX_F32 ? 1 : 0;
    rc = tmp.alloc(n * 8, &key_p);
    if (!rc) rc = tmp.alloc(n, &kn_p);
    if (rc) return rc;
    ProfScope ps(c, "k_win_range_key");
    hipLaunchKernelGGL(k_win_range_key, dim3(grid), dim3(BLOCK), 0, c->stream,
                       perm, n, *key, is_f64, key_p, (uint8_t*)kn_p);
  }
  {
    ProfScope ps(c, "k_win_range_bounds");
    hipLaunchKernelGGL(k_win_range_bounds, dim3(grid), dim3(BLOCK), 0,
                       c->stream, n, (const uint32_t*)starts_p, np_,
                       (const uint32_t*)starts_f, nf, (const void*)key_p,
                       (const uint8_t*)kn_p, is_f64, desc, bd, (uint32_t*)s_p,
                       (uint32_t*)e_p);
  }
  DsxColumn v{};
  if (v_or_null) v = *v_or_null;
  int out_f64 = out_dtype == DSX_F64 ? 1 : 0;
  if (positional) {
    ProfScope ps(c, "k_win_range_apply");
    hipLaunchKernelGGL(k_win_range_apply, dim3(grid), dim3(BLOCK), 0,
                       c->stream, perm, n, (const uint8_t*)marks, func, mm,
                       (const uint32_t*)s_p, (const uint32_t*)e_p,
                       (const double*)nullptr, (const int64_t*)nullptr,
                       (const double*)nullptr, (const uint8_t*)nullptr,
                       (const double*)nullptr, blocks, v, 0, out, out_valid);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  // ---- value staging and the per-partition scan -----------------------------
  void *vs_p = nullptr, *ok_p = nullptr;
  rc = tmp.alloc(n * 8, &vs_p);
  if (!rc) rc = tmp.alloc(n, &ok_p);
  if (rc) return rc;
  {
    ProfScope ps(c, "k_win_stage");
    hipLaunchKernelGGL(k_win_stage, dim3(grid), dim3(BLOCK), 0, c->stream,
                       perm, n, v, (double*)vs_p, (uint8_t*)ok_p);
  }
  // a bounded MIN/MAX scans with ADD: only its non-NULL count is used
  int op = mm == WIN_RANGE_MM_RMQ ? WIN_OP_ADD : win_rows_op(func);
  int rev = mm == WIN_RANGE_MM_REV ? 1 : 0;
  void *cum_p = nullptr, *cnt_p = nullptr, *tv_p = nullptr, *tc_p = nullptr,
       *tf_p = nullptr, *cv_p = nullptr, *cc_p = nullptr;
  rc = tmp.alloc(n * 8, &cum_p);
  if (!rc) rc = tmp.alloc(n * 8, &cnt_p);
  if (!rc) rc = tmp.alloc(ntiles * 8, &tv_p);
  if (!rc) rc = tmp.alloc(ntiles * 8, &tc_p);
  if (!rc) rc = tmp.alloc(ntiles * 4, &tf_p);
  if (!rc) rc = tmp.alloc(ntiles * 8, &cv_p);
  if (!rc) rc = tmp.alloc(ntiles * 8, &cc_p);
  if (rc) return rc;
  {
    ProfScope ps(c, "k_win_segscan_tile");
    hipLaunchKernelGGL(k_win_segscan_tile, dim3((uint32_t)ntiles),
                       dim3(WIN_TILE), 0, c->stream, (const double*)vs_p,
                       (const uint8_t*)ok_p, (const uint8_t*)marks, n, op, rev,
                       (double*)cum_p, (int64_t*)cnt_p, (double*)tv_p,
                       (int64_t*)tc_p, (int32_t*)tf_p);
  }
  {
    ProfScope ps(c, "k_win_segscan_carry");
    hipLaunchKernelGGL(k_win_segscan_carry, dim3(1), dim3(WIN_TILE), 0,
                       c->stream, (const double*)tv_p, (const int64_t*)tc_p,
                       (const int32_t*)tf_p, ntiles, op, (double*)cv_p,
                       (int64_t*)cc_p);
  }
  {
    ProfScope ps(c, "k_win_segscan_apply");
    hipLaunchKernelGGL(k_win_segscan_apply, dim3(grid), dim3(BLOCK), 0,
                       c->stream, n, op, rev, (const int32_t*)tf_p,
                       (const double*)cv_p, (const int64_t*)cc_p,
                       (double*)cum_p, (int64_t*)cnt_p);
  }
  // ---- sparse table for a bounded MIN/MAX -----------------------------------
  void* tab_p = nullptr;
  if (mm == WIN_RANGE_MM_RMQ) {
    int mop = win_rows_op(func);
    rc = tmp.alloc(8 * blocks * (int64_t)levels, &tab_p);
    if (rc) return rc;
    double* tab = (double*)tab_p;
    {
      ProfScope ps(c, "k_win_rmq_blocks");
      int g = (int)min((int64_t)MAX_GRID,
                       (blocks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
      hipLaunchKernelGGL(k_win_rmq_blocks, dim3(g), dim3(BLOCK), 0, c->stream,
                         (const double*)vs_p, (const uint8_t*)ok_p, n, blocks,
                         mop, tab);
    }
    int g = (int)min((int64_t)MAX_GRID, (blocks + BLOCK - 1) / BLOCK);
    for (int j = 1; j < levels; j++) {
      ProfScope ps(c, "k_win_rmq_level");
      hipLaunchKernelGGL(k_win_rmq_level, dim3(g), dim3(BLOCK), 0, c->stream,
                         (const double*)(tab + (int64_t)(j - 1) * blocks),
                         tab + (int64_t)j * blocks, blocks,
                         (int64_t)1 << (j - 1), mop);
    }
  }
  {
    ProfScope ps(c, "k_win_range_apply");
    hipLaunchKernelGGL(k_win_range_apply, dim3(grid), dim3(BLOCK), 0,
                       c->stream, perm, n, (const uint8_t*)marks, func, mm,
                       (const uint32_t*)s_p, (const uint32_t*)e_p,
                       (const double*)cum_p, (const int64_t*)cnt_p,
                       (const double*)vs_p, (const uint8_t*)ok_p,
                       (const double*)tab_p, blocks, v, out_f64, out,
                       out_valid);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int dsx_window_range(DsxCtx* c, const uint32_t* perm, int64_t n,
                                const uint64_t* pcode_sorted,
                                const uint64_t* fcode_sorted, int func,
                                const DsxColumn* v_or_null,
                                const DsxColumn* key_or_null, int desc,
                                const DsxWinBound* lo, const DsxWinBound* hi,
                                int out_dtype, void** out_data,
                                uint8_t** out_valid, int want_valid) {
  *out_data = nullptr;
  *out_valid = nullptr;
  bool pos = func == DSX_WIN_FIRST || func == DSX_WIN_LAST;
  bool agg = func >= DSX_WIN_RSUM && func <= DSX_WIN_RAVG;
  if (!pos && !agg) FAIL(-3, "dsx_window_range: unsupported func %d", func);
  if ((pos || func != DSX_WIN_RCOUNT) && !v_or_null)
    FAIL(-3, "dsx_window_range: func %d needs a value column", func);
  if (pos && out_dtype != v_or_null->dtype)
    FAIL(-3, "dsx_window_range: FIRST/LAST keep the value dtype");
  if (agg && out_dtype != DSX_F64 && out_dtype != DSX_I64)
    FAIL(-3, "dsx_window_range: aggregate output must be i64 or f64");
  if (agg && func == DSX_WIN_RAVG && out_dtype != DSX_F64)
    FAIL(-3, "dsx_window_range: AVG output must be f64");
  if (n < 0 || n > (int64_t)0xFFFFFFFFll)
    FAIL(-3, "dsx_window_range: bad row count %lld", (long long)n);
  if (!lo || !hi) FAIL(-3, "dsx_window_range: missing bound");
  for (const DsxWinBound* b : {lo, hi})
    if (b->kind != DSX_WIN_BOUND_UNBOUNDED &&
        b->kind != DSX_WIN_BOUND_CURRENT && b->kind != DSX_WIN_BOUND_OFFSET)
      FAIL(-3, "dsx_window_range: bad bound kind %d", b->kind);
  bool any_off = lo->kind == DSX_WIN_BOUND_OFFSET ||
                 hi->kind == DSX_WIN_BOUND_OFFSET;
  if (any_off && !key_or_null)
    FAIL(-3, "dsx_window_range: an offset bound needs the order key");
  if (any_off) {
    int kd = key_or_null->dtype;
    if (kd != DSX_I64 && kd != DSX_I32 && kd != DSX_I8 && kd != DSX_F64 &&
        kd != DSX_F32)
      FAIL(-3, "dsx_window_range: order key dtype %d", kd);
    if (key_or_null->len < n)
      FAIL(-3, "dsx_window_range: order key shorter than the table");
    bool fk = kd == DSX_F64 || kd == DSX_F32;
    for (const DsxWinBound* b : {lo, hi}) {
      if (b->kind != DSX_WIN_BOUND_OFFSET) continue;
      // -INT64_MIN does not exist: a DESC key negates the offset
      if (!fk && b->ival == INT64_MIN)
        FAIL(-3, "dsx_window_range: offset out of range");
      if (fk && b->fval != b->fval)
        FAIL(-3, "dsx_window_range: NaN offset");
    }
  }
  WinRangeBounds bd{lo->kind, hi->kind, lo->ival, hi->ival, lo->fval,
                    hi->fval};
  int sz = rj_dtype_size(out_dtype);
  int rc = pool_alloc(c, (n > 0 ? n : 1) * sz, out_data);
  if (!rc && want_valid)
    rc = pool_alloc(c, (n > 0 ? n : 1), (void**)out_valid);
  if (!rc && n > 0)
    rc = win_range_run(c, perm, n, pcode_sorted, fcode_sorted, func,
                       v_or_null, any_off ? key_or_null : nullptr,
                       desc ? 1 : 0, bd, out_dtype, *out_data,
                       want_valid ? *out_valid : nullptr);
  if (rc) {
    if (*out_data) pool_release(c, *out_data);
    if (*out_valid) pool_release(c, *out_valid);
    *out_data = nullptr;
    *out_valid = nullptr;
  }
  return rc;
}
