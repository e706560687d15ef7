// window_rows.inc — device explicit ROWS frames (reference
// rel/logical/window.py:145-198 runs these through pandas
// expanding/rolling/BaseIndexer per sorted partition). Included by
// dsxhip.hip after window.inc (shares k_win_mark / win_bsearch).
//
// A frame is (lo_off, hi_off) relative to sorted position i, either side
// optionally unbounded. For row i of partition [p0, p1):
//   s = max(p0, i + lo_off)   (p0 when the low side is unbounded)
//   e = min(p1 - 1, i + hi_off)  (p1 - 1 when the high side is unbounded)
// and the frame is EMPTY when s > e → NULL for every function, COUNT too
// (pandas rolling with min_periods=1 yields NaN there).
//
//   k_win_stage      value/validity gathered into sorted space as f64 + u8
//   k_win_rows_tile  bounded narrow frames: a 256-row tile plus its halo in
//                    LDS, every thread reduces its own clipped frame
//   k_win_segscan_*  per-partition inclusive scan over sorted space in three
//                    bounded phases (tile scan, carry scan, apply) — no
//                    block ever waits on another
//   k_win_rows_prefix frame result from the scans (prefix difference for
//                    SUM/COUNT/AVG, scan lookups for half-unbounded
//                    MIN/MAX), and the positional FIRST_VALUE/LAST_VALUE
// Results scatter back to ORIGINAL row order through the permutation.

#define WIN_ROWS_DIRECT_MAXW DSX_WIN_ROWS_DIRECT_MAXW
#define WIN_ROWS_TILE_MAXW DSX_WIN_ROWS_TILE_MAXW
#define WIN_TILE 256
#define WIN_TILE_LDS (WIN_TILE - 1 + WIN_ROWS_TILE_MAXW)

enum { WIN_OP_ADD = 0, WIN_OP_MIN = 1, WIN_OP_MAX = 2 };

__device__ __forceinline__ double win_ident(int op) {
  return op == WIN_OP_MIN ? __builtin_inf()
         : op == WIN_OP_MAX ? -__builtin_inf()
                            : 0.0;
}

__device__ __forceinline__ double win_comb(int op, double l, double r) {
  if (op == WIN_OP_MIN) return l < r ? l : r;
  if (op == WIN_OP_MAX) return l > r ? l : r;
  return l + r;
}

__host__ __device__ __forceinline__ int win_rows_op(int func) {
  return func == DSX_WIN_RMIN ? WIN_OP_MIN
         : func == DSX_WIN_RMAX ? WIN_OP_MAX
                                : WIN_OP_ADD;
}

// frame bounds of sorted position i (inclusive); empty when s > e
__device__ __forceinline__ void win_rows_bounds(
    const uint32_t* starts_p, int64_t np_, int64_t n, int64_t i, int lo_unb,
    int64_t lo_off, int hi_unb, int64_t hi_off, int64_t* p0_, int64_t* p1_,
    int64_t* s_, int64_t* e_) {
  int64_t sp = win_bsearch(starts_p, np_, i);
  int64_t p0 = (int64_t)starts_p[sp];
  int64_t p1 = sp + 1 < np_ ? (int64_t)starts_p[sp + 1] : n;
  int64_t s = p0, e = p1 - 1;
  if (!lo_unb && i + lo_off > s) s = i + lo_off;
  if (!hi_unb && i + hi_off < e) e = i + hi_off;
  *p0_ = p0;
  *p1_ = p1;
  *s_ = s;
  *e_ = e;
}

// one aggregate result into original row r. acc = SUM / MIN / MAX over the
// frame's non-NULL values, cnt = how many there were
__device__ __forceinline__ void win_rows_emit(int func, bool empty, double acc,
                                              int64_t cnt, int out_f64,
                                              int64_t r, void* out,
                                              uint8_t* out_valid) {
  bool any;
  double x;
  if (func == DSX_WIN_RCOUNT) {
    any = !empty;  // COUNT over a non-empty frame may be 0, never NULL
    x = (double)cnt;
  } else {
    any = !empty && cnt > 0;
    x = func == DSX_WIN_RAVG && any ? acc / (double)cnt : acc;
  }
  if (out_f64)
    ((double*)out)[r] = any ? x : __builtin_nan("");
  else if (func == DSX_WIN_RCOUNT)
    ((int64_t*)out)[r] = any ? cnt : 0;
  else
    ((int64_t*)out)[r] = any ? (int64_t)x : 0;
  if (out_valid) out_valid[r] = any ? 1 : 0;
}

// vs[i] = (double) v[perm[i]], ok[i] = its validity — contiguous in sorted
// space so the tile and scan passes stream coalesced. COUNT(*) (no value
// column): every row valid with value 1
__global__ void k_win_stage(const uint32_t* perm, int64_t n, DsxColumn v,
                            double* vs, uint8_t* ok) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < n; i += stride) {
    double x = 1.0;
    bool valid = true;
    if (v.data) {
      int64_t r = (int64_t)perm[i];
      valid = !v.validity || v.validity[r];
      x = 0.0;
      if (valid) {
        switch (v.dtype) {
          case DSX_F64: x = ((const double*)v.data)[r]; break;
          case DSX_I64: x = (double)((const int64_t*)v.data)[r]; break;
          case DSX_I32: x = (double)((const int32_t*)v.data)[r]; break;
          case DSX_F32: x = (double)((const float*)v.data)[r]; break;
          default: x = (double)((const int8_t*)v.data)[r];
        }
      }
    }
    vs[i] = x;
    ok[i] = valid ? 1 : 0;
  }
}

// bounded frames of width W = hi_off - lo_off + 1 <= WIN_ROWS_TILE_MAXW
// (W <= 0: every frame empty). Block b owns sorted positions
// [256 b, 256 b + 255]; it stages [256 b + lo_off, 256 b + 255 + hi_off]
// clipped to [0, n) — at most 255 + W entries — and each thread reduces
// its own partition-clipped frame left to right out of LDS.
__global__ void __launch_bounds__(WIN_TILE) k_win_rows_tile(
    const uint32_t* perm, int64_t n, const uint32_t* starts_p, int64_t np_,
    const double* vs, const uint8_t* ok, int func, int64_t lo_off,
    int64_t hi_off, int out_f64, void* out, uint8_t* out_valid) {
  __shared__ double s_v[WIN_TILE_LDS];
  __shared__ uint8_t s_ok[WIN_TILE_LDS];
  int64_t base = (int64_t)blockIdx.x * WIN_TILE;
  int64_t g0 = base + lo_off;
  int64_t g1 = base + WIN_TILE - 1 + hi_off;
  if (g0 < 0) g0 = 0;
  if (g1 > n - 1) g1 = n - 1;
  int64_t cnt_lds = g1 - g0 + 1;  // <= 0 when nothing is in range
  if (cnt_lds > WIN_TILE_LDS) cnt_lds = WIN_TILE_LDS;  // host checked W
  for (int64_t k = threadIdx.x; k < cnt_lds; k += WIN_TILE) {
    s_v[k] = vs[g0 + k];
    s_ok[k] = ok[g0 + k];
  }
  __syncthreads();
  int64_t i = base + threadIdx.x;
  if (i >= n) return;
  int64_t p0, p1, s, e;
  win_rows_bounds(starts_p, np_, n, i, 0, lo_off, 0, hi_off, &p0, &p1, &s,
                  &e);
  int op = win_rows_op(func);
  double acc = win_ident(op);
  int64_t cnt = 0;
  // s >= max(0, i + lo_off) >= g0 and e <= min(n - 1, i + hi_off) <= g1
  for (int64_t j = s; j <= e; j++) {
    int64_t k = j - g0;
    if (k < 0 || k >= cnt_lds) break;  // unreachable; keeps LDS in bounds
    if (s_ok[k]) {
      acc = win_comb(op, acc, s_v[k]);
      cnt++;
    }
  }
  win_rows_emit(func, s > e, acc, cnt, out_f64, (int64_t)perm[i], out,
                out_valid);
}

// ---- segmented (per-partition) inclusive scan, three bounded phases --------
// Logical index k runs over sorted positions forward (pos = k) or reverse
// (pos = n - 1 - k); a segment head is a partition's first position in
// that direction. marks[] = k_win_mark over the partition codes.
__device__ __forceinline__ bool win_seg_head(const uint8_t* marks, int64_t n,
                                             int64_t pos, int rev) {
  if (!rev) return marks[pos] != 0;
  return pos == n - 1 || marks[pos + 1] != 0;
}

// in-LDS segmented Hillis-Steele over one 256-entry chunk. On return
// s_f[t] says whether a head lies at or before t inside the chunk
__device__ __forceinline__ void win_seg_scan256(int op, double* s_v,
                                                int64_t* s_c, uint8_t* s_f) {
  int t = threadIdx.x;
  for (int d = 1; d < WIN_TILE; d <<= 1) {
    double pv = 0.0;
    int64_t pc = 0;
    uint8_t pf = 0;
    if (t >= d) {
      pv = s_v[t - d];
      pc = s_c[t - d];
      pf = s_f[t - d];
    }
    __syncthreads();
    if (t >= d && !s_f[t]) {
      s_v[t] = win_comb(op, pv, s_v[t]);
      s_c[t] += pc;
      s_f[t] = pf;
    }
    __syncthreads();
  }
}

// phase 1: tile-local scan into cum/cnt, the tile's tail aggregate, and the
// logical offset of its first segment head (WIN_TILE when it has none)
__global__ void __launch_bounds__(WIN_TILE) k_win_segscan_tile(
    const double* vs, const uint8_t* ok, const uint8_t* marks, int64_t n,
    int op, int rev, double* cum, int64_t* cnt, double* tile_v,
    int64_t* tile_c, int32_t* tile_first) {
  __shared__ double s_v[WIN_TILE];
  __shared__ int64_t s_c[WIN_TILE];
  __shared__ uint8_t s_f[WIN_TILE];
  __shared__ int s_first;
  int t = threadIdx.x;
  if (t == 0) s_first = WIN_TILE;
  __syncthreads();
  int64_t k = (int64_t)blockIdx.x * WIN_TILE + t;
  int64_t pos = rev ? n - 1 - k : k;
  double x = win_ident(op);
  int64_t c = 0;
  uint8_t f = 0;
  if (k < n) {
    if (ok[pos]) {
      x = vs[pos];
      c = 1;
    }
    f = win_seg_head(marks, n, pos, rev) ? 1 : 0;
    if (f) atomicMin(&s_first, t);
  }
  s_v[t] = x;
  s_c[t] = c;
  s_f[t] = f;
  __syncthreads();
  win_seg_scan256(op, s_v, s_c, s_f);
  if (k < n) {
    cum[pos] = s_v[t];
    cnt[pos] = s_c[t];
  }
  if (t == WIN_TILE - 1) {
    // lanes past n hold the identity without a head, so slot 255 carries
    // the scan value of the tile's last real element
    tile_v[blockIdx.x] = s_v[t];
    tile_c[blockIdx.x] = s_c[t];
    tile_first[blockIdx.x] = s_first;
  }
}

// phase 2 (one block): exclusive segmented scan of the tile aggregates →
// the carry entering each tile. ceil(ntiles / 256) iterations, fixed at
// launch.
__global__ void __launch_bounds__(WIN_TILE) k_win_segscan_carry(
    const double* tile_v, const int64_t* tile_c, const int32_t* tile_first,
    int64_t ntiles, int op, double* cin_v, int64_t* cin_c) {
  __shared__ double s_v[WIN_TILE];
  __shared__ int64_t s_c[WIN_TILE];
  __shared__ uint8_t s_f[WIN_TILE];
  int t = threadIdx.x;
  double carry_v = win_ident(op);
  int64_t carry_c = 0;
  for (int64_t base = 0; base < ntiles; base += WIN_TILE) {
    int64_t j = base + t;
    double x = win_ident(op);
    int64_t c = 0;
    uint8_t f = 0;
    if (j < ntiles) {
      x = tile_v[j];
      c = tile_c[j];
      f = tile_first[j] < WIN_TILE ? 1 : 0;
    }
    s_v[t] = x;
    s_c[t] = c;
    s_f[t] = f;
    __syncthreads();
    win_seg_scan256(op, s_v, s_c, s_f);
    double iv = s_v[t];
    int64_t ic = s_c[t];
    if (!s_f[t]) {  // no head up to here in this chunk: earlier chunks count
      iv = win_comb(op, carry_v, iv);
      ic += carry_c;
    }
    if (j == 0) {
      cin_v[0] = win_ident(op);
      cin_c[0] = 0;
    }
    if (j + 1 < ntiles) {
      cin_v[j + 1] = iv;
      cin_c[j + 1] = ic;
    }
    __syncthreads();
    if (t == WIN_TILE - 1) {
      s_v[0] = iv;
      s_c[0] = ic;
    }
    __syncthreads();
    carry_v = s_v[0];
    carry_c = s_c[0];
    __syncthreads();
  }
}

// phase 3: elements before their tile's first head continue a partition
// that began in an earlier tile — fold the incoming carry in
__global__ void k_win_segscan_apply(int64_t n, int op, int rev,
                                    const int32_t* tile_first,
                                    const double* cin_v, const int64_t* cin_c,
                                    double* cum, int64_t* cnt) {
  int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; k < n; k += stride) {
    int64_t tile = k / WIN_TILE;
    if ((int32_t)(k % WIN_TILE) >= tile_first[tile]) continue;
    int64_t pos = rev ? n - 1 - k : k;
    cum[pos] = win_comb(op, cin_v[tile], cum[pos]);
    cnt[pos] += cin_c[tile];
  }
}

// frame result from the scans, or the positional FIRST/LAST copy
//   SUM/COUNT/AVG (forward scan): cum[e] - (s > p0 ? cum[s - 1] : 0)
//   MIN/MAX low side unbounded (forward scan): value at e (p1 - 1 when the
//     high side is unbounded too); high side unbounded only (reverse scan):
//     value at s
//   FIRST_VALUE / LAST_VALUE: the row at s / e, bit-for-bit in v's dtype
__global__ void k_win_rows_prefix(
    const uint32_t* perm, int64_t n, const uint32_t* starts_p, int64_t np_,
    int func, int lo_unb, int64_t lo_off, int hi_unb, int64_t hi_off,
    const double* cum, const int64_t* cnt, DsxColumn v, int out_f64,
    void* out, uint8_t* out_valid) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < n; i += stride) {
    int64_t p0, p1, s, e;
    win_rows_bounds(starts_p, np_, n, i, lo_unb, lo_off, hi_unb, hi_off, &p0,
                    &p1, &s, &e);
    bool empty = s > e;
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
      if (func == DSX_WIN_RMIN || func == DSX_WIN_RMAX) {
        int64_t at = lo_unb ? e : s;  // reverse scan when only hi is open
        acc = cum[at];
        c = cnt[at];
      } else {
        acc = cum[e];
        c = cnt[e];
        if (s > p0) {
          acc -= cum[s - 1];
          c -= cnt[s - 1];
        }
      }
    }
    win_rows_emit(func, empty, acc, c, out_f64, r, out, out_valid);
  }
}

// pool allocations of one dsx_window_rows call: released on every exit path
struct WinRowsTemps {
  DsxCtx* c;
  std::vector<void*> ptrs;
  explicit WinRowsTemps(DsxCtx* ctx) : c(ctx) {}
  ~WinRowsTemps() {
    for (void* p : ptrs) pool_release(c, p);
  }
  int alloc(int64_t bytes, void** out) {
    int rc = pool_alloc(c, bytes, out);
    if (!rc) ptrs.push_back(*out);
    return rc;
  }
};

extern "C" int dsx_window_rows_limits(int* direct_maxw, int* tile_maxw) {
  if (direct_maxw) *direct_maxw = WIN_ROWS_DIRECT_MAXW;
  if (tile_maxw) *tile_maxw = WIN_ROWS_TILE_MAXW;
  return 0;
}

static int win_rows_run(DsxCtx* c, const uint32_t* perm, int64_t n,
                        const uint64_t* pcode_sorted, int func,
                        const DsxColumn* v_or_null, int lo_unb, int64_t lo_off,
                        int hi_unb, int64_t hi_off, int out_dtype, void* out,
                        uint8_t* out_valid) {
  WinRowsTemps tmp(c);
  void* marks_p = nullptr;
  int rc = tmp.alloc(n, &marks_p);
  if (rc) return rc;
  uint8_t* marks = (uint8_t*)marks_p;
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  int64_t ntiles = (n + WIN_TILE - 1) / WIN_TILE;
  DsxInstr prog[1] = {{DSX_OP_COL, 0, 0}};
  DsxColumn mc{marks, nullptr, n, DSX_BOOL8};
  uint32_t* starts_p = nullptr;
  int64_t np_ = 0;
  hipLaunchKernelGGL(k_win_mark, dim3(grid), dim3(BLOCK), 0, c->stream,
                     pcode_sorted, n, marks);
  rc = dsx_filter(c, prog, 1, &mc, 1, n, &starts_p, &np_);
  if (rc) return rc;
  tmp.ptrs.push_back(starts_p);
  DsxColumn v{};
  if (v_or_null) v = *v_or_null;
  int out_f64 = out_dtype == DSX_F64 ? 1 : 0;
  if (func == DSX_WIN_FIRST || func == DSX_WIN_LAST) {
    ProfScope ps(c, "k_win_rows_prefix");
    hipLaunchKernelGGL(k_win_rows_prefix, dim3(grid), dim3(BLOCK), 0,
                       c->stream, perm, n, starts_p, np_, func, lo_unb, lo_off,
                       hi_unb, hi_off, (const double*)nullptr,
                       (const int64_t*)nullptr, v, 0, out, out_valid);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  void* vs_p = nullptr;
  void* ok_p = nullptr;
  rc = tmp.alloc(n * 8, &vs_p);
  if (!rc) rc = tmp.alloc(n, &ok_p);
  if (rc) return rc;
  {
    ProfScope ps(c, "k_win_stage");
    hipLaunchKernelGGL(k_win_stage, dim3(grid), dim3(BLOCK), 0, c->stream,
                       perm, n, v, (double*)vs_p, (uint8_t*)ok_p);
  }
  bool bounded = !lo_unb && !hi_unb;
  bool minmax = func == DSX_WIN_RMIN || func == DSX_WIN_RMAX;
  // W in (-2n, 2n] after the caller's clamp to [-n, n]
  int64_t w = bounded ? hi_off - lo_off + 1 : 0;
  if (bounded &&
      w <= (minmax ? WIN_ROWS_TILE_MAXW : WIN_ROWS_DIRECT_MAXW)) {
    ProfScope ps(c, "k_win_rows_tile");
    hipLaunchKernelGGL(k_win_rows_tile, dim3((uint32_t)ntiles),
                       dim3(WIN_TILE), 0, c->stream, perm, n, starts_p, np_,
                       (const double*)vs_p, (const uint8_t*)ok_p, func, lo_off,
                       hi_off, out_f64, out, out_valid);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  if (bounded && minmax)
    FAIL(-7, "bounded MIN/MAX ROWS frame of width %lld exceeds %d",
         (long long)w, WIN_ROWS_TILE_MAXW);
  int op = win_rows_op(func);
  int rev = minmax && !lo_unb ? 1 : 0;  // only the high side is open
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
  {
    ProfScope ps(c, "k_win_rows_prefix");
    hipLaunchKernelGGL(k_win_rows_prefix, dim3(grid), dim3(BLOCK), 0,
                       c->stream, perm, n, starts_p, np_, func, lo_unb, lo_off,
                       hi_unb, hi_off, (const double*)cum_p,
                       (const int64_t*)cnt_p, v, out_f64, out, out_valid);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int dsx_window_rows(DsxCtx* c, const uint32_t* perm, int64_t n,
                               const uint64_t* pcode_sorted, int func,
                               const DsxColumn* v_or_null, int lo_unbounded,
                               int64_t lo_off, int hi_unbounded,
                               int64_t hi_off, int out_dtype, void** out_data,
                               uint8_t** out_valid, int want_valid) {
  *out_data = nullptr;
  *out_valid = nullptr;
  bool pos = func == DSX_WIN_FIRST || func == DSX_WIN_LAST;
  bool agg = func >= DSX_WIN_RSUM && func <= DSX_WIN_RAVG;
  if (!pos && !agg) FAIL(-3, "dsx_window_rows: unsupported func %d", func);
  if ((pos || func != DSX_WIN_RCOUNT) && !v_or_null)
    FAIL(-3, "dsx_window_rows: func %d needs a value column", func);
  if (pos && out_dtype != v_or_null->dtype)
    FAIL(-3, "dsx_window_rows: FIRST/LAST keep the value dtype");
  if (agg && out_dtype != DSX_F64 && out_dtype != DSX_I64)
    FAIL(-3, "dsx_window_rows: aggregate output must be i64 or f64");
  if (agg && func == DSX_WIN_RAVG && out_dtype != DSX_F64)
    FAIL(-3, "dsx_window_rows: AVG output must be f64");
  if (n < 0 || n > (int64_t)0xFFFFFFFFll)
    FAIL(-3, "dsx_window_rows: bad row count %lld", (long long)n);
  // offsets beyond the table act like the table edge; clamping keeps
  // i + off and the frame width inside int64
  if (lo_off < -n) lo_off = -n;
  if (lo_off > n) lo_off = n;
  if (hi_off < -n) hi_off = -n;
  if (hi_off > n) hi_off = n;
  int sz = rj_dtype_size(out_dtype);
  int rc = pool_alloc(c, (n > 0 ? n : 1) * sz, out_data);
  if (!rc && want_valid)
    rc = pool_alloc(c, (n > 0 ? n : 1), (void**)out_valid);
  if (!rc && n > 0)
    rc = win_rows_run(c, perm, n, pcode_sorted, func, v_or_null,
                      lo_unbounded ? 1 : 0, lo_off, hi_unbounded ? 1 : 0,
                      hi_off, out_dtype, *out_data,
                      want_valid ? *out_valid : nullptr);
  if (rc) {
    if (*out_data) pool_release(c, *out_data);
    if (*out_valid) pool_release(c, *out_valid);
    *out_data = nullptr;
    *out_valid = nullptr;
  }
  return rc;
}
