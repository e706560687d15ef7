// window.inc — device ordered window frames (VERDICT r1 #5; reference
// rel/logical/window.py:212-428 computes these in pandas per sorted
// partition). Included by dsxhip.hip.
//
// The caller supplies the sort permutation (dsx_sort_perm over
// partition-then-order keys) plus the per-row partition codes and
// full (partition+order) codes GATHERED INTO SORTED ORDER. Here:
//   (1) boundary marks + compaction → partition starts / peer starts,
//   (2) per-position binary search over the starts → ROW_NUMBER / RANK /
//       DENSE_RANK / LAG / LEAD / FIRST_VALUE,
//   (3) running aggregates (default RANGE UNBOUNDED..CURRENT frame with
//       peer broadcast): one block per partition — chunked LDS inclusive
//       scan with a running carry, then each row takes its peer group's
//       last cumulative value.
// Results scatter back to ORIGINAL row order through the permutation.

enum DsxWinFunc {
  DSX_WIN_ROWNO = 0, DSX_WIN_RANK = 1, DSX_WIN_DENSERANK = 2,
  DSX_WIN_LAG = 3, DSX_WIN_LEAD = 4, DSX_WIN_FIRST = 5,
  DSX_WIN_RSUM = 6, DSX_WIN_RCOUNT = 7, DSX_WIN_RMIN = 8, DSX_WIN_RMAX = 9,
  DSX_WIN_RAVG = 10,
  DSX_WIN_LAST = 11,  // explicit ROWS frames only (window_rows.inc)
};

__global__ void k_win_mark(const uint64_t* codes, int64_t n, uint8_t* out) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < n; i += stride)
    out[i] = (i == 0) || (codes[i] != codes[i - 1]);
}

__device__ __forceinline__ int64_t win_bsearch(const uint32_t* starts,
                                               int64_t ns, int64_t pos) {
  // greatest k with starts[k] <= pos
  int64_t lo = 0, hi = ns - 1;
  while (lo < hi) {
    int64_t mid = (lo + hi + 1) >> 1;
    if ((int64_t)starts[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ranking + shift family: one pass over sorted positions
__global__ void k_win_pos(const uint32_t* perm, int64_t n,
                          const uint32_t* starts_p, int64_t np_,
                          const uint32_t* starts_f, int64_t nf, int func,
                          DsxColumn v, int64_t offset, int64_t def_bits,
                          int has_def, void* out, uint8_t* out_valid) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < n; i += stride) {
    int64_t sp = win_bsearch(starts_p, np_, i);
    int64_t p0 = (int64_t)starts_p[sp];
    int64_t p1 = sp + 1 < np_ ? (int64_t)starts_p[sp + 1] : n;
    int64_t r = (int64_t)perm[i];
    if (func == DSX_WIN_ROWNO) {
      ((int64_t*)out)[r] = i - p0 + 1;
      continue;
    }
    if (func == DSX_WIN_RANK || func == DSX_WIN_DENSERANK) {
      int64_t sf = win_bsearch(starts_f, nf, i);
      if (func == DSX_WIN_RANK) {
        ((int64_t*)out)[r] = (int64_t)starts_f[sf] - p0 + 1;
      } else {
        int64_t f0 = win_bsearch(starts_f, nf, p0);
        ((int64_t*)out)[r] = sf - f0 + 1;
      }
      continue;
    }
    // value-carrying: LAG/LEAD/FIRST_VALUE copy v through the permutation
    int64_t j;
    bool ok;
    if (func == DSX_WIN_FIRST) {
      j = p0;
      ok = true;
    } else if (func == DSX_WIN_LAG) {
      j = i - offset;
      ok = j >= p0;
    } else {
      j = i + offset;
      ok = j < p1;
    }
    uint64_t bits = (uint64_t)def_bits;
    bool valid = has_def != 0;
    if (ok) {
      int64_t src = (int64_t)perm[j];
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
  }
}

// running aggregates: one block per partition, chunked LDS inclusive scan
// with running carry → cum[] in SORTED space (f64 accumulate; count i64)
__global__ void __launch_bounds__(256) k_win_scan(
    const uint32_t* perm, const uint32_t* starts_p, int64_t np_, int64_t n,
    int func, DsxColumn v, double* cum, int64_t* cnt) {
  __shared__ double s_val[256];
  __shared__ int64_t s_cnt[256];
  int64_t p0 = (int64_t)starts_p[blockIdx.x];
  int64_t p1 = blockIdx.x + 1 < np_ ? (int64_t)starts_p[blockIdx.x + 1] : n;
  double carry = (func == DSX_WIN_RMIN) ? __builtin_inf()
                 : (func == DSX_WIN_RMAX) ? -__builtin_inf()
                                          : 0.0;
  int64_t ccnt = 0;
  for (int64_t base = p0; base < p1; base += 256) {
    int64_t i = base + threadIdx.x;
    double x = (func == DSX_WIN_RMIN) ? __builtin_inf()
               : (func == DSX_WIN_RMAX) ? -__builtin_inf()
                                        : 0.0;
    int64_t c = 0;
    if (i < p1) {
      int64_t r = (int64_t)perm[i];
      bool valid = !v.data || !v.validity || v.validity[r];
      if (v.data && valid) {
        switch (v.dtype) {
          case DSX_F64: x = ((const double*)v.data)[r]; break;
          case DSX_I64: x = (double)((const int64_t*)v.data)[r]; break;
          case DSX_I32: x = (double)((const int32_t*)v.data)[r]; break;
          case DSX_F32: x = (double)((const float*)v.data)[r]; break;
          default: x = (double)((const int8_t*)v.data)[r];
        }
        c = 1;
      } else if (!v.data) {
        c = 1;  // COUNT(*) counts rows
      } else if (func == DSX_WIN_RMIN) {
        x = __builtin_inf();
      } else if (func == DSX_WIN_RMAX) {
        x = -__builtin_inf();
      } else {
        x = 0.0;  // NULL contributes identity to SUM
      }
    }
    s_val[threadIdx.x] = x;
    s_cnt[threadIdx.x] = c;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      double pv = 0.0;
      int64_t pc = 0;
      if (threadIdx.x >= d) {
        pv = s_val[threadIdx.x - d];
        pc = s_cnt[threadIdx.x - d];
      }
      __syncthreads();
      if (threadIdx.x >= d) {
        if (func == DSX_WIN_RMIN) s_val[threadIdx.x] =
            pv < s_val[threadIdx.x] ? pv : s_val[threadIdx.x];
        else if (func == DSX_WIN_RMAX) s_val[threadIdx.x] =
            pv > s_val[threadIdx.x] ? pv : s_val[threadIdx.x];
        else s_val[threadIdx.x] += pv;
        s_cnt[threadIdx.x] += pc;
      }
      __syncthreads();
    }
    if (i < p1) {
      double tv = s_val[threadIdx.x];
      int64_t tc = s_cnt[threadIdx.x] + ccnt;
      if (func == DSX_WIN_RMIN) tv = tv < carry ? tv : carry;
      else if (func == DSX_WIN_RMAX) tv = tv > carry ? tv : carry;
      else tv += carry;
      cum[i] = tv;
      cnt[i] = tc;
    }
    __syncthreads();
    double last = s_val[255];
    int64_t lastc = s_cnt[255];
    if (threadIdx.x == 0) {
      if (func == DSX_WIN_RMIN) carry = last < carry ? last : carry;
      else if (func == DSX_WIN_RMAX) carry = last > carry ? last : carry;
      else carry += last;
      ccnt += lastc;
    }
    // broadcast carry via LDS
    __syncthreads();
    if (threadIdx.x == 0) { s_val[0] = carry; s_cnt[0] = ccnt; }
    __syncthreads();
    carry = s_val[0];
    ccnt = s_cnt[0];
    __syncthreads();
  }
}

// peer broadcast: out[perm[i]] = cum at the LAST position of i's peer group
__global__ void k_win_peer(const uint32_t* perm, int64_t n,
                           const uint32_t* starts_f, int64_t nf,
                           const uint32_t* starts_p, int64_t np_,
                           const double* cum, const int64_t* cnt, int func,
                           int out_f64, void* out, uint8_t* out_valid) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < n; i += stride) {
    int64_t sf = win_bsearch(starts_f, nf, i);
    int64_t end = sf + 1 < nf ? (int64_t)starts_f[sf + 1] - 1 : n - 1;
    // peer group never crosses a partition (partition starts ⊂ peer starts)
    int64_t r = (int64_t)perm[i];
    if (func == DSX_WIN_RCOUNT) {
      ((int64_t*)out)[r] = cnt[end];
      if (out_valid) out_valid[r] = 1;
      continue;
    }
    // SUM/MIN/MAX over zero non-null rows → NULL
    int64_t sp = win_bsearch(starts_p, np_, i);
    bool any = cnt[end] > 0;
    double x = cum[end];
    if (func == DSX_WIN_RAVG) x = any ? x / (double)cnt[end] : x;
    (void)sp;
    if (out_f64)
      ((double*)out)[r] = any ? x : __builtin_nan("");
    else
      ((int64_t*)out)[r] = any ? (int64_t)x : 0;
    if (out_valid) out_valid[r] = any ? 1 : 0;
  }
}

extern "C" int dsx_window_ordered(
    DsxCtx* c, const uint32_t* perm, int64_t n, const uint64_t* pcode_sorted,
    const uint64_t* fcode_sorted, int func, const DsxColumn* v_or_null,
    int64_t offset, int64_t def_bits, int has_def, int out_dtype,
    void** out_data, uint8_t** out_valid, int want_valid) {
  *out_data = nullptr;
  *out_valid = nullptr;
  int sz = rj_dtype_size(out_dtype);
  int rc = pool_alloc(c, (n > 0 ? n : 1) * sz, out_data);
  if (rc) return rc;
  if (want_valid) {
    rc = pool_alloc(c, (n > 0 ? n : 1), (void**)out_valid);
    if (rc) return rc;
  }
  if (n == 0) return 0;
  // boundary starts via mark + the filter compaction (order-preserving).
  // marks live in POOL memory — dsx_filter reuses the scratch arena for
  // its own mask/counts and would clobber them there
  void* marks_p = nullptr;
  rc = pool_alloc(c, n, &marks_p);
  if (rc) return rc;
  uint8_t* marks = (uint8_t*)marks_p;
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  DsxInstr prog[1] = {{DSX_OP_COL, 0, 0}};
  DsxColumn mc{marks, nullptr, n, DSX_BOOL8};
  uint32_t* starts_p = nullptr;
  uint32_t* starts_f = nullptr;
  int64_t np_ = 0, nf = 0;
  hipLaunchKernelGGL(k_win_mark, dim3(grid), dim3(BLOCK), 0, c->stream,
                     pcode_sorted, n, marks);
  rc = dsx_filter(c, prog, 1, &mc, 1, n, &starts_p, &np_);
  if (rc) return rc;
  bool need_f = func == DSX_WIN_RANK || func == DSX_WIN_DENSERANK ||
                func >= DSX_WIN_RSUM;
  if (need_f) {
    hipLaunchKernelGGL(k_win_mark, dim3(grid), dim3(BLOCK), 0, c->stream,
                       fcode_sorted, n, marks);
    rc = dsx_filter(c, prog, 1, &mc, 1, n, &starts_f, &nf);
    if (rc) {
      pool_release(c, starts_p);
      return rc;
    }
  }
  DsxColumn v{};
  if (v_or_null) v = *v_or_null;
  if (func < DSX_WIN_RSUM) {
    ProfScope ps(c, "k_win_pos");
    hipLaunchKernelGGL(k_win_pos, dim3(grid), dim3(BLOCK), 0, c->stream,
                       perm, n, starts_p, np_, starts_f, nf, func, v,
                       offset, def_bits, has_def, *out_data,
                       want_valid ? *out_valid : nullptr);
  } else {
    void* cum_p = nullptr;
    void* cnt_p = nullptr;
    rc = pool_alloc(c, n * 8, &cum_p);
    if (!rc) rc = pool_alloc(c, n * 8, &cnt_p);
    if (rc) return rc;
    {
      ProfScope ps(c, "k_win_scan");
      hipLaunchKernelGGL(k_win_scan, dim3((uint32_t)np_), dim3(256), 0,
                         c->stream, perm, starts_p, np_, n, func, v,
                         (double*)cum_p, (int64_t*)cnt_p);
    }
    {
      ProfScope ps(c, "k_win_peer");
      hipLaunchKernelGGL(k_win_peer, dim3(grid), dim3(BLOCK), 0, c->stream,
                         perm, n, starts_f, nf, starts_p, np_,
                         (const double*)cum_p, (const int64_t*)cnt_p, func,
                         out_dtype == DSX_F64 ? 1 : 0, *out_data,
                         want_valid ? *out_valid : nullptr);
    }
    pool_release(c, cum_p);
    pool_release(c, cnt_p);
  }
  pool_release(c, marks_p);
  pool_release(c, starts_p);
  if (starts_f) pool_release(c, starts_f);
  HIP_TRY(hipGetLastError());
  return 0;
}
