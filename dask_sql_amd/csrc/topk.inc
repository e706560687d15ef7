// topk.inc — dsx_topk_rows: the candidate rows of ORDER BY ... LIMIT k picked
// on the device and brought to the host with ONE wait (reference
// physical/utils/sort.py:9-34 topk_sort: nsmallest / nlargest on the primary
// key). Included from dsxhip.hip; the host/device arithmetic is
// topk_select.h.
//
// MSB-first radix select over the order code of the primary key: pass p
// histograms digit p of the rows whose higher digits equal the prefix chosen
// so far (k_topk_hist, per-block LDS histogram, one global atomic per
// non-zero bin), a one-block kernel picks the bucket of the k-th row from the
// finished histogram (k_topk_pick) and stops the select as soon as every row
// at or before that bucket fits the candidate cap. k_topk_emit then writes
// those rows — row id, every column's value and validity byte — into one
// packed buffer that a single D2H copy brings to a pinned host buffer. All
// launches are queued back to back; a pass after "done" returns at once. The
// host trims the (at most cap) rows to the exact set {key at or before the
// k-th row's key}.

#include "topk_select.h"

struct TopkState {      // device words, zeroed by the call's one memset
  uint64_t prefix;      // digits chosen so far, in place; lower bits 0
  uint32_t want;        // rank of the k-th row inside the prefix (1-based)
  uint32_t taken;       // rows before the prefix
  uint32_t done;        // later passes return at once
  uint32_t status;      // 0 running, 1 selected, 2 not applicable
  uint32_t pass;        // pass whose bucket ended the select
  uint32_t na;          // NULL / NaN primary keys (counted in pass 0)
  uint32_t count;       // emit slot counter
  uint32_t pad[7];
};
static_assert(sizeof(TopkState) == 64, "TopkState is the 64-byte header");

#define TOPK_ROWS_PER_BLOCK 4096  // a block must outweigh its 2048-bin flush

// order code of row r's primary key; false for NULL / NaN
__device__ __forceinline__ bool topk_row_code(const void* data,
                                              const uint8_t* validity,
                                              int dtype, int desc, int64_t r,
                                              uint64_t& code) {
  if (validity && !validity[r]) return false;
  switch (dtype) {
    case DSX_F64:
      return dsx_topk_code_f64(((const double*)data)[r], desc, &code);
    case DSX_I64:
      code = dsx_topk_code_i64(((const int64_t*)data)[r], desc);
      return true;
    case DSX_I32:
      code = dsx_topk_code_i64(((const int32_t*)data)[r], desc);
      return true;
    default:  // DSX_I8
      code = dsx_topk_code_i64(((const int8_t*)data)[r], desc);
      return true;
  }
}

__global__ void __launch_bounds__(BLOCK)
k_topk_hist(const void* data, const uint8_t* validity, int dtype, int desc,
            int64_t n, int pass, TopkState* st, uint32_t* hist) {
  __shared__ uint32_t s_h[DSX_TOPK_BINS];
  __shared__ uint32_t s_na;
  if (st->done) return;  // uniform: written by an earlier kernel
  uint64_t prefix = st->prefix;
  for (int b = threadIdx.x; b < DSX_TOPK_BINS; b += BLOCK) s_h[b] = 0;
  if (threadIdx.x == 0) s_na = 0;
  __syncthreads();
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    uint64_t code;
    if (!topk_row_code(data, validity, dtype, desc, r, code)) {
      if (pass == 0) atomicAdd(&s_na, 1u);
      continue;
    }
    if (dsx_topk_in_prefix(code, prefix, pass))
      atomicAdd(&s_h[dsx_topk_digit(code, pass)], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < DSX_TOPK_BINS; b += BLOCK)
    if (s_h[b]) atomicAdd(&hist[b], s_h[b]);
  if (threadIdx.x == 0 && s_na) atomicAdd(&st->na, s_na);
}

// one block: bucket of the k-th row out of pass `pass`'s finished histogram.
// Thread t owns bins [8t, 8t+8); a block scan of the 256 sums finds the
// owner of the wanted rank, which runs dsx_topk_pick over its own bins.
__global__ void __launch_bounds__(BLOCK)
k_topk_pick(const uint32_t* hist, int pass, uint32_t k, uint32_t cap,
            TopkState* st) {
  constexpr int PER = DSX_TOPK_BINS / BLOCK;
  __shared__ uint32_t s_h[DSX_TOPK_BINS];
  __shared__ uint32_t s_scan[BLOCK];
  __shared__ int s_found;
  uint32_t done = st->done, na = st->na;
  uint32_t want = pass == 0 ? k : st->want;
  uint32_t taken = pass == 0 ? 0 : st->taken;
  uint64_t prefix = st->prefix;
  if (threadIdx.x == 0) s_found = 0;
  __syncthreads();  // every thread has read the state before any write
  if (done) return;
  if (na) {  // NULL / NaN primary key: the caller's host path orders those
    if (threadIdx.x == 0) {
      st->status = 2;
      st->done = 1;
    }
    return;
  }
  for (int b = threadIdx.x; b < DSX_TOPK_BINS; b += BLOCK) s_h[b] = hist[b];
  __syncthreads();
  const uint32_t* mine = &s_h[threadIdx.x * PER];
  uint32_t sum = 0;
  for (int i = 0; i < PER; i++) sum += mine[i];
  s_scan[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < BLOCK; d <<= 1) {  // inclusive Hillis-Steele scan
    uint32_t v = threadIdx.x >= d ? s_scan[threadIdx.x - d] : 0;
    __syncthreads();
    s_scan[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t inc = s_scan[threadIdx.x], exc = inc - sum;
  if (exc < want && want <= inc) {  // exactly one thread
    uint32_t before;
    int fin;
    int b = dsx_topk_pick(mine, PER, want - exc, taken + exc, cap, &before,
                          &fin);
    uint32_t digit = threadIdx.x * PER + b;
    st->prefix = prefix | ((uint64_t)digit << dsx_topk_shift(pass));
    st->want = want - exc - before;
    st->taken = taken + exc + before;
    st->pass = pass;
    if (fin) {
      st->status = 1;
      st->done = 1;
    } else if (pass == DSX_TOPK_PASSES - 1) {
      st->status = 2;  // the k-th key's exact ties do not fit the cap
      st->done = 1;
    }
    s_found = 1;
  }
  __syncthreads();
  if (threadIdx.x == 0 && !s_found) {  // fewer than k keyed rows
    st->status = 2;
    st->done = 1;
  }
}

__global__ void __launch_bounds__(BLOCK)
k_topk_emit(const void* data, const uint8_t* validity, int dtype, int desc,
            int64_t n, TopkState* st, JoinMatArg M, uint32_t* out_rowid,
            uint32_t cap, unsigned int* dbg) {
  if (st->status != 1) return;
  uint64_t prefix = st->prefix;
  int pass = (int)st->pass;
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    uint64_t code;
    if (!topk_row_code(data, validity, dtype, desc, r, code)) continue;
    if (!dsx_topk_at_or_before(code, prefix, pass)) continue;
    uint32_t o = atomicAdd(&st->count, 1u);
    if (o >= cap) {
      atomicOr(dbg, 4u);
      continue;
    }
    out_rowid[o] = (uint32_t)r;
    jm_write(M, (int64_t)o, r, 0u);
  }
}

static bool topk_enabled_dtype(int dtype) {
  return dtype == DSX_I64 || dtype == DSX_F64 || dtype == DSX_I32 ||
         dtype == DSX_F32 || dtype == DSX_I8;
}

static int topk_esz(int dtype) {
  return dtype == DSX_I64 || dtype == DSX_F64 ? 8
         : dtype == DSX_I32 || dtype == DSX_F32 ? 4 : 1;
}

extern "C" int dsx_topk_rows(DsxCtx* c, const DsxColumn* cols, int ncols,
                             int key_col, int desc, int64_t n, int64_t k,
                             int64_t cap, const void** out_host,
                             int64_t* out_offsets, int64_t* out_count) {
  *out_host = nullptr;
  *out_count = 0;
  if (ncols < 1 || ncols > DSX_MAX_COLS || key_col < 0 || key_col >= ncols)
    FAIL(-3, "topk_rows takes 1..%d columns and a key among them",
         DSX_MAX_COLS);
  if (n < 1 || n > 0xFFFFFFFEll) FAIL(-3, "topk_rows: n out of range");
  if (k < 1 || k > n || cap < 1 || cap > (1 << 20))
    FAIL(-3, "topk_rows: k or cap out of range");
  for (int i = 0; i < ncols; i++)
    if (!topk_enabled_dtype(cols[i].dtype) || cols[i].len < n)
      FAIL(-3, "topk_rows: column %d has an unsupported dtype or is short", i);
  const DsxColumn& key = cols[key_col];
  if (key.dtype == DSX_F32) FAIL(-3, "topk_rows: f32 primary key");

  // packed output: header, row ids, then per column values and validity
  // bytes, every part 8-byte aligned
  auto al8 = [](int64_t x) { return (x + 7) / 8 * 8; };
  int64_t off = sizeof(TopkState);
  out_offsets[0] = off;
  off += al8(cap * 4);
  for (int i = 0; i < ncols; i++) {
    out_offsets[1 + 2 * i] = off;
    off += al8(cap * topk_esz(cols[i].dtype));
    out_offsets[2 + 2 * i] = -1;
    if (cols[i].validity) {
      out_offsets[2 + 2 * i] = off;
      off += al8(cap);
    }
  }
  int64_t out_bytes = off;
  int64_t hist_bytes = (int64_t)DSX_TOPK_PASSES * DSX_TOPK_BINS * 4;
  int rc = ensure_scratch(c, hist_bytes + out_bytes);
  if (rc) return rc;
  if (c->topk_pinned_bytes < out_bytes) {
    if (c->topk_pinned) hipHostFree(c->topk_pinned);
    c->topk_pinned = nullptr;
    c->topk_pinned_bytes = 0;
    int64_t want = out_bytes + out_bytes / 2;
    HIP_TRY(hipHostMalloc(&c->topk_pinned, want));
    c->topk_pinned_bytes = want;
  }
  uint32_t* d_hist = (uint32_t*)c->scratch;
  char* d_out = (char*)c->scratch + hist_bytes;
  TopkState* d_st = (TopkState*)d_out;
  // histograms of all passes and the header, adjacent: one memset
  HIP_TRY(hipMemsetAsync(d_hist, 0, hist_bytes + sizeof(TopkState),
                         c->stream));
  JoinMatArg M{};
  M.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    M.src[i] = cols[i].data;
    M.srcv[i] = cols[i].validity;
    M.dst[i] = d_out + out_offsets[1 + 2 * i];
    M.dstv[i] = cols[i].validity
                    ? (uint8_t*)(d_out + out_offsets[2 + 2 * i]) : nullptr;
    M.dtype[i] = cols[i].dtype;
    M.side[i] = 0;
  }
  int grid = (int)min((int64_t)MAX_GRID,
                      (n + TOPK_ROWS_PER_BLOCK - 1) / TOPK_ROWS_PER_BLOCK);
  {
    ProfScope ps(c, "k_topk_select");
    for (int p = 0; p < DSX_TOPK_PASSES; p++) {
      uint32_t* h = d_hist + (int64_t)p * DSX_TOPK_BINS;
      hipLaunchKernelGGL(k_topk_hist, dim3(grid), dim3(BLOCK), 0, c->stream,
                         key.data, key.validity, key.dtype, desc, n, p, d_st,
                         h);
      hipLaunchKernelGGL(k_topk_pick, dim3(1), dim3(BLOCK), 0, c->stream, h,
                         p, (uint32_t)k, (uint32_t)cap, d_st);
    }
  }
  {
    ProfScope ps(c, "k_topk_emit");
    hipLaunchKernelGGL(k_topk_emit, dim3(grid), dim3(BLOCK), 0, c->stream,
                       key.data, key.validity, key.dtype, desc, n, d_st, M,
                       (uint32_t*)(d_out + out_offsets[0]), (uint32_t)cap,
                       c->dbg_flag);
  }
  HIP_TRY(hipGetLastError());
  char* h_out = (char*)c->topk_pinned;
  HIP_TRY(hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  TopkState st;
  memcpy(&st, h_out, sizeof(st));
  if (st.status != 1) {
    rc = dbg_check(c, "dsx_topk_rows");
    return rc ? rc : DSX_NOT_APPLICABLE;
  }
  if (st.count > (uint64_t)cap || st.count < (uint64_t)k)
    FAIL(-9, "topk_rows: %u candidates for k=%lld cap=%lld", st.count,
         (long long)k, (long long)cap);
  // trim the bucket to the exact set: rows whose key is at or before the
  // k-th row's key (an early stop took the whole bucket)
  int64_t cnt = st.count;
  std::vector<uint64_t> codes(cnt);
  const char* kd = h_out + out_offsets[1 + 2 * key_col];
  for (int64_t i = 0; i < cnt; i++) {
    switch (key.dtype) {
      case DSX_F64:
        dsx_topk_code_f64(((const double*)kd)[i], desc, &codes[i]);
        break;
      case DSX_I64:
        codes[i] = dsx_topk_code_i64(((const int64_t*)kd)[i], desc);
        break;
      case DSX_I32:
        codes[i] = dsx_topk_code_i64(((const int32_t*)kd)[i], desc);
        break;
      default:
        codes[i] = dsx_topk_code_i64(((const int8_t*)kd)[i], desc);
    }
  }
  std::vector<uint8_t> keep(cnt);
  dsx_topk_trim(codes.data(), cnt, k, keep.data());
  int64_t w = 0;
  uint32_t* rid = (uint32_t*)(h_out + out_offsets[0]);
  for (int64_t i = 0; i < cnt; i++) {
    if (!keep[i]) continue;
    if (w != i) {
      rid[w] = rid[i];
      for (int j = 0; j < ncols; j++) {
        int esz = topk_esz(cols[j].dtype);
        char* d = h_out + out_offsets[1 + 2 * j];
        memcpy(d + w * esz, d + i * esz, esz);
        if (out_offsets[2 + 2 * j] >= 0) {
          char* v = h_out + out_offsets[2 + 2 * j];
          v[w] = v[i];
        }
      }
    }
    w++;
  }
  *out_host = h_out;
  *out_count = w;
  return dbg_check(c, "dsx_topk_rows");
}
