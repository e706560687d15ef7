// window_words.inc — partition / peer boundaries for window keys that do not
// pack into one code: float keys, more than DSX_MAX_KEYS keys, key spaces
// above 2^62 (reference rel/logical/window.py:212-428 groups the sorted frame
// with pandas groupby(dropna=False)). Included by dsxhip.hip after
// radix_sort.inc (shares the word parser, rsort_word_code and rsort_grid).
//
// The sort side is the dsx_sort_word chain. Here, per word of that chain:
//   k_win_mark_word  mark[i] |= code(perm[i]) != code(perm[i-1]) over sorted
//                    positions — the word's code is computed once per row, a
//                    lane takes its left neighbour's by a wave shuffle, lane
//                    0 of each wave computes the one halo code itself
// and once per boundary kind (partition, peer):
//   k_win_seg_count / k_win_seg_carry / k_win_seg_ids
//                    ids[i] = (marks in [0, i]) - 1 by a three-phase scan:
//                    per-block mark counts, a one-block exclusive scan of
//                    them, then each block numbers its own range
// The ids differ between adjacent sorted rows exactly at a boundary, which
// is all dsx_window_ordered / dsx_window_rows ask of pcode_sorted /
// fcode_sorted. No block waits on another; every loop is bounded.

__device__ __forceinline__ uint64_t win_word_code_at(
    const ColsArg& C, const KeyArg& K, int fcol, int fmode,
    const uint32_t* perm, int64_t i, int64_t n) {
  uint32_t r = perm ? perm[i] : (uint32_t)i;
  if ((int64_t)r >= n) return 0;  // a malformed perm reads nothing
  return rsort_word_code(C, K, fcol, fmode, (int64_t)r);
}

// Waves start at multiples of 64 (BLOCK and the grid stride are), so the
// halo rows are the sorted positions 64, 128, 192, ...
__global__ void __launch_bounds__(BLOCK) k_win_mark_word(
    ColsArg C, KeyArg K, int fcol, int fmode, int64_t n, const uint32_t* perm,
    uint8_t* marks, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  // grid-uniform trip count: tail lanes stay in every shuffle
  const int64_t ntiles = (n + stride - 1) / stride;
  for (int64_t t = 0; t < ntiles; t++) {
    const int64_t i = t * stride + (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < n;
    unsigned long long code = 0;
    if (live) code = win_word_code_at(C, K, fcol, fmode, perm, i, n);
    unsigned long long left = __shfl_up(code, 1);
    if (lane == 0 && live && i > 0)
      left = win_word_code_at(C, K, fcol, fmode, perm, i - 1, n);
    if (live) {
      const bool m = i == 0 || code != left;
      if (!accumulate) marks[i] = m ? 1 : 0;
      else if (m) marks[i] = 1;
    }
  }
}

// phase 1: marks in the block's row range
__global__ void __launch_bounds__(BLOCK) k_win_seg_count(
    const uint8_t* marks, int64_t n, int64_t* partial) {
  __shared__ int s_w[WAVES_PER_BLOCK];
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  int cnt = 0;  // n < 2^32: a thread sees < 2^24 rows, a wave < 2^30
  for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK)
    cnt += marks[i] != 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; w++) tot += s_w[w];
    partial[blockIdx.x] = tot;
  }
}

// phase 2 (one block): partial[] → its exclusive prefix in place, the grand
// total to *total. Thread t owns ceil(nparts / BLOCK) consecutive entries.
__global__ void __launch_bounds__(BLOCK) k_win_seg_carry(
    int64_t* partial, int nparts, int64_t* total) {
  __shared__ int64_t s_sum[BLOCK];
  const int t = threadIdx.x;
  const int per = (nparts + BLOCK - 1) / BLOCK;
  const int b0 = t * per;
  int64_t sum = 0;
  for (int k = 0; k < per; k++)
    if (b0 + k < nparts) sum += partial[b0 + k];
  s_sum[t] = sum;
  __syncthreads();
  for (int d = 1; d < BLOCK; d <<= 1) {
    int64_t pv = t >= d ? s_sum[t - d] : 0;
    __syncthreads();
    s_sum[t] += pv;
    __syncthreads();
  }
  int64_t run = s_sum[t] - sum;
  for (int k = 0; k < per; k++) {
    if (b0 + k < nparts) {
      int64_t v = partial[b0 + k];
      partial[b0 + k] = run;
      run += v;
    }
  }
  if (t == BLOCK - 1) *total = s_sum[t];
}

// phase 3: the block walks its range tile by tile in order; a lane ranks
// among the marks of its wave by ballot, waves chain through LDS
__global__ void __launch_bounds__(BLOCK) k_win_seg_ids(
    const uint8_t* marks, int64_t n, const int64_t* carry, uint64_t* ids) {
  __shared__ int s_w[WAVES_PER_BLOCK];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  int64_t base = carry[blockIdx.x];  // marks before lo
  // block-uniform trip count: the body has barriers
  const int64_t ntiles = (hi - lo + BLOCK - 1) / BLOCK;
  for (int64_t t = 0; t < ntiles; t++) {
    const int64_t i = lo + t * BLOCK + threadIdx.x;
    const bool live = i < hi;
    const bool m = live && marks[i] != 0;  // tail lanes vote false
    const uint64_t b = __ballot(m);
    const int incl = __popcll(b & ((2ull << lane) - 1ull));
    if (lane == 0) s_w[wid] = __popcll(b);
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; w++) {
      int cw = s_w[w];
      if (w < wid) before += cw;
      tot += cw;
    }
    if (live) ids[i] = (uint64_t)(base + before + incl - 1);
    base += tot;
    __syncthreads();  // s_w is rewritten by the next tile
  }
}

extern "C" int dsx_window_mark_word(DsxCtx* c, const DsxColumn* cols,
                                    int ncols, const DsxKeySpec* keys,
                                    int nkeys, int64_t n, const uint32_t* perm,
                                    uint8_t** marks_inout) {
  uint8_t* given = *marks_inout;
  *marks_inout = nullptr;
  KeyArg K;
  ColsArg C;
  int fcol, fmode;
  int rc = rsort_parse_word(cols, ncols, keys, nkeys, n, K, fcol, fmode, C);
  if (rc) return rc;
  uint8_t* marks = given;
  if (!marks) {
    rc = pool_alloc(c, n > 0 ? n : 1, (void**)&marks);
    if (rc) return rc;
  }
  if (n > 0) {
    ProfScope ps(c, "k_win_mark_word");
    hipLaunchKernelGGL(k_win_mark_word, dim3(rsort_grid(n)), dim3(BLOCK), 0,
                       c->stream, C, K, fcol, fmode, n, perm, marks,
                       given ? 1 : 0);
  }
  hipError_t e = n > 0 ? hipGetLastError() : hipSuccess;
  if (e != hipSuccess) {
    if (!given) {
      (void)hipStreamSynchronize(c->stream);  // nothing in flight on release
      pool_release(c, marks);
    }
    FAIL(-1, "k_win_mark_word launch: %s", hipGetErrorString(e));
  }
  *marks_inout = marks;
  return 0;
}

static int win_seg_ids_run(DsxCtx* c, const uint8_t* marks, int64_t n,
                           uint64_t* ids, int64_t* out_segments) {
  const int grid = rsort_grid(n);
  int rc = ensure_scratch(c, ((int64_t)grid + 1) * 8);
  if (rc) return rc;
  int64_t* partial = (int64_t*)c->scratch;
  int64_t* total = partial + grid;
  {
    ProfScope ps(c, "k_win_seg_ids");
    hipLaunchKernelGGL(k_win_seg_count, dim3(grid), dim3(BLOCK), 0, c->stream,
                       marks, n, partial);
    hipLaunchKernelGGL(k_win_seg_carry, dim3(1), dim3(BLOCK), 0, c->stream,
                       partial, grid, total);
    hipLaunchKernelGGL(k_win_seg_ids, dim3(grid), dim3(BLOCK), 0, c->stream,
                       marks, n, (const int64_t*)partial, ids);
  }
  int64_t h_total = 0;
  HIP_TRY(hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipGetLastError());
  if (out_segments) *out_segments = h_total;
  return 0;
}

extern "C" int dsx_window_seg_ids(DsxCtx* c, const uint8_t* marks, int64_t n,
                                  uint64_t** out_ids, int64_t* out_segments) {
  *out_ids = nullptr;
  if (out_segments) *out_segments = 0;
  if (n < 0 || n > 0xFFFFFFFEll)
    FAIL(-3, "dsx_window_seg_ids: bad row count %lld", (long long)n);
  if (n > 0 && !marks) FAIL(-3, "dsx_window_seg_ids: no marks");
  int rc = pool_alloc(c, (n > 0 ? n : 1) * 8, (void**)out_ids);
  if (rc || n == 0) return rc;
  rc = win_seg_ids_run(c, marks, n, *out_ids, out_segments);
  if (rc) {
    (void)hipStreamSynchronize(c->stream);  // nothing in flight on release
    pool_release(c, *out_ids);
    *out_ids = nullptr;
    if (out_segments) *out_segments = 0;
  }
  return rc;
}
