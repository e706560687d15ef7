// radix_sort.inc — stable LSD radix sort over 64-bit order codes: the
// skew-proof, width-independent half of ORDER BY (reference
// physical/utils/sort.py:36-60 sorts key by key, last to first, with pandas
// mergesort). Included by dsxhip.hip.
//
// dsx_sort_word sorts a row-id sequence stably by ONE u64 "word": either up
// to DSX_MAX_KEYS integer-kind keys packed exactly like dsx_sort_perm
// (pack_key), or one float key coded by dsx_f64_order_code (mode bit 8).
// Because the sort is stable, the caller chains words least significant
// first and gets composite keys of any width; no bucket can overflow, so
// skew costs nothing.
//
//   k_rsort_codes    code[i], rid[i] for row perm_in[i] + the global 8×256
//                    digit totals; digits constant across all rows are
//                    skipped (one 16-KB D2H + sync decides)
//   per remaining digit, least significant first:
//   k_rsort_hist     per-block 256-bin histogram
//   k_gbpart_scan / k_gbpart_bases (nb = 256)
//   k_rsort_scatter  block walks its range tile by tile IN ORDER; within a
//                    tile lanes rank among their digit peers by ballot
//
// No block waits on another; every loop is bounded.

#include "sort_code.h"

#define RSORT_RADIX 256
#define RSORT_DIGITS 8
static_assert(BLOCK == RSORT_RADIX, "one thread per digit bin");

// one 256-bin LDS increment per active lane; a wave whose active lanes all
// hold the same digit (constant high bytes, skewed keys) adds once
__device__ __forceinline__ void rsort_count(uint32_t* s_bins, uint32_t dg,
                                            bool active, uint64_t act,
                                            int lane) {
  uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)dg);
  uint64_t same = __ballot(active && dg == first);
  if (same == act) {
    // active lanes are a prefix of the wave, so lane 0 is active here
    if (lane == 0) atomicAdd(&s_bins[first], (uint32_t)__popcll(act));
  } else if (active) {
    atomicAdd(&s_bins[dg], 1u);
  }
}

// the word's u64 order code of row r: one float key (fcol >= 0) or the
// packed integer-kind keys. Shared with k_win_mark_word (window_words.inc),
// which must tell rows apart exactly where the sort does.
__device__ __forceinline__ uint64_t rsort_word_code(const ColsArg& C,
                                                    const KeyArg& K, int fcol,
                                                    int fmode, int64_t r) {
  if (fcol >= 0) {
    Slot v;
    bool valid;
    vm_load_col(C, fcol, r, v, valid);
    return dsx_f64_order_code(v.f, valid ? 1 : 0, fmode);
  }
  return pack_key(K, C, r);
}

__global__ void __launch_bounds__(BLOCK) k_rsort_codes(
    ColsArg C, int64_t n, const KeyArg* Kp, int fcol, int fmode,
    const uint32_t* perm_in, uint64_t* code_out, uint32_t* rid_out,
    unsigned long long* dig_totals) {
  __shared__ uint32_t s_hist[RSORT_DIGITS * RSORT_RADIX];
  for (int i = threadIdx.x; i < RSORT_DIGITS * RSORT_RADIX; i += BLOCK)
    s_hist[i] = 0;
  __syncthreads();
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  const int lane = threadIdx.x & 63;
  for (int64_t base = lo; base < hi; base += BLOCK) {
    int64_t i = base + threadIdx.x;
    bool active = i < hi;
    uint64_t act = __ballot(active);
    if (act == 0) continue;  // wave-uniform
    uint64_t code = 0;
    if (active) {
      uint32_t r = perm_in ? perm_in[i] : (uint32_t)i;
      code = rsort_word_code(C, *Kp, fcol, fmode, (int64_t)r);
      code_out[i] = code;
      rid_out[i] = r;
    }
#pragma unroll
    for (int d = 0; d < RSORT_DIGITS; d++)
      rsort_count(s_hist + d * RSORT_RADIX, (uint32_t)(code >> (8 * d)) & 255u,
                  active, act, lane);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < RSORT_DIGITS * RSORT_RADIX; i += BLOCK) {
    uint32_t v = s_hist[i];
    if (v) atomicAdd(&dig_totals[i], (unsigned long long)v);
  }
}

__global__ void __launch_bounds__(BLOCK) k_rsort_hist(
    const uint64_t* code, int64_t n, int shift, int64_t* hist) {
  __shared__ uint32_t s_hist[RSORT_RADIX];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  const int lane = threadIdx.x & 63;
  for (int64_t base = lo; base < hi; base += BLOCK) {
    int64_t i = base + threadIdx.x;
    bool active = i < hi;
    uint64_t act = __ballot(active);
    if (act == 0) continue;
    uint32_t dg = active ? (uint32_t)(code[i] >> shift) & 255u : 0u;
    rsort_count(s_hist, dg, active, act, lane);
  }
  __syncthreads();
  hist[(int64_t)blockIdx.x * RSORT_RADIX + threadIdx.x] =
      (int64_t)s_hist[threadIdx.x];
}

// hist[block][d] holds the block's exclusive offset inside digit d (after
// k_gbpart_scan), bases[d] the digit's absolute start. code_out == nullptr
// on the last pass: only row ids are written, straight into the result.
__global__ void __launch_bounds__(BLOCK) k_rsort_scatter(
    const uint64_t* code_in, const uint32_t* rid_in, int64_t n, int shift,
    const int64_t* hist, const int64_t* bases, uint64_t* code_out,
    uint32_t* rid_out) {
  __shared__ int64_t s_base[RSORT_RADIX];  // running destination per digit
  __shared__ uint32_t s_wcnt[WAVES_PER_BLOCK][RSORT_RADIX];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  s_base[tid] = bases[tid] + hist[(int64_t)blockIdx.x * RSORT_RADIX + tid];
#pragma unroll
  for (int w = 0; w < WAVES_PER_BLOCK; w++) s_wcnt[w][tid] = 0;
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  // block-uniform trip count: the body has barriers
  const int64_t ntiles = (hi - lo + BLOCK - 1) / BLOCK;
  for (int64_t t = 0; t < ntiles; t++) {
    int64_t i = lo + t * BLOCK + tid;
    bool active = i < hi;
    uint64_t code = 0;
    uint32_t rid = 0;
    if (active) {
      code = code_in[i];
      rid = rid_in[i];
    }
    uint32_t dg = (uint32_t)(code >> shift) & 255u;
    // peer mask: active lanes of this wave with the same digit. Tail lanes
    // run every ballot with a false predicate and drop out of every mask
    // through the leading ballot of `active`.
    uint64_t peers = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      bool bit = (dg >> b) & 1u;
      uint64_t m = __ballot(active && bit);
      peers &= bit ? m : ~m;
    }
    int rank = __popcll(peers & ((1ull << lane) - 1ull));
    __syncthreads();  // s_wcnt zeroed / s_base advanced by the last tile
    if (active && rank == 0) s_wcnt[wid][dg] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (active) {
      int64_t o = s_base[dg] + rank;
#pragma unroll
      for (int w = 0; w < WAVES_PER_BLOCK; w++)
        if (w < wid) o += s_wcnt[w][dg];
      if ((uint64_t)o < (uint64_t)n) {  // holds by construction
        if (code_out) code_out[o] = code;
        rid_out[o] = rid;
      }
    }
    __syncthreads();
    // thread d owns digit d: advance its base, clear its counters (the same
    // cells it just read, so no barrier in between)
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; w++) {
      tot += s_wcnt[w][tid];
      s_wcnt[w][tid] = 0;
    }
    s_base[tid] += tot;
  }
}

// launch grid of the row passes; DSX_RSORT_GRID caps it (read per call —
// the test knob that lets a small input make one block walk several tiles)
static int rsort_grid(int64_t n) {
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  if (const char* e = getenv("DSX_RSORT_GRID")) {
    int g = atoi(e);
    if (g >= 1 && g < grid) grid = g;
  }
  return grid;
}

struct RsortBufs {
  void* code[2] = {nullptr, nullptr};
  void* rid[2] = {nullptr, nullptr};
};

static int rsort_run(DsxCtx* c, const ColsArg& C, const KeyArg& K, int fcol,
                     int fmode, int64_t n, const uint32_t* perm_in,
                     RsortBufs& B, uint32_t* out_perm) {
  int grid = rsort_grid(n);
  const int nb = RSORT_RADIX;
  const int64_t hist_b = (int64_t)grid * nb * 8;
  const int64_t dig_b = RSORT_DIGITS * RSORT_RADIX * 8;
  int64_t need = hist_b + nb * 8 + (nb + 2) * 8 + dig_b + sizeof(KeyArg) + 64;
  int rc = ensure_scratch(c, need);
  if (rc) return rc;
  char* base = (char*)c->scratch;
  int64_t* hist = (int64_t*)base;
  base += hist_b;
  int64_t* totals = (int64_t*)base;
  base += nb * 8;
  int64_t* bases = (int64_t*)base;
  base += (nb + 2) * 8;
  unsigned long long* d_dig = (unsigned long long*)base;
  base += dig_b;
  KeyArg* d_K = (KeyArg*)base;
  HIP_TRY(hipMemcpyAsync(d_K, &K, sizeof(KeyArg), hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipMemsetAsync(d_dig, 0, dig_b, c->stream));
  rc = pool_alloc(c, n * 8, &B.code[0]);
  if (rc) return rc;
  rc = pool_alloc(c, n * 4, &B.rid[0]);
  if (rc) return rc;
  {
    ProfScope ps(c, "k_rsort_codes");
    hipLaunchKernelGGL(k_rsort_codes, dim3(grid), dim3(BLOCK), 0, c->stream,
                       C, n, d_K, fcol, fmode, perm_in, (uint64_t*)B.code[0],
                       (uint32_t*)B.rid[0], d_dig);
  }
  static thread_local unsigned long long h_dig[RSORT_DIGITS * RSORT_RADIX];
  HIP_TRY(hipMemcpyAsync(h_dig, d_dig, dig_b, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // a digit whose every row falls in one bin cannot reorder anything
  int pass_digit[RSORT_DIGITS];
  int npass = 0;
  for (int d = 0; d < RSORT_DIGITS; d++) {
    bool constant = false;
    for (int v = 0; v < RSORT_RADIX; v++)
      if (h_dig[d * RSORT_RADIX + v] == (unsigned long long)n) constant = true;
    if (!constant) pass_digit[npass++] = d;
  }
  if (npass == 0) {
    HIP_TRY(hipMemcpyAsync(out_perm, B.rid[0], n * 4,
                           hipMemcpyDeviceToDevice, c->stream));
  }
  if (npass >= 2) {
    rc = pool_alloc(c, n * 8, &B.code[1]);
    if (rc) return rc;
    rc = pool_alloc(c, n * 4, &B.rid[1]);
    if (rc) return rc;
  }
  for (int p = 0; p < npass; p++) {
    const int shift = 8 * pass_digit[p];
    const int in = p & 1, out = in ^ 1;
    const bool last = p == npass - 1;
    {
      ProfScope ps(c, "k_rsort_hist");
      hipLaunchKernelGGL(k_rsort_hist, dim3(grid), dim3(BLOCK), 0, c->stream,
                         (const uint64_t*)B.code[in], n, shift, hist);
    }
    hipLaunchKernelGGL(k_gbpart_scan, dim3(nb / 8), dim3(BLOCK), 0, c->stream,
                       hist, grid, nb, totals);
    hipLaunchKernelGGL(k_gbpart_bases, dim3(1), dim3(1024), 0, c->stream,
                       totals, nb, bases);
    {
      ProfScope ps(c, "k_rsort_scatter");
      hipLaunchKernelGGL(k_rsort_scatter, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const uint64_t*)B.code[in],
                         (const uint32_t*)B.rid[in], n, shift, hist, bases,
                         last ? (uint64_t*)nullptr : (uint64_t*)B.code[out],
                         last ? out_perm : (uint32_t*)B.rid[out]);
    }
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

// validates one word (dsx_sort_word's contract) and fills the kernel
// arguments; -3 on a malformed spec, -4 on a key space above 2^62
static int rsort_parse_word(const DsxColumn* cols, int ncols,
                            const DsxKeySpec* keys, int nkeys, int64_t n,
                            KeyArg& K, int& fcol, int& fmode, ColsArg& C) {
  if (ncols < 1 || ncols > DSX_MAX_COLS || nkeys < 1 || nkeys > DSX_MAX_KEYS)
    FAIL(-3, "sort word spec");
  if (n < 0 || n > 0xFFFFFFFEll)
    FAIL(-3, "sort too large for u32 row ids");
  K = KeyArg{};
  K.nkeys = nkeys;
  fcol = -1;
  fmode = 0;
  uint64_t space = 1;
  for (int j = 0; j < nkeys; j++) {
    if (keys[j].col < 0 || keys[j].col >= ncols)
      FAIL(-3, "sort word key column out of range");
    if (keys[j].mode & 1) FAIL(-3, "f64-bits mode is not an ORDER BY mode");
    int dt = cols[keys[j].col].dtype;
    bool isf = dt == DSX_F64 || dt == DSX_F32;
    if (keys[j].mode & 8) {
      if (nkeys != 1) FAIL(-3, "a float key must be a word of its own");
      if (!isf) FAIL(-3, "mode bit 8 on a non-float column");
      fcol = keys[j].col;
      fmode = keys[j].mode;
      continue;
    }
    if (isf) FAIL(-3, "float column without mode bit 8");
    K.k[j] = keys[j];
    K.stride[j] = space;
    uint64_t range = (uint64_t)keys[j].range + (keys[j].nullable ? 1 : 0);
    if (keys[j].range <= 0 || range == 0) FAIL(-3, "empty key range");
    if (space > (1ull << 62) / range) FAIL(-4, "sort key space > 2^62");
    space *= range;
  }
  C = ColsArg{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    C.data[i] = cols[i].data;
    C.validity[i] = cols[i].validity;
    C.dtype[i] = cols[i].dtype;
  }
  return 0;
}

extern "C" int dsx_sort_word(DsxCtx* c, const DsxColumn* cols, int ncols,
                             const DsxKeySpec* keys, int nkeys, int64_t n,
                             const uint32_t* perm_in, uint32_t** out_perm) {
  *out_perm = nullptr;
  KeyArg K;
  ColsArg C;
  int fcol, fmode;
  int rc = rsort_parse_word(cols, ncols, keys, nkeys, n, K, fcol, fmode, C);
  if (rc) return rc;
  if (n == 0) return pool_alloc(c, 4, (void**)out_perm);
  rc = pool_alloc(c, n * 4, (void**)out_perm);
  if (rc) return rc;
  RsortBufs B;
  rc = rsort_run(c, C, K, fcol, fmode, n, perm_in, B, *out_perm);
  // nothing in flight on release
  if (rc) (void)hipStreamSynchronize(c->stream);
  for (int i = 0; i < 2; i++) {
    if (B.code[i]) pool_release(c, B.code[i]);
    if (B.rid[i]) pool_release(c, B.rid[i]);
  }
  if (rc) {
    pool_release(c, *out_perm);
    *out_perm = nullptr;
  }
  return rc;
}
