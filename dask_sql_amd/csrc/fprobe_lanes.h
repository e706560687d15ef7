// fprobe_lanes.h — handing the set bits of a batch of filter-probe mask words
// to the lanes of a wave, so that lanes stay dense at any match density. One
// definition for the kernels of dsxhip.hip (k_fprobe_emit, k_fprobe_agg) and
// the generated j_fprobe_agg (group_join.inc pastes this text into its
// source), by the convention of join_filter.h: the functions are written
// inside DSX_FPL_CODE(...) so that a second include can stringify them. Hence
// no preprocessor directive inside the parentheses.
//
// A wave holds a batch of 64 mask words, one per lane (m), their popcounts
// (cnt) and the inclusive prefix of those (inc = fp_wave_inclusive(cnt)); the
// batch total is inc of lane 63. fp_batch_row finds the probe row of the
// batch's j-th (0-based) set bit; wb is the batch's first word. Every lane
// must call it (the shuffles stay outside divergent code): lanes past the
// batch total pass the last row's j and ignore the answer.
#ifndef DSX_FPL_CODE
#define DSX_FPL_CODE(...) __VA_ARGS__
#endif

DSX_FPL_CODE(
/* position of the k-th (0-based) set bit of m; k < popcount(m) */
__device__ __forceinline__ int fp_select_bit(unsigned long long m, int k) {
  int pos = 0;
  _Pragma("unroll")
  for (int w = 32; w > 0; w >>= 1) {
    int cnt = __popcll(m & ((1ull << w) - 1));
    if (k >= cnt) {
      k -= cnt;
      m >>= w;
      pos += w;
    }
  }
  return pos;
}

/* inclusive prefix over the wave of a lane's count */
__device__ __forceinline__ int fp_wave_inclusive(int cnt) {
  int lane = (int)(threadIdx.x & 63);
  int inc = cnt;
  for (int d = 1; d < 64; d <<= 1) {
    int t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  return inc;
}

__device__ __forceinline__ long long fp_batch_row(unsigned long long m,
                                                  int inc, int cnt,
                                                  long long wb, int j) {
  int L = 0;  /* smallest lane whose inclusive count exceeds j */
  for (int step = 32; step > 0; step >>= 1) {
    int v = __shfl(inc, L + step - 1, 64);
    if (v <= j) L += step;
  }
  unsigned int m_lo = (unsigned int)m;
  unsigned int m_hi = (unsigned int)(m >> 32);
  unsigned long long mL =
      ((unsigned long long)(unsigned int)__shfl((int)m_hi, L, 64) << 32) |
      (unsigned int)__shfl((int)m_lo, L, 64);
  int k = j - __shfl(inc - cnt, L, 64);
  return (wb + L) * 64 + fp_select_bit(mL, k);
}
)
