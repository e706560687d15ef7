// sort_code.h — order-preserving u64 code of one f64 ORDER BY key
// (DsxKeySpec mode bit 8; bit 2 = DESC, bit 4 = NULLS LAST). Plain C++ so
// the host test can compile it alone with g++; radix_sort.inc uses it on
// the device.
//
// Unsigned comparison of the codes, ties broken by ascending row id, is the
// order of pandas sort_values(kind="mergesort", ascending=..., na_position=
// ...) (reference physical/utils/sort.py:36-60):
//   - NULL and NaN take the null slot (~0 with NULLS LAST, 0 with NULLS
//     FIRST) in either direction — pandas places both at na_position;
//   - -0.0 and +0.0 tie;
//   - no real value reaches 0 or ~0 (only NaN bit patterns map there), so
//     the null slot never collides.
#ifndef DSX_SORT_CODE_H
#define DSX_SORT_CODE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define DSX_HD __host__ __device__
#else
#define DSX_HD
#endif

DSX_HD static inline uint64_t dsx_f64_order_code(double x, int valid,
                                                 int mode) {
  if (!valid || x != x) return (mode & 4) ? ~0ull : 0ull;
  if (x == 0.0) x = 0.0;  // -0.0 → +0.0
  uint64_t b;
  __builtin_memcpy(&b, &x, 8);
  uint64_t u = b ^ ((b >> 63) ? ~0ull : (1ull << 63));
  return (mode & 2) ? ~u : u;
}

#endif  // DSX_SORT_CODE_H
