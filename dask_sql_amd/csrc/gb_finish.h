// gb_finish.h — group-by output columns from (packed key code, raw aggregate
// value, non-NULL count): the arithmetic of the finish kernel (dsxhip.hip
// k_gb_finish, entry dsx_hash_groupby_cols). Plain C++ so the host test can
// compile it alone with g++; the kernel uses the same functions on the device.
//
// Keys invert pack_key (dsxhip.hip): code = Σ_j part_j · stride_j with
// part_j = value − min (+1 when the key is nullable, slot 0 = NULL), and
// stride_j = Π_{i<j} space_i, space = range + nullable. So
//   part_j = (code / stride_j) % space_j.
// Mode 1 (a single f64 key): code = canonical bits + 1, code 0 = NaN/NULL.
//
// Aggregates: COUNT is the count; SUM/MIN/MAX are NULL when no non-NULL input
// reached the group (custom_sum min_count=1, reference aggregate.py:486-493);
// AVG = sum / count. MIN/MAX accumulate in an order-preserving u64 transform
// (atomicMin/Max on unsigned) that is undone here.
#ifndef DSX_GB_FINISH_H
#define DSX_GB_FINISH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define DSX_GBF_HD __host__ __device__
#else
#define DSX_GBF_HD
#endif

// finalize kinds (DsxGbFinishKind in include/dsxhip.h)
#define DSX_GBF_COUNT 0
#define DSX_GBF_SUM_I 1
#define DSX_GBF_SUM_F 2
#define DSX_GBF_MIN_I 3
#define DSX_GBF_MAX_I 4
#define DSX_GBF_MIN_F 5
#define DSX_GBF_MAX_F 6
#define DSX_GBF_AVG 7

// one key's unpack plan; uniform across a launch
struct DsxGbKeyPlan {
  uint64_t stride;       // Π space of the keys before this one
  uint64_t space;        // range + nullable (≥ 1)
  int64_t min;
  int32_t stride_shift;  // log2(stride) when a power of two, else −1
  int32_t space_shift;   // log2(space) when a power of two, else −1
  int32_t nullable;
  int32_t mode;          // 0 radix-packed integer, 1 f64 bit pattern
};

// log2(x) when x is a power of two, else −1
DSX_GBF_HD static inline int32_t dsx_gbf_log2_exact(uint64_t x) {
  if (x == 0 || (x & (x - 1)) != 0) return -1;
  int32_t s = 0;
  while ((x >> s) != 1) s++;
  return s;
}

DSX_GBF_HD static inline DsxGbKeyPlan dsx_gbf_key_plan(uint64_t stride,
                                                       uint64_t space,
                                                       int64_t min,
                                                       int nullable,
                                                       int mode) {
  DsxGbKeyPlan p;
  p.stride = stride;
  p.space = space;
  p.min = min;
  p.stride_shift = dsx_gbf_log2_exact(stride);
  p.space_shift = dsx_gbf_log2_exact(space);
  p.nullable = nullable ? 1 : 0;
  p.mode = mode;
  return p;
}

// (code / stride) % space: nothing for a space of 1, shift and mask for
// powers of two, a plain 64-bit divide for the rest
DSX_GBF_HD static inline uint64_t dsx_gbf_key_part(uint64_t code,
                                                   const DsxGbKeyPlan& p) {
  if (p.space == 1) return 0;
  uint64_t q = p.stride_shift >= 0 ? (code >> p.stride_shift)
                                   : (code / p.stride);
  return p.space_shift >= 0 ? (q & (p.space - 1)) : (q % p.space);
}

// the key's value as 64 output bits (i64, or f64 bits in mode 1); returns 0
// for the NULL group, whose cell holds 0 (i64) or NaN (f64)
DSX_GBF_HD static inline int dsx_gbf_key_value(uint64_t code,
                                               const DsxGbKeyPlan& p,
                                               uint64_t* out_bits) {
  if (p.mode == 1) {
    if (code == 0) {
      *out_bits = 0x7FF8000000000000ull;  // quiet NaN, as k_eval writes
      return 0;
    }
    *out_bits = code - 1;
    return 1;
  }
  uint64_t part = dsx_gbf_key_part(code, p);
  if (p.nullable) {
    if (part == 0) {
      *out_bits = 0;
      return 0;
    }
    part -= 1;
  }
  *out_bits = part + (uint64_t)p.min;  // two's complement: min may be < 0
  return 1;
}

// inverse of the order-preserving f64 → u64 transform of the MIN/MAX
// accumulators (f64_ordered in dsxhip.hip)
DSX_GBF_HD static inline uint64_t dsx_gbf_f64_unordered_bits(uint64_t b) {
  return (b & 0x8000000000000000ull) ? (b & 0x7FFFFFFFFFFFFFFFull) : ~b;
}

// one aggregate cell from the accumulator's raw bits and the non-NULL input
// count; returns validity. `raw` is unused for COUNT.
DSX_GBF_HD static inline int dsx_gbf_finalize(int kind, uint64_t raw,
                                              uint64_t count,
                                              uint64_t* out_bits) {
  if (kind == DSX_GBF_COUNT) {
    *out_bits = count;
    return 1;
  }
  const bool f64_out = kind == DSX_GBF_SUM_F || kind == DSX_GBF_MIN_F ||
                       kind == DSX_GBF_MAX_F || kind == DSX_GBF_AVG;
  if (count == 0) {
    *out_bits = f64_out ? 0x7FF8000000000000ull : 0ull;
    return 0;
  }
  switch (kind) {
    case DSX_GBF_MIN_I:
    case DSX_GBF_MAX_I:
      *out_bits = raw ^ 0x8000000000000000ull;
      break;
    case DSX_GBF_MIN_F:
    case DSX_GBF_MAX_F:
      *out_bits = dsx_gbf_f64_unordered_bits(raw);
      break;
    case DSX_GBF_AVG: {
      double s;
      __builtin_memcpy(&s, &raw, 8);
      double q = s / (double)(int64_t)count;
      __builtin_memcpy(out_bits, &q, 8);
      break;
    }
    default:  // SUM_I, SUM_F: the accumulator's bits as they are
      *out_bits = raw;
  }
  return 1;
}

#endif  // DSX_GB_FINISH_H
