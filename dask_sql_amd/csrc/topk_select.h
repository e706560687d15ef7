// topk_select.h — host/device pieces of the ORDER BY ... LIMIT row selection
// (dsx_topk_rows, topk.inc). Plain C++ so the host test can compile it alone
// with g++, like sort_code.h.
//
// Two things live here:
//  - the order-preserving u64 code of the PRIMARY sort key: unsigned
//    comparison of the codes is the key order in the asked direction, smaller
//    code = earlier row. NULL and NaN are reported (return 0), not coded: a
//    frame that holds one is not selected on the device.
//  - the digit pick of the MSB-first radix select: given the histogram of one
//    digit over the rows that share the chosen prefix, which bucket holds the
//    row still wanted, how many rows lie before it, and whether everything up
//    to and including the bucket already fits the candidate cap.
#ifndef DSX_TOPK_SELECT_H
#define DSX_TOPK_SELECT_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "sort_code.h"

// 11-bit digits, most significant first: five full digits and a last one of
// 9 bits cover the 64-bit code in 6 passes; a histogram is 8 KB of LDS.
#define DSX_TOPK_DIGIT_BITS 11
#define DSX_TOPK_BINS (1 << DSX_TOPK_DIGIT_BITS)
#define DSX_TOPK_PASSES 6

// bit position of pass p's digit and its width
DSX_HD static inline int dsx_topk_shift(int pass) {
  int s = 64 - DSX_TOPK_DIGIT_BITS * (pass + 1);
  return s < 0 ? 0 : s;
}
DSX_HD static inline int dsx_topk_width(int pass) {
  int top = 64 - DSX_TOPK_DIGIT_BITS * pass;  // bits not yet consumed
  return top < DSX_TOPK_DIGIT_BITS ? top : DSX_TOPK_DIGIT_BITS;
}
DSX_HD static inline uint32_t dsx_topk_digit(uint64_t code, int pass) {
  return (uint32_t)(code >> dsx_topk_shift(pass)) &
         ((1u << dsx_topk_width(pass)) - 1u);
}
// does `code` share the digits of passes 0..pass-1 with `prefix`?
DSX_HD static inline int dsx_topk_in_prefix(uint64_t code, uint64_t prefix,
                                            int pass) {
  if (pass == 0) return 1;
  int s = dsx_topk_shift(pass - 1);
  return (code >> s) == (prefix >> s);
}
// is `code` at or before the bucket chosen through pass `pass`?
DSX_HD static inline int dsx_topk_at_or_before(uint64_t code, uint64_t prefix,
                                               int pass) {
  int s = dsx_topk_shift(pass);
  return (code >> s) <= (prefix >> s);
}

// ---- codes ----------------------------------------------------------------
// f64: dsx_f64_order_code (−0.0 ties with +0.0); returns 0 for NaN.
DSX_HD static inline int dsx_topk_code_f64(double x, int desc,
                                           uint64_t* code) {
  if (x != x) return 0;
  *code = dsx_f64_order_code(x, 1, desc ? 2 : 0);
  return 1;
}
// integers (i8/i32 widened by the caller): flip the sign bit; DESC complements
DSX_HD static inline uint64_t dsx_topk_code_i64(int64_t x, int desc) {
  uint64_t u = (uint64_t)x ^ (1ull << 63);
  return desc ? ~u : u;
}

// ---- digit pick -----------------------------------------------------------
// hist[0..nbins): rows per digit value among the rows inside the prefix.
// want: 1-based rank, inside the prefix, of the row looked for (the k-th row
// overall minus the rows before the prefix); 1 <= want <= sum(hist).
// taken: rows before the prefix. Returns the bucket of the wanted row;
// *before = rows of the prefix before that bucket; *done = 1 when taken +
// before + hist[bucket] <= cap, i.e. every row at or before the bucket fits
// the candidate cap and the select can stop here.
DSX_HD static inline int dsx_topk_pick(const uint32_t* hist, int nbins,
                                       uint32_t want, uint32_t taken,
                                       uint32_t cap, uint32_t* before,
                                       int* done) {
  uint64_t cum = 0;
  int b = 0;
  for (; b < nbins - 1; b++) {
    if (cum + hist[b] >= want) break;
    cum += hist[b];
  }
  *before = (uint32_t)cum;
  *done = (uint64_t)taken + cum + hist[b] <= (uint64_t)cap;
  return b;
}

// ---- trim (host) ------------------------------------------------------------
// The select stops at the first bucket that fits the cap, so the emitted rows
// are a superset of the answer. keep[i] = 1 for the cnt emitted codes at or
// before the k-th smallest of them (the k-th row is always among them);
// returns how many are kept.
static inline int64_t dsx_topk_trim(const uint64_t* codes, int64_t cnt,
                                    int64_t k, uint8_t* keep) {
  std::vector<uint64_t> sel(codes, codes + cnt);
  std::nth_element(sel.begin(), sel.begin() + (k - 1), sel.end());
  uint64_t kth = sel[k - 1];
  int64_t kept = 0;
  for (int64_t i = 0; i < cnt; i++) {
    keep[i] = codes[i] <= kth;
    kept += keep[i];
  }
  return kept;
}

#endif  // DSX_TOPK_SELECT_H
