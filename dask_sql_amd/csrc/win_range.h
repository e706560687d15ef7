// win_range.h — host/device arithmetic of the RANGE window frames
// (dsx_window_range, window_range.inc). Plain C++ so the host test can
// compile it alone with g++, like topk_select.h and gb_finish.h.
//
// Three things live here, the ones that go wrong silently:
//  - the saturating key + offset add;
//  - the two binary searches over the sorted order key of a partition's
//    non-NULL rows, in either direction;
//  - the decomposition of a frame [s, e] into a head of loose rows, a run of
//    whole 64-row blocks answered by two sparse-table entries, and a tail of
//    loose rows.
#ifndef DSX_WIN_RANGE_H
#define DSX_WIN_RANGE_H

#include <stdint.h>

#include "sort_code.h"

// rows per sparse-table block: one wave reduces one block
#define DSX_WIN_RMQ_BLOCK 64
#define DSX_WIN_RMQ_SHIFT 6
// frames up to this many rows are reduced by a direct loop; any wider frame
// holds at least one whole block (a head and a tail of at most 63 rows each
// leave 3 rows or more, and they start on a block edge)
#define DSX_WIN_RMQ_DIRECT_MAXW 128

// k + off, saturating at the int64 limits (never wraps)
DSX_HD static inline int64_t dsx_win_sat_add(int64_t k, int64_t off) {
  if (off > 0 && k > INT64_MAX - off) return INT64_MAX;
  if (off < 0 && k < INT64_MIN - off) return INT64_MIN;
  return k + off;
}

// The same, and *ovf tells which limit the exact sum lies beyond: +1 above
// INT64_MAX, -1 below INT64_MIN, 0 when it fits. A search target beyond a
// limit either admits every key (the saturated value does that by itself)
// or none at all, which the saturated value cannot say: a key AT the limit
// would compare equal to it.
DSX_HD static inline int64_t dsx_win_sat_add_ovf(int64_t k, int64_t off,
                                                 int* ovf) {
  *ovf = 0;
  if (off > 0 && k > INT64_MAX - off) *ovf = 1;
  if (off < 0 && k < INT64_MIN - off) *ovf = -1;
  return dsx_win_sat_add(k, off);
}

// Does an overflow `ovf` of the search target leave the bound without any
// row? The low bound wants keys at or after the target, so a target beyond
// the far end of the sort direction admits none; the high bound wants keys
// at or before it, so a target before the near end admits none.
DSX_HD static inline int dsx_win_low_none(int ovf, int desc) {
  return ovf == (desc ? -1 : 1);
}
DSX_HD static inline int dsx_win_high_none(int ovf, int desc) {
  return ovf == (desc ? 1 : -1);
}

// The searches run over key[lo, hi), which is sorted ascending (desc = 0) or
// descending (desc != 0) and holds no NULL and no NaN. "After" is the sort
// direction: a larger key when ascending, a smaller one when descending.
//
// first j in [lo, hi) whose key is AT or after t (hi when there is none):
// ascending key[j] >= t, descending key[j] <= t
template <class K>
DSX_HD static inline int64_t dsx_win_lower(const K* key, int64_t lo,
                                           int64_t hi, K t, int desc) {
  while (lo < hi) {
    int64_t mid = lo + ((hi - lo) >> 1);
    K x = key[mid];
    bool before = desc ? x > t : x < t;
    if (before) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// first j in [lo, hi) whose key is strictly after t (hi when there is
// none): ascending key[j] > t, descending key[j] < t. The last row at or
// before t is the answer minus one.
template <class K>
DSX_HD static inline int64_t dsx_win_upper(const K* key, int64_t lo,
                                           int64_t hi, K t, int desc) {
  while (lo < hi) {
    int64_t mid = lo + ((hi - lo) >> 1);
    K x = key[mid];
    bool at_or_before = desc ? x >= t : x <= t;
    if (at_or_before) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// levels of the sparse table over `blocks` blocks: level j entry i covers
// blocks [i, i + 2^j), so the top level is floor(log2(blocks))
DSX_HD static inline int dsx_win_rmq_levels(int64_t blocks) {
  int lv = 1;
  while (((int64_t)2 << (lv - 1)) <= blocks) lv++;
  return lv;
}

// A frame of sorted rows [s, e], s <= e, splits into
//   head rows   [s, head_end]      (empty when head_end < s)
//   whole blocks [b0, b1]          (empty when b1 < b0)
//   tail rows   [tail_begin, e]    (empty when tail_begin > e)
// With no whole block everything is head. The block run is answered by the
// two entries `left` and `right` of level `level`: blocks [left, left + 2^
// level) and [right, right + 2^level), which overlap and together cover
// exactly [b0, b1].
struct DsxWinRmqSplit {
  int64_t head_end;
  int64_t tail_begin;
  int64_t b0, b1;
  int level;
  int64_t left, right;
};

DSX_HD static inline DsxWinRmqSplit dsx_win_rmq_split(int64_t s, int64_t e) {
  DsxWinRmqSplit r;
  r.b0 = (s + DSX_WIN_RMQ_BLOCK - 1) >> DSX_WIN_RMQ_SHIFT;
  r.b1 = ((e + 1) >> DSX_WIN_RMQ_SHIFT) - 1;
  r.level = 0;
  r.left = r.right = 0;
  if (r.b1 < r.b0) {
    r.head_end = e;
    r.tail_begin = e + 1;
    return r;
  }
  r.head_end = (r.b0 << DSX_WIN_RMQ_SHIFT) - 1;
  r.tail_begin = (r.b1 + 1) << DSX_WIN_RMQ_SHIFT;
  int64_t nb = r.b1 - r.b0 + 1;
  int lv = 0;
  while (((int64_t)2 << lv) <= nb) lv++;
  r.level = lv;
  r.left = r.b0;
  r.right = r.b1 - ((int64_t)1 << lv) + 1;
  return r;
}

#endif  // DSX_WIN_RANGE_H
