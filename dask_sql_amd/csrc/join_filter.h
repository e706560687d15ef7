// join_filter.h — bit positions of the hash table's key-membership filter
// (DsxHashTable::filter, dsxhip.hip). One definition for three readers: the
// host and device code of dsxhip.hip, the generated filter-probe kernel
// (jit_kernels.inc pastes this text into its source) and a plain g++ test.
//
// Mode 1, exact: bit `code` of the array, for codes 0..code_max. A set bit IS
//   a build key, so the mask pass needs no table at all.
// Mode 2, hashed: a blocked two-bit Bloom filter. A key owns ONE 32-bit word
//   and two DISTINCT bits inside it, so a probe costs one word load. Word and
//   bits come from the top half of dsx_jf_mix64(code); the table's slot index
//   is the low bits of the same value (same function as mix64), so for tables
//   of up to 2^32 slots the two never share a bit.
//
// The functions are written inside DSX_JF_CODE(...) so that jit_kernels.inc
// can include this file a second time with DSX_JF_CODE stringifying its
// argument. Hence no preprocessor directive, string or character literal
// inside the parentheses.
#ifndef DSX_JOIN_FILTER_H
#define DSX_JOIN_FILTER_H
#define DSX_JF_NONE 0
#define DSX_JF_EXACT 1
#define DSX_JF_HASHED 2
// default byte cap of a filter: half of one XCD's 4 MiB L2
// (DSX_JOIN_FILTER_MAX_BYTES overrides it per call)
#define DSX_JOIN_FILTER_MAX_BYTES (2ll << 20)
// hashed mode: bits per build row asked for, and the least the cap must leave
// (DSX_JOIN_FILTER_MIN_BITS overrides the latter per call)
#define DSX_JF_BITS_PER_KEY 8
#define DSX_JF_MIN_BITS_PER_KEY 4
#endif  // DSX_JOIN_FILTER_H

#ifndef DSX_JF_CODE
#define DSX_JF_CODE(...) __VA_ARGS__
#endif
#ifndef DSX_JF_HD
#if defined(__HIPCC__)
#define DSX_JF_HD __host__ __device__ static inline
#else
#define DSX_JF_HD static inline
#endif
#endif

DSX_JF_CODE(
typedef unsigned long long dsx_jf_u64;
typedef unsigned int dsx_jf_u32;

DSX_JF_HD dsx_jf_u64 dsx_jf_mix64(dsx_jf_u64 x) {
  x += 0x9E3779B97F4A7C15ull; x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31; return x;
}

/* exact: 32-bit words that hold bits 0..code_max */
DSX_JF_HD dsx_jf_u64 dsx_jf_exact_words(dsx_jf_u64 code_max) {
  return (code_max >> 5) + 1;
}
DSX_JF_HD dsx_jf_u64 dsx_jf_exact_word(dsx_jf_u64 code) { return code >> 5; }
DSX_JF_HD dsx_jf_u32 dsx_jf_exact_bit(dsx_jf_u64 code) {
  return 1u << (dsx_jf_u32)(code & 31);
}

/* hashed: h = dsx_jf_mix64(code); word_mask = words - 1, words a power of 2.
   Word from bits 32.., first bit from bits 54..58, distance to the second
   bit (1..31) from bits 59..63. */
DSX_JF_HD dsx_jf_u64 dsx_jf_hashed_word(dsx_jf_u64 h, dsx_jf_u64 word_mask) {
  return (h >> 32) & word_mask;
}
DSX_JF_HD dsx_jf_u32 dsx_jf_hashed_bits(dsx_jf_u64 h) {
  dsx_jf_u32 b1 = (dsx_jf_u32)(h >> 54) & 31u;
  dsx_jf_u32 d = 1u + (((dsx_jf_u32)(h >> 59) * 31u) >> 5);
  return (1u << b1) | (1u << ((b1 + d) & 31u));
}
)
