// group_join.inc — dsx_filter_probe_groupby: an inner PK-FK join grouped by
// the PK (plus columns of the PK side) without materializing the join. The
// build keys are unique, so the group of a matched probe row IS its build row
// id: the probe sweep of dsx_filter_probe_cols keeps its mask pass and, in
// place of the emit pass and the whole group-by after it, accumulates each
// matched row's aggregate inputs at acc[bid]. Included from dsxhip.hip.
//
// Accumulators, array-of-structs per build row so that a row's updates fall
// in one line:  word 0        live byte, or the group's row count when a
//                             finish call needs one (COUNT or AVG over a
//                             never-NULL input); absent when a sum tells
//                             liveness (below);
//               voff[a]       accumulator a's value;
//               coff[a]       its non-NULL count, kept for nullable inputs
//                             only.
// Device-scope atomics run at ~23 RMW/ns chip-wide (DESIGN.md §3), which is
// the pass's floor: a never-NULL SUM with no count output costs ONE RMW per
// matched row. Liveness costs nothing where a never-NULL f64 SUM exists and no
// row count is kept: that accumulator starts at −0.0 and every addend goes in
// as x + 0.0, so it stays −0.0 exactly as long as no row arrived (−0.0 +
// (+0.0) is +0.0), and holds bit for bit what a sum started at +0.0 would.
// Otherwise liveness is a plain byte store (every writer stores 1) — a second
// write per row to the record's line, which only the interpreter kernel
// carries (jit_fprobe_agg_source).
//
// Finish: live build rows counted per block, k_scan_block_counts, then one
// launch writes every output column for the live rows in ascending build row
// order — key columns gathered from their build-side source, aggregate cells
// through dsx_gbf_finalize (gb_finish.h). The outputs are allocated at the
// n_build bound, so everything is queued before the call's ONE wait, which
// fetches {groups, dup flag} together.

struct GjAggArg {
  int32_t op[DSX_MAX_AGGS];
  int32_t nn[DSX_MAX_AGGS];    // never-NULL input
  int32_t voff[DSX_MAX_AGGS];  // word of the value inside a record
  int32_t coff[DSX_MAX_AGGS];  // word of the non-NULL count, −1 when nn
  int32_t naggs;
  int32_t stride;     // words per record
  int32_t need_gcnt;  // word 0 counts rows
  int32_t live_agg;   // ≥ 0: this never-NULL f64 SUM tells liveness and the
                      // record has no word 0; −1: word 0 (count or live byte)
  int32_t live_word;  // a record is live iff rec[live_word] != live_none
  uint64_t live_none;
  uint64_t init[1 + 2 * DSX_MAX_AGGS];  // a fresh record, word by word
};
#define GJ_NEG_ZERO 0x8000000000000000ull

// records larger than this in total decline (DSX_NOT_APPLICABLE): a quarter
// of what the buffer pool keeps cached
#define GJ_MAX_ACC_BYTES ((int64_t)4 << 30)

// fresh records where a plain memset of 0 does not do: MIN accumulators start
// at all-ones (agg_identity), the liveness sum at −0.0
__global__ void k_gj_init(uint64_t* acc, const GjAggArg* Ap, int64_t words) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t step = (int64_t)gridDim.x * BLOCK;
  int stride = Ap->stride;
  for (; i < words; i += step) acc[i] = Ap->init[i % stride];
}

// the accumulate pass, interpreter form. k_fprobe_emit's structure: each wave
// takes a contiguous quarter of the block's mask words, 64 words at a time,
// and lane j takes the batch's j-th matched row. No offsets, no total.
template <bool LITE>
__global__ void __launch_bounds__(BLOCK)
k_fprobe_agg(KeyArg K, ColsArg C, int64_t n, const uint64_t* tkeys,
             const uint32_t* tvals, int64_t tmask, int packed,
             const uint64_t* mask, const DsxInstr* agg_progs,
             const int32_t* agg_lens, const GjAggArg* Ap, uint64_t* acc,
             int64_t n_build, unsigned int* dbg) {
  int64_t lo, hi;
  block_range(n, 64, lo, hi);
  int lane = threadIdx.x & 63;
  int wid = threadIdx.x >> 6;
  int64_t w0 = (lo + 63) / 64, w1 = (hi + 63) / 64;  // lo == hi ⇒ no words
  int64_t q = (w1 - w0 + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  int64_t c0 = min(w1, w0 + wid * q), c1 = min(w1, c0 + q);
  const int stride = Ap->stride, naggs = Ap->naggs;
  const int need_gcnt = Ap->need_gcnt, live_agg = Ap->live_agg;
  for (int64_t wb = c0; wb < c1; wb += 64) {
    uint64_t m = (wb + lane < c1) ? mask[wb + lane] : 0;
    int cnt = __popcll(m);
    int inc = fp_wave_inclusive(cnt);
    int T = __shfl(inc, 63, 64);
    for (int j0 = 0; j0 < T; j0 += 64) {
      int j = min(j0 + lane, T - 1);
      int64_t r = fp_batch_row(m, inc, cnt, wb, j);
      if (j0 + lane >= T) continue;
      uint32_t bid = DSX_NULL_IDX;
      bool hit = r < n && fp_probe(tkeys, tvals, tmask, packed,
                                   pack_key(K, C, r), bid);
      if (!hit || (int64_t)bid >= n_build) {  // cannot happen: the mask says
        atomicOr(dbg, 2u);                    // the row matched
        continue;
      }
      uint64_t* rec = acc + (int64_t)bid * stride;
      if (need_gcnt) atomicAdd((unsigned long long*)rec, 1ull);
      else if (live_agg < 0) *(uint8_t*)rec = 1;
      const DsxInstr* p = agg_progs;
      for (int a = 0; a < naggs; a++) {
        Slot v;
        bool valid = vm_eval<LITE>(p, agg_lens[a], C, r, v);
        p += DSX_MAX_PROG;
        if (a == live_agg) v.f += 0.0;  // −0.0 goes in as +0.0
        int nn = Ap->nn[a];
        agg_update_global(Ap->op[a], nn, rec + Ap->voff[a],
                          (unsigned long long*)(rec + (nn ? 0 : Ap->coff[a])),
                          v, valid);
      }
    }
  }
}

// ---- generated form ---------------------------------------------------------
// j_fprobe_agg: the same pass with key pack, table layout, aggregate
// expressions, ops and record layout inlined per shape; pointers and sizes are
// arguments so the source text — the cache key — is stable from call to
// call. The key and aggregate-input loads of a row are issued before its
// probe, so they are in flight while the chain is walked.
#undef DSX_FPL_CODE
#define DSX_FPL_CODE(...) #__VA_ARGS__
static const char* JIT_FPROBE_LANES =
#include "fprobe_lanes.h"
    ;
#undef DSX_FPL_CODE
#define DSX_FPL_CODE(...) __VA_ARGS__

static std::string jit_fprobe_agg_source(const ColsArg& C, const KeyArg& K,
                                         const DsxAggSpec* aggs,
                                         const GjAggArg& A, bool packed) {
  if (K.nkeys < 1) return "";
  // The live-byte layout stays with the interpreter kernel: generated, the
  // byte store and the RMW leave back to back for the same line and the pass
  // measured 0.53 ms against the interpreter's 0.27 (DESIGN.md §8 Round 11),
  // which has the aggregate's loads between the two.
  if (A.live_agg < 0 && !A.need_gcnt) return "";
  std::ostringstream os;
  os << JIT_PRELUDE << JIT_FPROBE_LANES << "\n";
  std::vector<char> kinds(A.naggs, 'l');
  for (int a = 0; a < A.naggs; a++) {
    if (A.op[a] == DSX_AGG_COUNT && A.nn[a]) continue;  // nothing per row
    char name[32];
    snprintf(name, sizeof name, "eval_agg%d", a);
    if (!jit_emit_fn(os, name, aggs[a].prog, aggs[a].prog_len, &C, &kinds[a]))
      return "";
  }
  jit_emit_pack(os, K, &C);
  os << "#define EMPTY_KEY 0xFFFFFFFFFFFFFFFFull\n#define STRIDE " << A.stride
     << "\n"
     << R"(
extern "C" __global__ void __launch_bounds__(BLOCK) j_fprobe_agg(
    ColsArg C, i64 n, const u64* __restrict__ tkeys,
    const u32* __restrict__ tvals, i64 tmask, const u64* __restrict__ mask,
    u64* __restrict__ acc, i64 n_build, u32* __restrict__ dbg) {
  i64 lo, hi; block_range(n, 64, lo, hi);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const i64 w0 = (lo + 63) / 64, w1 = (hi + 63) / 64;  // lo == hi: no words
  const i64 q = (w1 - w0 + BLOCK / 64 - 1) / (BLOCK / 64);
  i64 c0 = w0 + wid * q; if (c0 > w1) c0 = w1;
  i64 c1 = c0 + q; if (c1 > w1) c1 = w1;
  for (i64 wb = c0; wb < c1; wb += 64) {
    u64 m = (wb + lane < c1) ? mask[wb + lane] : 0;
    int cnt = __popcll(m);
    int inc = fp_wave_inclusive(cnt);
    int T = __shfl(inc, 63, 64);
    for (int j0 = 0; j0 < T; j0 += 64) {
      int jj = j0 + lane < T ? j0 + lane : T - 1;
      i64 r = fp_batch_row(m, inc, cnt, wb, jj);
      if (j0 + lane >= T) continue;
      if (r >= n) { atomicOr(dbg, 2u); continue; }
      u64 code = jit_pack(C, r);
)";
  for (int a = 0; a < A.naggs; a++) {
    if (A.op[a] == DSX_AGG_COUNT && A.nn[a]) continue;
    os << "      " << (kinds[a] == 'd' ? "double" : "i64") << " v" << a
       << "; bool ok" << a << " = eval_agg" << a << "(C, r, v" << a << ");\n";
  }
  os << "      i64 s = (i64)(mix64(code) & (u64)tmask);\n"
     << "      u32 bid = 0xFFFFFFFFu; bool hit = false;\n"
     << "      while (true) {\n        u64 k = tkeys[s];\n"
     << "        if (k == EMPTY_KEY) break;\n";
  if (packed)
    os << "        if ((k >> 32) == code) { bid = (u32)k; hit = true; break; }\n";
  else
    os << "        if (k == code) { bid = tvals[s]; hit = true; break; }\n";
  os << "        s = (s + 1) & tmask;\n      }\n"
     << "      if (!hit || (i64)bid >= n_build) { atomicOr(dbg, 2u); continue; }\n"
     << "      u64* rec = acc + (i64)bid * STRIDE;\n";
  if (A.need_gcnt) os << "      atomicAdd(rec, 1ull);\n";
  for (int a = 0; a < A.naggs; a++) {
    if (A.op[a] == DSX_AGG_COUNT && A.nn[a]) continue;
    std::string val = "rec + " + std::to_string(A.voff[a]);
    std::string v = "v" + std::to_string(a);
    os << "      if (ok" << a << ") { ";
    switch (A.op[a]) {
      case DSX_AGG_SUM_F64:
        // the liveness sum takes −0.0 as +0.0 (header comment)
        os << "atomicAdd((double*)(" << val << "), (double)" << v
           << (a == A.live_agg ? " + 0.0); " : "); ");
        break;
      case DSX_AGG_SUM_I64:
        os << "atomicAdd(" << val << ", (u64)(i64)" << v << "); ";
        break;
      case DSX_AGG_MIN_F64:
        os << "atomicMin(" << val << ", f64_ordered((double)" << v << ")); ";
        break;
      case DSX_AGG_MAX_F64:
        os << "atomicMax(" << val << ", f64_ordered((double)" << v << ")); ";
        break;
      case DSX_AGG_MIN_I64:
        os << "atomicMin(" << val << ", i64_ordered((i64)" << v << ")); ";
        break;
      case DSX_AGG_MAX_I64:
        os << "atomicMax(" << val << ", i64_ordered((i64)" << v << ")); ";
        break;
      case DSX_AGG_COUNT:
        os << "(void)" << v << "; ";
        break;
      default:
        return "";
    }
    if (!A.nn[a]) os << "atomicAdd(rec + " << A.coff[a] << ", 1ull); ";
    os << "}\n";
  }
  os << "    }\n  }\n}\n";
  return os.str();
}

// ---- finish -------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
k_gj_count(const uint64_t* acc, int stride, int live_word,
           uint64_t live_none, int64_t n_build, int64_t* block_counts) {
  __shared__ int s_w[WAVES_PER_BLOCK];
  int64_t lo, hi;
  block_range(n_build, 1, lo, hi);
  int local = 0;
  for (int64_t b = lo + threadIdx.x; b < hi; b += BLOCK)
    local += acc[b * stride + live_word] != live_none;
  for (int d = 32; d > 0; d >>= 1) local += __shfl_down(local, d, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t t = 0;
    for (int i = 0; i < WAVES_PER_BLOCK; i++) t += s_w[i];
    block_counts[blockIdx.x] = t;
  }
}

// by value, loops fully unrolled: launch-uniform fields stay in SGPRs (note at
// GbFinishArg)
struct GjWriteArg {
  const void* ksrc[DSX_MAX_KEYS];  // build-side source of output key j
  const uint8_t* ksrcv[DSX_MAX_KEYS];
  uint64_t* kdata[DSX_MAX_KEYS];
  uint8_t* kvalid[DSX_MAX_KEYS];   // allocated iff the source has validity
  uint64_t* adata[DSX_MAX_AGGS];
  uint8_t* avalid[DSX_MAX_AGGS];   // nullptr for COUNT
  int32_t kdtype[DSX_MAX_KEYS];
  int32_t kind[DSX_MAX_AGGS];      // DSX_GBF_*
  int32_t voff[DSX_MAX_AGGS];
  int32_t coff[DSX_MAX_AGGS];      // −1: never-NULL input
  int32_t nkeys, ncalls, stride, need_gcnt, live_word;
  uint64_t live_none;
};

// integer sources widen to i64, float sources to f64: the cell types of the
// group-by's own key columns (dsx_hash_groupby_cols)
__device__ __forceinline__ uint64_t gj_key_bits(const void* src, int dtype,
                                                int64_t b) {
  switch (dtype) {
    case DSX_I64: return (uint64_t)((const int64_t*)src)[b];
    case DSX_F64: return ((const uint64_t*)src)[b];
    case DSX_I32: return (uint64_t)(int64_t)((const int32_t*)src)[b];
    case DSX_F32:
      return (uint64_t)__double_as_longlong((double)((const float*)src)[b]);
    case DSX_I8: return (uint64_t)(int64_t)((const int8_t*)src)[b];
    default: return (uint64_t)((const uint8_t*)src)[b];  // BOOL8
  }
}

__global__ void __launch_bounds__(BLOCK)
k_gj_write(GjWriteArg W, const uint64_t* acc, int64_t n_build,
           const int64_t* block_offsets) {
  __shared__ int s_w[WAVES_PER_BLOCK];
  int64_t lo, hi;
  block_range(n_build, 1, lo, hi);
  int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int64_t base = block_offsets[blockIdx.x];
  for (int64_t b0 = lo; b0 < hi; b0 += BLOCK) {
    int64_t b = b0 + threadIdx.x;
    const uint64_t* rec = acc + b * W.stride;
    bool live = b < hi && rec[W.live_word] != W.live_none;
    uint64_t bal = __ballot(live);
    if (lane == 0) s_w[wid] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < WAVES_PER_BLOCK; i++) {
      if (i < wid) before += s_w[i];
      all += s_w[i];
    }
    if (live) {
      int64_t o = base + before + __popcll(bal & ((1ull << lane) - 1));
#pragma unroll
      for (int j = 0; j < DSX_MAX_KEYS; j++) {
        if (j >= W.nkeys) break;
        W.kdata[j][o] = gj_key_bits(W.ksrc[j], W.kdtype[j], b);
        if (W.kvalid[j]) W.kvalid[j][o] = W.ksrcv[j][b];
      }
#pragma unroll
      for (int a = 0; a < DSX_MAX_AGGS; a++) {
        if (a >= W.ncalls) break;
        // a live group whose input is never NULL and kept no count has
        // at least one row; only count > 0 matters to its finalize
        uint64_t cnt = W.coff[a] >= 0 ? rec[W.coff[a]]
                       : W.need_gcnt  ? rec[0]
                                      : 1ull;
        uint64_t raw = W.kind[a] == DSX_GBF_COUNT ? 0ull : rec[W.voff[a]];
        uint64_t bits;
        int valid = dsx_gbf_finalize(W.kind[a], raw, cnt, &bits);
        W.adata[a][o] = bits;
        if (W.avalid[a]) W.avalid[a][o] = (uint8_t)valid;
      }
    }
    base += all;
    __syncthreads();
  }
}

// record layout from op, nn, naggs and need_gcnt (header comment)
static void gj_layout(GjAggArg& A) {
  A.live_agg = -1;
  if (!A.need_gcnt)
    for (int a = 0; a < A.naggs && A.live_agg < 0; a++)
      if (A.op[a] == DSX_AGG_SUM_F64 && A.nn[a]) A.live_agg = a;
  A.stride = A.live_agg < 0 ? 1 : 0;
  for (int a = 0; a < A.naggs; a++) {
    A.voff[a] = A.stride++;
    A.coff[a] = A.nn[a] ? -1 : A.stride++;
  }
  memset(A.init, 0, sizeof A.init);
  for (int a = 0; a < A.naggs; a++)
    A.init[A.voff[a]] = a == A.live_agg ? GJ_NEG_ZERO : agg_identity(A.op[a]);
  A.live_word = A.live_agg < 0 ? 0 : A.voff[A.live_agg];
  A.live_none = A.live_agg < 0 ? 0 : GJ_NEG_ZERO;
}

extern "C" int64_t dsx_fprobe_agg_jit_launches(DsxCtx* c) {
  return c->fprobe_agg_jit_launches;
}

extern "C" int dsx_filter_probe_groupby(
    DsxCtx* c, DsxHashTable* t, const DsxInstr* prog, int prog_len,
    const DsxColumn* cols, int ncols, const DsxKeySpec* keys, int nkeys,
    int64_t n, const DsxAggSpec* aggs, int naggs,
    const DsxGbFinishCall* calls, int ncalls, const DsxColumn* kcols,
    int n_kcols, void** out_datas, uint8_t** out_valids,
    int64_t* out_groups) {
  if (prog_len > DSX_MAX_PROG || ncols > DSX_MAX_COLS || nkeys > DSX_MAX_KEYS)
    FAIL(-3, "filter-probe spec too large");
  if (naggs < 0 || naggs > DSX_MAX_AGGS || ncalls < 0 ||
      ncalls > DSX_MAX_AGGS || n_kcols < 1 || n_kcols > DSX_MAX_KEYS)
    FAIL(-3, "group-join spec too large or without key columns");
  int rc = gb_finish_calls_check(aggs, naggs, calls, ncalls);
  if (rc) return rc;
  *out_groups = 0;
  int nout = n_kcols + ncalls;
  for (int i = 0; i < nout; i++) {
    out_datas[i] = nullptr;
    out_valids[i] = nullptr;
  }
  const int64_t n_build = t->n_build;
  for (int j = 0; j < n_kcols; j++)
    if (kcols[j].len != n_build)
      FAIL(-3, "group-join key source is not a build-side column");
  ProgArg P{};
  memcpy(P.ins, prog, prog_len * sizeof(DsxInstr));
  P.len = prog_len;
  KeyArg K{};
  rc = make_keyarg(keys, nkeys, K);
  if (rc) return rc;
  for (int j = 0; j < nkeys; j++)
    if (keys[j].mode != 0 || keys[j].col < 0 || keys[j].col >= ncols)
      FAIL(-3, "filter-probe takes radix-packed integer keys only");
  ColsArg C{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    C.data[i] = cols[i].data;
    C.validity[i] = cols[i].validity;
    C.dtype[i] = cols[i].dtype;
  }

  // record layout
  GjAggArg A{};
  A.naggs = naggs;
  bool any_min = false, lite = true;
  for (int a = 0; a < naggs; a++) {
    if (aggs[a].prog_len < 0 || aggs[a].prog_len > DSX_MAX_PROG)
      FAIL(-3, "aggregate program too large");
    A.op[a] = aggs[a].op;
    int nn = 1;
    for (int i = 0; i < aggs[a].prog_len; i++) {
      const DsxInstr& in = aggs[a].prog[i];
      if (in.op == DSX_OP_LIT_NULL) nn = 0;
      if (in.op == DSX_OP_COL) {
        if (in.arg0 < 0 || in.arg0 >= ncols)
          FAIL(-3, "aggregate program reads no probe column");
        if (cols[in.arg0].validity != nullptr) nn = 0;
      }
    }
    A.nn[a] = nn;
    lite &= vm_prog_is_lite(aggs[a].prog, aggs[a].prog_len);
  }
  // a row count only where a finish call reads one that no per-aggregate
  // count supplies
  for (int i = 0; i < ncalls; i++)
    if ((calls[i].kind == DSX_GBF_COUNT || calls[i].kind == DSX_GBF_AVG) &&
        A.nn[calls[i].agg])
      A.need_gcnt = 1;
  gj_layout(A);
  for (int a = 0; a < naggs; a++)
    any_min |= A.op[a] == DSX_AGG_MIN_F64 || A.op[a] == DSX_AGG_MIN_I64;
  int64_t acc_bytes = (n_build > 0 ? n_build : 1) * A.stride * 8;
  if (acc_bytes > GJ_MAX_ACC_BYTES) return DSX_NOT_APPLICABLE;

  int64_t nwords = (n + 63) / 64;
  int grid = (int)min((int64_t)MAX_GRID, (nwords + WAVES_PER_BLOCK - 1) /
                                             WAVES_PER_BLOCK);
  int grid2 = (int)min((int64_t)MAX_GRID, (n_build + BLOCK - 1) / BLOCK);
  // host block copied in one piece: programs, lengths, record layout
  int64_t prog_bytes = (int64_t)naggs * DSX_MAX_PROG * sizeof(DsxInstr);
  int64_t lens_off = prog_bytes;
  int64_t a_off = ((lens_off + naggs * 4 + 15) / 16) * 16;
  int64_t blk_bytes = a_off + (int64_t)sizeof(GjAggArg);
  std::vector<char> hblk((size_t)blk_bytes, 0);
  for (int a = 0; a < naggs; a++) {
    memcpy(&hblk[(size_t)a * DSX_MAX_PROG * sizeof(DsxInstr)], aggs[a].prog,
           aggs[a].prog_len * sizeof(DsxInstr));
    ((int32_t*)&hblk[lens_off])[a] = aggs[a].prog_len;
  }
  memcpy(&hblk[a_off], &A, sizeof(GjAggArg));
  int64_t res_off = nwords * 8 + (int64_t)grid * 8;
  int64_t bc2_off = res_off + 16;
  int64_t blk_off = ((bc2_off + (int64_t)grid2 * 8 + 63) / 64) * 64;
  rc = ensure_scratch(c, blk_off + blk_bytes + 64);
  if (rc) return rc;
  char* sbase = (char*)c->scratch;
  uint64_t* mask = (uint64_t*)sbase;
  int64_t* block_counts = (int64_t*)(mask + nwords);
  int64_t* d_res = (int64_t*)(sbase + res_off);  // [0] groups, [1] dup flag
  int64_t* bc2 = (int64_t*)(sbase + bc2_off);
  const DsxInstr* d_progs = (const DsxInstr*)(sbase + blk_off);
  const int32_t* d_lens = (const int32_t*)(sbase + blk_off + lens_off);
  const GjAggArg* d_A = (const GjAggArg*)(sbase + blk_off + a_off);

  // outputs at the n_build bound, so that the write launch is queued before
  // the wait; on any failure below nothing stays allocated
  uint64_t* acc = nullptr;
  auto release_all = [&]() {
    for (int i = 0; i < nout; i++) {
      if (out_datas[i]) pool_release(c, out_datas[i]);
      if (out_valids[i]) pool_release(c, out_valids[i]);
      out_datas[i] = nullptr;
      out_valids[i] = nullptr;
    }
    if (acc) pool_release(c, acc);
    acc = nullptr;
  };
  GjWriteArg W{};
  W.nkeys = n_kcols;
  W.ncalls = ncalls;
  W.stride = A.stride;
  W.need_gcnt = A.need_gcnt;
  W.live_word = A.live_word;
  W.live_none = A.live_none;
  int64_t b1 = n_build > 0 ? n_build : 1;
  rc = pool_alloc(c, acc_bytes, (void**)&acc);
  for (int i = 0; i < nout && !rc; i++) {
    bool want_valid = i < n_kcols ? kcols[i].validity != nullptr
                                  : calls[i - n_kcols].kind != DSX_GBF_COUNT;
    rc = pool_alloc(c, b1 * 8, &out_datas[i]);
    if (!rc && want_valid) rc = pool_alloc(c, b1, (void**)&out_valids[i]);
  }
  if (rc) {
    release_all();
    return rc;
  }
  for (int j = 0; j < n_kcols; j++) {
    W.ksrc[j] = kcols[j].data;
    W.ksrcv[j] = kcols[j].validity;
    W.kdtype[j] = kcols[j].dtype;
    W.kdata[j] = (uint64_t*)out_datas[j];
    W.kvalid[j] = out_valids[j];
  }
  for (int i = 0; i < ncalls; i++) {
    int a = calls[i].agg;
    W.adata[i] = (uint64_t*)out_datas[n_kcols + i];
    W.avalid[i] = out_valids[n_kcols + i];
    W.kind[i] = calls[i].kind;
    W.voff[i] = A.voff[a];
    W.coff[i] = A.coff[a];
  }

  int64_t h_res[2] = {0, 0};
  if (grid > 0 && grid2 > 0) {
    hipError_t e = hipMemcpyAsync(sbase + blk_off, hblk.data(), blk_bytes,
                                  hipMemcpyHostToDevice, c->stream);
    {
      ProfScope ps(c, "k_gj_clear");
      if (e == hipSuccess && !(any_min || A.live_agg >= 0))
        e = hipMemsetAsync(acc, 0, acc_bytes, c->stream);
      else if (e == hipSuccess)
        hipLaunchKernelGGL(k_gj_init, dim3(grid2), dim3(BLOCK), 0, c->stream,
                           acc, d_A, n_build * A.stride);
    }
    if (e != hipSuccess) {
      release_all();
      FAIL(-1, "group-join setup: %s", hipGetErrorString(e));
    }
    fprobe_mask_pass(c, t, prog, prog_len, P, K, C, n, grid, mask,
                     block_counts, d_res + 1);
    {
      // generated kernel first; the interpreter is the fallback (JIT off,
      // DSX_DISABLE_JIT_FPROBE=1 as for the mask pass, an expression the
      // generator rejects, hipRTC failure)
      JitEntry* je =
          jit_enabled() && jit_fprobe_enabled()
              ? jit_source_entry(
                    c, jit_fprobe_agg_source(C, K, aggs, A, t->packed != 0))
              : nullptr;
      hipFunction_t fj = je ? jit_fn(c, je, "j_fprobe_agg") : nullptr;
      ProfScope ps(c, "k_fprobe_agg");
      if (fj) {
        ColsArg Ca = C;
        int64_t tmask = t->slots - 1, nb = n_build;
        const uint64_t* tk = t->keys;
        const uint32_t* tv = t->vals;
        const uint64_t* mk = mask;
        unsigned int* dbg = c->dbg_flag;
        void* args[] = {&Ca, &n, &tk, &tv, &tmask, &mk, &acc, &nb, &dbg};
        e = hipModuleLaunchKernel(fj, grid, 1, 1, BLOCK, 1, 1, 0, c->stream,
                                  args, nullptr);
        if (e != hipSuccess) {
          release_all();
          FAIL(-1, "j_fprobe_agg launch: %s", hipGetErrorString(e));
        }
        c->fprobe_agg_jit_launches++;
      } else {
        auto kern = lite ? k_fprobe_agg<true> : k_fprobe_agg<false>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK), 0, c->stream, K, C,
                           n, t->keys, t->vals, t->slots - 1, t->packed, mask,
                           d_progs, d_lens, d_A, acc, n_build, c->dbg_flag);
      }
    }
    {
      ProfScope ps(c, "k_gj_finish");
      hipLaunchKernelGGL(k_gj_count, dim3(grid2), dim3(BLOCK), 0, c->stream,
                         acc, A.stride, A.live_word, A.live_none, n_build,
                         bc2);
      hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0,
                         c->stream, bc2, grid2, d_res);
      hipLaunchKernelGGL(k_gj_write, dim3(grid2), dim3(BLOCK), 0, c->stream,
                         W, acc, n_build, bc2);
    }
    e = hipGetLastError();
    if (e == hipSuccess)
      e = hipMemcpyAsync(h_res, d_res, 16, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      release_all();
      FAIL(-1, "group-join: %s", hipGetErrorString(e));
    }
    // duplicate build keys: a group is not one build row. The accumulators
    // are garbage, but nothing faulted: fp_probe returns the first match.
    if (h_res[1] != 0) {
      release_all();
      return DSX_NOT_APPLICABLE;
    }
  }
  pool_release(c, acc);
  acc = nullptr;
  *out_groups = h_res[0];
  return dbg_check(c, "dsx_filter_probe_groupby");
}

// dsx_jit_fprobe_agg_selftest — TEST INFRASTRUCTURE: hipRTC-compile the
// generated accumulate kernel WITHOUT a GPU (like dsx_jit_fprobe_selftest) for
// each record layout: Q3's shape (one packed i64 key, one never-NULL f64 SUM:
// the liveness sum, no word 0), an unpacked composite key with nullable
// inputs, every op and a row count in word 0, and the same key with a
// never-NULL i64 SUM and f64 MIN alone (the live byte in word 0), which the
// generator must decline.
// Returns 0, or shape + 1 of the first failure.
extern "C" int dsx_jit_compile_check(const char* src);
extern "C" int dsx_jit_fprobe_agg_selftest(void) {
  for (int shape = 0; shape < 3; shape++) {
    ColsArg C{};
    C.ncols = 4;
    C.dtype[0] = DSX_I64;  // key
    C.dtype[1] = DSX_F64;
    C.dtype[2] = DSX_F64;
    C.dtype[3] = DSX_I32;  // second key; nullable value column of shape 1
    if (shape) C.validity[3] = (const uint8_t*)1;
    DsxKeySpec keys[2]{};
    keys[0].col = 0;
    keys[0].range = shape ? (int64_t)1 << 40 : 60'000'000;
    keys[1].col = 3;
    keys[1].range = 1000;
    KeyArg K{};
    if (make_keyarg(keys, shape ? 2 : 1, K)) return shape + 1;
    static DsxAggSpec aggs[8];
    memset(aggs, 0, sizeof aggs);
    GjAggArg A{};
    if (!shape) {  // SUM(c1 * (1 - c2))
      double one = 1.0;
      aggs[0].op = DSX_AGG_SUM_F64;
      aggs[0].prog[0] = {DSX_OP_COL, 1, 0};
      aggs[0].prog[1] = {DSX_OP_LIT_F64, 0, 0};
      memcpy(&aggs[0].prog[1].imm, &one, 8);
      aggs[0].prog[2] = {DSX_OP_COL, 2, 0};
      aggs[0].prog[3] = {DSX_OP_SUB_F64, 0, 0};
      aggs[0].prog[4] = {DSX_OP_MUL_F64, 0, 0};
      aggs[0].prog_len = 5;
      A.naggs = 1;
      A.op[0] = DSX_AGG_SUM_F64;
      A.nn[0] = 1;
    } else if (shape == 2) {
      for (int a = 0; a < 2; a++) {
        aggs[a].op = A.op[a] = a ? DSX_AGG_MIN_F64 : DSX_AGG_SUM_I64;
        aggs[a].prog[0] = {DSX_OP_COL, a, 0};
        aggs[a].prog_len = 1;
        A.nn[a] = 1;
      }
      A.naggs = 2;
    } else {
      const int ops[7] = {DSX_AGG_SUM_F64, DSX_AGG_SUM_I64, DSX_AGG_COUNT,
                          DSX_AGG_MIN_F64, DSX_AGG_MAX_F64, DSX_AGG_MIN_I64,
                          DSX_AGG_MAX_I64};
      A.naggs = 8;
      A.need_gcnt = 1;
      for (int a = 0; a < 8; a++) {
        int op = a < 7 ? ops[a] : DSX_AGG_COUNT;
        bool f = op == DSX_AGG_SUM_F64 || op == DSX_AGG_MIN_F64 ||
                 op == DSX_AGG_MAX_F64;
        aggs[a].op = op;
        aggs[a].prog[0] = {DSX_OP_COL, f ? 1 : 3, 0};
        aggs[a].prog_len = 1;
        A.op[a] = op;
        A.nn[a] = f || a == 7;  // the last COUNT reads nothing per row
        if (a == 7) aggs[a].prog[0] = {DSX_OP_LIT_I64, 0, 1};
      }
    }
    gj_layout(A);
    // each shape must take the layout it is here for
    if ((A.live_agg >= 0) != (shape == 0) || A.need_gcnt != (shape == 1))
      return shape + 1;
    std::string src = jit_fprobe_agg_source(C, K, aggs, A, shape == 0);
    if (shape == 2) {  // left to the interpreter kernel
      if (!src.empty()) return shape + 1;
      continue;
    }
    if (const char* dump = getenv("DSX_JIT_DUMP")) {  // as jit_source_entry
      char fn[512];
      snprintf(fn, sizeof fn, "%s/jit_fprobe_agg_%d.cu", dump, shape);
      if (FILE* f = fopen(fn, "w")) {
        fwrite(src.data(), 1, src.size(), f);
        fclose(f);
      }
    }
    if (src.empty() || dsx_jit_compile_check(src.c_str())) return shape + 1;
  }
  return 0;
}
