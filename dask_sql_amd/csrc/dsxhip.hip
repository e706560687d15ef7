// dsxhip.hip — MI355X (gfx950/CDNA4) kernels + C ABI for the dask-sql hot
// path. See include/dsxhip.h for the boundary contract and the reference
// call each entry point replaces. Design: DESIGN.md §3.
//
// All kernels are HBM-roofline scan/hash work (no MFMA): 256-thread blocks,
// contiguous per-block row ranges (coalesced 8 B/lane loads), wave64 ballot
// compaction, device-scope atomics for cross-XCD-coherent hash tables.

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dsxhip.h"
#include "join_filter.h"
#include "gb_finish.h"

#define BLOCK 256
#define WAVES_PER_BLOCK (BLOCK / 64)
#define MAX_GRID 2048
#define EMPTY_KEY 0xFFFFFFFFFFFFFFFFull

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local char g_err[512];
extern "C" const char* dsx_last_error(void) { return g_err; }

#define FAIL(code, ...)                                                        \
  do {                                                                         \
    snprintf(g_err, sizeof(g_err), __VA_ARGS__);                               \
    return (code);                                                             \
  } while (0)

#define HIP_TRY(expr)                                                          \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      FAIL(-1, "%s:%d HIP error: %s", __FILE__, __LINE__,                      \
           hipGetErrorString(_e));                                             \
  } while (0)

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
struct ProfRec {
  char name[32];
  hipEvent_t start, stop;
};

struct DsxCtx {
  int device = 0;
  hipStream_t stream = nullptr;
  // scratch arena reused across calls (programs, block counts, flags)
  void* scratch = nullptr;
  int64_t scratch_bytes = 0;
  bool prof = false;
  std::vector<ProfRec> prof_recs;
  // size-bucketed buffer pool: per-step outputs (group tables, selection
  // vectors, join pairs) would otherwise pay ~0.1-1 ms of hipMalloc/Free
  // per query step
  std::unordered_map<int64_t, std::vector<void*>> pool_free;
  std::unordered_map<void*, int64_t> pool_sizes;
  int64_t pool_cached = 0;
  unsigned int* dbg_flag = nullptr;  // device word; bit0 gather OOB,
                                     // bit1 probe-emit OOB (DSX_DEBUG)
  bool debug = false;
  void* jit_cache = nullptr;  // JitCacheMap (jit.inc)
  int64_t fprobe_jit_launches = 0;  // generated j_fprobe_mask launches
  int64_t fprobe_agg_jit_launches = 0;  // generated j_fprobe_agg launches
  int64_t join_filter_builds[3] = {0, 0, 0};  // filtered builds per mode
  // pinned staging arena for host→HBM ingest (parquet path): pageable
  // hipMemcpy forces an internal staging copy at ~⅓ the PCIe rate;
  // memcpy→pinned + hipMemcpyAsync is the fast path
  void* pinned = nullptr;
  int64_t pinned_bytes = 0;
  // pinned landing buffer of dsx_topk_rows (topk.inc): grows on demand, the
  // returned host pointer stays valid until the next call on this context
  void* topk_pinned = nullptr;
  int64_t topk_pinned_bytes = 0;
  // balance-guard verdict cache for the direct-index groupby: keyed on the
  // key column's device pointer + shape — the distribution is a property
  // of the data, so the mid-pipeline totals sync runs once per table, not
  // every step (repeat steps of the same query pay no guard stall)
  std::unordered_map<uint64_t, int> gb_guard_cache;
  // per-table (hist, bases) cache for the partition groupby: the histogram
  // is predicate-free (pure function of the key column), so repeat steps
  // skip the hist+scan passes. Sig = key col ptrs + n + space + layout +
  // per-key min/range (aliasing a recycled device ptr additionally needs
  // identical n/min/max — accepted residual risk, like the stats cache).
  struct GbHist {
    uint64_t sig;
    void* hist;
    void* bases;
    const void* srcs[DSX_MAX_KEYS];  // key column data ptrs: a free of any
    int nsrc;                        // of these evicts the entry (stale-
                                     // pointer-reuse hazard)
  };
  std::vector<GbHist> gb_hist_cache;
  bool gb_hist_cache_on = true;  // off for externally-backed key columns
                                 // (torch tensors recycle pointers outside
                                 // the pool's eviction hook)
};

static void gb_hist_evict_ptr(DsxCtx* c, void* p);

static int64_t pool_round(int64_t bytes) {
  int64_t r = 256;
  while (r < bytes) r <<= 1;
  return r;
}

static int pool_alloc(DsxCtx* c, int64_t bytes, void** out) {
  int64_t r = pool_round(bytes > 0 ? bytes : 1);
  auto it = c->pool_free.find(r);
  if (it != c->pool_free.end() && !it->second.empty()) {
    *out = it->second.back();
    it->second.pop_back();
    c->pool_cached -= r;
    return 0;
  }
  hipError_t e = hipMalloc(out, r);
  if (e != hipSuccess) {
    // pressure: drop the pool and retry once
    for (auto& kv : c->pool_free)
      for (void* p : kv.second) hipFree(p);
    c->pool_free.clear();
    c->pool_cached = 0;
    e = hipMalloc(out, r);
    if (e != hipSuccess)
      FAIL(-2, "device alloc of %lld failed: %s", (long long)r,
           hipGetErrorString(e));
  }
  c->pool_sizes[*out] = r;
  return 0;
}

static void pool_release(DsxCtx* c, void* p) {
  gb_hist_evict_ptr(c, p);
  if (!p) return;
  auto it = c->pool_sizes.find(p);
  if (it == c->pool_sizes.end()) {
    hipFree(p);  // not pool-allocated
    return;
  }
  int64_t r = it->second;
  if (c->pool_cached + r > (int64_t)16 << 30) {
    hipFree(p);
    c->pool_sizes.erase(it);
    return;
  }
  c->pool_free[r].push_back(p);
  c->pool_cached += r;
}

static int ensure_scratch(DsxCtx* c, int64_t bytes) {
  if (c->scratch_bytes >= bytes) return 0;
  if (c->scratch) hipFree(c->scratch);
  int64_t want = bytes + bytes / 2;
  if (hipMalloc(&c->scratch, want) != hipSuccess) {
    c->scratch = nullptr;
    c->scratch_bytes = 0;
    FAIL(-2, "scratch alloc of %lld bytes failed", (long long)want);
  }
  c->scratch_bytes = want;
  return 0;
}

extern "C" int dsx_ctx_create(int device_id, DsxCtx** out) {
  HIP_TRY(hipSetDevice(device_id));
  DsxCtx* c = new DsxCtx();
  c->device = device_id;
  if (hipStreamCreate(&c->stream) != hipSuccess) {
    delete c;
    FAIL(-1, "stream create failed");
  }
  c->debug = getenv("DSX_DEBUG") != nullptr;
  HIP_TRY(hipMalloc((void**)&c->dbg_flag, 16));
  HIP_TRY(hipMemset(c->dbg_flag, 0, 16));
  *out = c;
  return 0;
}

static int dbg_check(DsxCtx* c, const char* what) {
  if (!c->debug) return 0;
  unsigned int f[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(f, c->dbg_flag, 16, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (f[0])
    FAIL(-9,
         "DEVICE BOUNDS VIOLATION (flags 0x%x, bad_sel=%u, n_src=%u, "
         "pos=%u) at %s", f[0], f[1], f[2], f[3], what);
  return 0;
}

void jit_cache_destroy(DsxCtx* c);  // defined after jit includes

extern "C" void dsx_ctx_destroy(DsxCtx* c) {
  if (!c) return;
  hipStreamSynchronize(c->stream);
  jit_cache_destroy(c);
  for (auto& kv : c->pool_free)
    for (void* p : kv.second) hipFree(p);
  for (auto& kv : c->pool_sizes) (void)kv;
  for (auto& r : c->prof_recs) {
    hipEventDestroy(r.start);
    hipEventDestroy(r.stop);
  }
  for (auto& h : c->gb_hist_cache) {
    pool_release(c, h.hist);
    pool_release(c, h.bases);
  }
  if (c->scratch) hipFree(c->scratch);
  if (c->pinned) hipHostFree(c->pinned);
  if (c->topk_pinned) hipHostFree(c->topk_pinned);
  hipStreamDestroy(c->stream);
  delete c;
}

extern "C" int dsx_synchronize(DsxCtx* c) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int dsx_malloc(DsxCtx* c, int64_t bytes, void** out) {
  return pool_alloc(c, bytes, out);
}
extern "C" int dsx_free(DsxCtx* c, void* p) {
  pool_release(c, p);
  return 0;
}
extern "C" int dsx_upload(DsxCtx* c, const void* host, int64_t bytes,
                          void** out_dev) {
  int rc = pool_alloc(c, bytes, out_dev);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(*out_dev, host, bytes, hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
/* host→device upload through a persistent PINNED staging arena, chunked
 * and overlapped: memcpy(host→pinned chunk) runs while the previous
 * chunk's hipMemcpyAsync is in flight. Replaces the pandas/pageable path
 * for parquet ingest. */
extern "C" int dsx_upload_pinned(DsxCtx* c, const void* host, int64_t bytes,
                                 void** out_dev) {
  int rc = pool_alloc(c, bytes, out_dev);
  if (rc) return rc;
  const int64_t CHUNK = 32ll << 20;  // two 32-MiB halves
  if (c->pinned_bytes < 2 * CHUNK) {
    if (c->pinned) hipHostFree(c->pinned);
    HIP_TRY(hipHostMalloc(&c->pinned, 2 * CHUNK));
    c->pinned_bytes = 2 * CHUNK;
  }
  char* halves[2] = {(char*)c->pinned, (char*)c->pinned + CHUNK};
  hipEvent_t done[2];
  HIP_TRY(hipEventCreate(&done[0]));
  HIP_TRY(hipEventCreate(&done[1]));
  int flip = 0;
  bool used[2] = {false, false};
  for (int64_t off = 0; off < bytes; off += CHUNK, flip ^= 1) {
    int64_t n = bytes - off < CHUNK ? bytes - off : CHUNK;
    if (used[flip]) HIP_TRY(hipEventSynchronize(done[flip]));
    memcpy(halves[flip], (const char*)host + off, (size_t)n);
    HIP_TRY(hipMemcpyAsync((char*)*out_dev + off, halves[flip], (size_t)n,
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(done[flip], c->stream));
    used[flip] = true;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  hipEventDestroy(done[0]);
  hipEventDestroy(done[1]);
  return 0;
}

extern "C" int dsx_download(DsxCtx* c, const void* dev, void* host,
                            int64_t bytes) {
  HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// profiling ------------------------------------------------------------------
extern "C" int dsx_prof_enable(DsxCtx* c, int enable) {
  c->prof = enable != 0;
  return 0;
}
extern "C" int dsx_prof_reset(DsxCtx* c) {
  hipStreamSynchronize(c->stream);
  for (auto& r : c->prof_recs) {
    hipEventDestroy(r.start);
    hipEventDestroy(r.stop);
  }
  c->prof_recs.clear();
  return 0;
}
extern "C" int dsx_prof_get(DsxCtx* c, char names[][32], double* total_ms,
                            int64_t* launches, int cap) {
  hipStreamSynchronize(c->stream);
  // aggregate by name
  std::vector<std::string> seen;
  std::vector<double> ms;
  std::vector<int64_t> cnt;
  for (auto& r : c->prof_recs) {
    float el = 0.f;
    hipEventElapsedTime(&el, r.start, r.stop);
    size_t i = 0;
    for (; i < seen.size(); i++)
      if (seen[i] == r.name) break;
    if (i == seen.size()) {
      seen.push_back(r.name);
      ms.push_back(0);
      cnt.push_back(0);
    }
    ms[i] += el;
    cnt[i]++;
  }
  int n = (int)seen.size() < cap ? (int)seen.size() : cap;
  for (int i = 0; i < n; i++) {
    snprintf(names[i], 32, "%s", seen[i].c_str());
    total_ms[i] = ms[i];
    launches[i] = cnt[i];
  }
  return n;
}

struct ProfScope {
  DsxCtx* c;
  bool on;
  ProfScope(DsxCtx* ctx, const char* name) : c(ctx), on(ctx->prof) {
    if (!on) return;
    ProfRec r{};
    snprintf(r.name, sizeof(r.name), "%s", name);
    hipEventCreate(&r.start);
    hipEventCreate(&r.stop);
    hipEventRecord(r.start, c->stream);
    c->prof_recs.push_back(r);
  }
  ~ProfScope() {
    if (on) hipEventRecord(c->prof_recs.back().stop, c->stream);
  }
};

// ---------------------------------------------------------------------------
// expression VM (device) — typed postfix with SQL 3-valued logic
// (reference rex/core/call.py:1047-1156 op semantics; ReduceOperation
//  comparisons :1050-1062; NULL propagation as pandas does on the same ops)
// ---------------------------------------------------------------------------
struct ColsArg {
  const void* data[DSX_MAX_COLS];
  const uint8_t* validity[DSX_MAX_COLS];
  int32_t dtype[DSX_MAX_COLS];
  int32_t ncols;
};

union Slot {
  double f;
  int64_t i;
};

__device__ __forceinline__ void vm_load_col(const ColsArg& C, int ci,
                                            int64_t r, Slot& v, bool& valid) {
  valid = C.validity[ci] ? (C.validity[ci][r] != 0) : true;
  switch (C.dtype[ci]) {
    case DSX_I64: v.i = ((const int64_t*)C.data[ci])[r]; break;
    case DSX_F64: v.f = ((const double*)C.data[ci])[r]; break;
    case DSX_I32: v.i = (int64_t)((const int32_t*)C.data[ci])[r]; break;
    case DSX_F32: v.f = (double)((const float*)C.data[ci])[r]; break;
    case DSX_I8:  v.i = (int64_t)((const int8_t*)C.data[ci])[r]; break;
    case DSX_BOOL8: v.i = (int64_t)((const uint8_t*)C.data[ci])[r]; break;
    default: v.i = 0; valid = false;
  }
}

// civil date from days-since-epoch (Howard Hinnant's algorithm; the
// reference gets this from pandas datetime64[D] → .dt.year/month/day,
// rex/core/call.py date extraction)
__device__ __forceinline__ void civil_from_days(int64_t days, int& y, int& m,
                                                int& d) {
  int64_t z = days + 719468;
  int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  int64_t doe = z - era * 146097;
  int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  int64_t yy = yoe + era * 400;
  int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  int64_t mp = (5 * doy + 2) / 153;
  d = (int)(doy - (153 * mp + 2) / 5 + 1);
  m = (int)(mp < 10 ? mp + 3 : mp - 9);
  y = (int)(yy + (m <= 2));
}

// VM stack lives in NAMED registers: `sp` is wave-uniform (every lane runs
// the same program), so the switch below lowers to scalar branches and the
// slots stay in VGPRs — a runtime-indexed local array would spill every
// push/pop to scratch (cdna_hip_programming.md §5.4 rule 20; measured
// 224 B/lane of scratch before this change). Host compiler enforces
// depth ≤ 8 (runtime.py make_prog).
struct VmStack {
  Slot s0, s1, s2, s3, s4, s5, s6, s7;
  bool v0, v1, v2, v3, v4, v5, v6, v7;
  __device__ __forceinline__ void set(int i, Slot s, bool v) {
    switch (i) {
      case 0: s0 = s; v0 = v; break;
      case 1: s1 = s; v1 = v; break;
      case 2: s2 = s; v2 = v; break;
      case 3: s3 = s; v3 = v; break;
      case 4: s4 = s; v4 = v; break;
      case 5: s5 = s; v5 = v; break;
      case 6: s6 = s; v6 = v; break;
      default: s7 = s; v7 = v; break;
    }
  }
  __device__ __forceinline__ void get(int i, Slot& s, bool& v) const {
    switch (i) {
      case 0: s = s0; v = v0; break;
      case 1: s = s1; v = v1; break;
      case 2: s = s2; v = v2; break;
      case 3: s = s3; v = v3; break;
      case 4: s = s4; v = v4; break;
      case 5: s = s5; v = v5; break;
      case 6: s = s6; v = v6; break;
      default: s = s7; v = v7; break;
    }
  }
};

// returns value in out, validity flag as return
// returns value in out, validity flag as return
//
// LITE drops the ops that compile to long routines (64-bit integer and f64
// division, sqrt, exp/log/pow, trigonometry, civil dates): with them inlined
// a kernel needs 128 VGPRs plus scratch and runs at half occupancy. A kernel
// instantiates both and the host picks by vm_prog_is_lite(); a LITE
// evaluator handed such an op yields NULL like any unknown op.
template <bool LITE = false>
__device__ __forceinline__ bool vm_eval(const DsxInstr* prog, int len, const ColsArg& C,
                        int64_t r, Slot& out) {
  VmStack k;
  int sp = 0;
  for (int pc = 0; pc < len; pc++) {
    const DsxInstr raw = prog[pc];
    // the program is wave-uniform (all lanes execute the same instruction
    // stream) but may have been loaded through vector loads (global-memory
    // programs); readfirstlane makes uniformity PROVABLE so the switch is a
    // scalar branch and kernarg structs are scalar-indexed instead of being
    // privatized to scratch (cdna_hip_programming.md T20 recipe).
    const int op = __builtin_amdgcn_readfirstlane(raw.op);
    const int arg0 = __builtin_amdgcn_readfirstlane(raw.arg0);
    const int64_t imm =
        ((int64_t)__builtin_amdgcn_readfirstlane((int)(raw.imm >> 32))
         << 32) |
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(raw.imm & 0xFFFFFFFF));
    Slot a, b, c, res;
    bool av, bv, cv, rv;
    switch (op) {
      case DSX_OP_COL:
        vm_load_col(C, arg0, r, res, rv);
        k.set(sp++, res, rv);
        break;
      case DSX_OP_LIT_F64:
      case DSX_OP_LIT_I64:
        res.i = imm;
        k.set(sp++, res, true);
        break;
      case DSX_OP_LIT_NULL:
        res.i = 0;
        k.set(sp++, res, false);
        break;
#define POP2()                                                                 \
  k.get(sp - 2, a, av);                                                        \
  k.get(sp - 1, b, bv);                                                        \
  sp--;
#define VM_HEAVY()                                                             \
  if (LITE) {                                                                  \
    out.i = 0;                                                                 \
    return false;                                                              \
  }
#define BIN_F(OP, EXPR)                                                        \
  case OP: {                                                                   \
    POP2();                                                                    \
    res.EXPR;                                                                  \
    k.set(sp - 1, res, av && bv);                                              \
  } break;
#define BIN_H(OP, EXPR)                                                        \
  case OP: {                                                                   \
    VM_HEAVY();                                                                \
    POP2();                                                                    \
    res.EXPR;                                                                  \
    k.set(sp - 1, res, av && bv);                                              \
  } break;
      BIN_F(DSX_OP_ADD_F64, f = a.f + b.f)
      BIN_F(DSX_OP_SUB_F64, f = a.f - b.f)
      BIN_F(DSX_OP_MUL_F64, f = a.f * b.f)
      BIN_H(DSX_OP_DIV_F64, f = a.f / b.f)
      BIN_F(DSX_OP_LT_F64, i = (a.f < b.f) ? 1 : 0)
      BIN_F(DSX_OP_LE_F64, i = (a.f <= b.f) ? 1 : 0)
      BIN_F(DSX_OP_GT_F64, i = (a.f > b.f) ? 1 : 0)
      BIN_F(DSX_OP_GE_F64, i = (a.f >= b.f) ? 1 : 0)
      BIN_F(DSX_OP_EQ_F64, i = (a.f == b.f) ? 1 : 0)
      BIN_F(DSX_OP_NE_F64, i = (a.f != b.f) ? 1 : 0)
      BIN_F(DSX_OP_ADD_I64, i = a.i + b.i)
      BIN_F(DSX_OP_SUB_I64, i = a.i - b.i)
      BIN_F(DSX_OP_MUL_I64, i = a.i * b.i)
      BIN_H(DSX_OP_DIV_I64, i = b.i ? a.i / b.i : 0)
      BIN_H(DSX_OP_MOD_I64, i = b.i ? a.i % b.i : 0)
      BIN_H(DSX_OP_FLOORMOD_I64, i = b.i ? ((a.i % b.i) + b.i) % b.i : 0)
      BIN_F(DSX_OP_LT_I64, i = (a.i < b.i) ? 1 : 0)
      BIN_F(DSX_OP_LE_I64, i = (a.i <= b.i) ? 1 : 0)
      BIN_F(DSX_OP_GT_I64, i = (a.i > b.i) ? 1 : 0)
      BIN_F(DSX_OP_GE_I64, i = (a.i >= b.i) ? 1 : 0)
      BIN_F(DSX_OP_EQ_I64, i = (a.i == b.i) ? 1 : 0)
      BIN_F(DSX_OP_NE_I64, i = (a.i != b.i) ? 1 : 0)
#undef BIN_F
#undef BIN_H
      case DSX_OP_AND: {
        // SQL 3-valued: F if either F; NULL if any NULL else T
        POP2();
        bool fa = av && a.i == 0, fb = bv && b.i == 0;
        bool false_wins = fa || fb;
        res.i = (!false_wins && av && bv) ? 1 : 0;
        k.set(sp - 1, res, false_wins || (av && bv));
        break;
      }
      case DSX_OP_OR: {
        POP2();
        bool ta = av && a.i != 0, tb = bv && b.i != 0;
        bool true_wins = ta || tb;
        res.i = true_wins ? 1 : 0;
        k.set(sp - 1, res, true_wins || (av && bv));
        break;
      }
#undef POP2
#define UN()                                                                   \
  k.get(sp - 1, a, av);
      case DSX_OP_NOT:
        UN();
        res.i = a.i ? 0 : 1;
        k.set(sp - 1, res, av);  // validity unchanged
        break;
      case DSX_OP_IS_NULL:
        UN();
        res.i = av ? 0 : 1;
        k.set(sp - 1, res, true);
        break;
      case DSX_OP_IS_NOT_NULL:
        UN();
        res.i = av ? 1 : 0;
        k.set(sp - 1, res, true);
        break;
      case DSX_OP_I64_TO_F64:
        UN();
        res.f = (double)a.i;
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_F64_TO_I64:
        UN();
        res.i = (int64_t)a.f;  // trunc, mappings.py:346-353
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_BITS_F64:
        UN();
        res.f = __longlong_as_double(a.i);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_ABS_I64:
        UN();
        res.i = a.i < 0 ? -a.i : a.i;
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_ABS_F64:
        UN();
        res.f = fabs(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_FLOOR_F64:
        UN();
        res.f = floor(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_CEIL_F64:
        UN();
        res.f = ceil(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_RINT_F64:  // ties-to-even, numpy round (call.py round op)
        UN();
        res.f = rint(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_EXP_F64:
        VM_HEAVY();
        UN();
        res.f = exp(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_LN_F64:
        VM_HEAVY();
        UN();
        res.f = log(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_POW_F64:
        VM_HEAVY();
        k.get(--sp, b, bv);
        k.get(sp - 1, a, av);
        res.f = pow(a.f, b.f);
        k.set(sp - 1, res, av && bv);
        break;
      case DSX_OP_YEAR:
      case DSX_OP_MONTH:
      case DSX_OP_DAY: {
        VM_HEAVY();
        UN();
        int y, m, d;
        civil_from_days(a.i, y, m, d);
        res.i = op == DSX_OP_YEAR ? y : op == DSX_OP_MONTH ? m : d;
        k.set(sp - 1, res, av);
        break;
      }
      case DSX_OP_NEG_F64:
        UN();
        res.f = -a.f;
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_SQRT_F64:
        VM_HEAVY();
        UN();
        res.f = sqrt(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_NEG_I64:
        UN();
        res.i = -a.i;
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_SIN_F64:
        VM_HEAVY();
        UN();
        res.f = sin(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_COS_F64:
        VM_HEAVY();
        UN();
        res.f = cos(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_TAN_F64:
        VM_HEAVY();
        UN();
        res.f = tan(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_ASIN_F64:
        VM_HEAVY();
        UN();
        res.f = asin(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_ACOS_F64:
        VM_HEAVY();
        UN();
        res.f = acos(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_ATAN_F64:
        VM_HEAVY();
        UN();
        res.f = atan(a.f);
        k.set(sp - 1, res, av);
        break;
      case DSX_OP_ATAN2_F64:
        VM_HEAVY();
        k.get(--sp, b, bv);
        k.get(sp - 1, a, av);
        res.f = atan2(a.f, b.f);
        k.set(sp - 1, res, av && bv);
        break;
#undef UN
#undef VM_HEAVY
      case DSX_OP_SELECT: {
        // (cond, a, b): cond true→a, false/NULL→b (CASE WHEN semantics)
        k.get(sp - 3, c, cv);
        k.get(sp - 2, a, av);
        k.get(sp - 1, b, bv);
        sp -= 2;
        bool take = cv && c.i != 0;
        k.set(sp - 1, take ? a : b, take ? av : bv);
        break;
      }
      default:
        out.i = 0;
        return false;
    }
  }
  {
    Slot s;
    bool v;
    k.get(0, s, v);
    out = s;
    return v;
  }
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// contiguous per-block row range (coalesced; XCD-friendly: big linear chunks
// keep each XCD's L2 on its own slice)
__device__ __forceinline__ void block_range(int64_t n, int64_t unit,
                                            int64_t& lo, int64_t& hi) {
  int64_t nu = (n + unit - 1) / unit;  // units of `unit` rows
  int64_t per = (nu + gridDim.x - 1) / gridDim.x;
  lo = (int64_t)blockIdx.x * per * unit;
  hi = min(n, (lo + per * unit));
  if (lo > n) lo = n;
}

struct ProgArg {
  DsxInstr ins[DSX_MAX_PROG];
  int32_t len;
};

// no op that vm_eval<true> leaves out (see vm_eval)
static bool vm_prog_is_lite(const DsxInstr* prog, int len) {
  for (int i = 0; i < len; i++) {
    switch (prog[i].op) {
      case DSX_OP_DIV_F64: case DSX_OP_DIV_I64: case DSX_OP_MOD_I64:
      case DSX_OP_FLOORMOD_I64: case DSX_OP_SQRT_F64: case DSX_OP_EXP_F64:
      case DSX_OP_LN_F64: case DSX_OP_POW_F64: case DSX_OP_YEAR:
      case DSX_OP_MONTH: case DSX_OP_DAY: case DSX_OP_SIN_F64:
      case DSX_OP_COS_F64: case DSX_OP_TAN_F64: case DSX_OP_ASIN_F64:
      case DSX_OP_ACOS_F64: case DSX_OP_ATAN_F64: case DSX_OP_ATAN2_F64:
        return false;
      default:
        break;
    }
  }
  return true;
}

// ---------------------------------------------------------------------------
// dsx_eval — projection (project.py:56-65)
// ---------------------------------------------------------------------------
__global__ void k_eval(ProgArg prog, ColsArg C, int64_t n, void* out,
                       uint8_t* out_validity, int32_t out_dtype) {
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    Slot v;
    bool valid = vm_eval(prog.ins, prog.len, C, r, v);
    switch (out_dtype) {
      case DSX_F64: ((double*)out)[r] = valid ? v.f : __builtin_nan(""); break;
      case DSX_I64: ((int64_t*)out)[r] = v.i; break;
      case DSX_BOOL8: ((uint8_t*)out)[r] = (valid && v.i) ? 1 : 0; break;
    }
    if (out_validity) out_validity[r] = valid ? 1 : 0;
  }
}

extern "C" int dsx_eval(DsxCtx* c, const DsxInstr* prog, int prog_len,
                        const DsxColumn* cols, int ncols, int64_t n,
                        void* out_data, uint8_t* out_validity,
                        int32_t out_dtype) {
  if (prog_len > DSX_MAX_PROG || ncols > DSX_MAX_COLS)
    FAIL(-3, "program/cols too large");
  ProgArg P{};
  memcpy(P.ins, prog, prog_len * sizeof(DsxInstr));
  P.len = prog_len;
  ColsArg C{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    C.data[i] = cols[i].data;
    C.validity[i] = cols[i].validity;
    C.dtype[i] = cols[i].dtype;
  }
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  if (grid == 0) return 0;
  ProfScope ps(c, "k_eval");
  hipLaunchKernelGGL(k_eval, dim3(grid), dim3(BLOCK), 0, c->stream, P, C, n,
                     out_data, out_validity, out_dtype);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// dsx_filter — predicate + ORDER-PRESERVING compaction (filter.py:20-45)
// two passes over a wave64 ballot bitmask
// ---------------------------------------------------------------------------
template <bool LITE>
__global__ void k_filter_mask(ProgArg prog, ColsArg C, int64_t n,
                              uint64_t* mask, int64_t* block_counts) {
  int64_t lo, hi;
  block_range(n, 64, lo, hi);
  __shared__ int64_t s_count;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  int lane = threadIdx.x & 63;
  int64_t local = 0;
  // each wave owns consecutive 64-row words. NB: an idle block has lo
  // clamped to n, and floor(n/64) would alias the last partial word when
  // n % 64 != 0 — every idle block would re-count its bits (observed +470
  // rows at 1.5M/2048 blocks). Round UP so lo==hi ⇒ no words.
  for (int64_t w = (lo + 63) / 64 + threadIdx.x / 64; w * 64 < hi;
       w += WAVES_PER_BLOCK) {
    int64_t r = w * 64 + lane;
    bool pred = false;
    if (r < n) {
      Slot v;
      bool valid = vm_eval<LITE>(prog.ins, prog.len, C, r, v);
      pred = valid && v.i != 0;  // NULL → False (filter.py:39)
    }
    uint64_t m = __ballot(pred);
    if (lane == 0) {
      mask[w] = m;
      local += __popcll(m);
    }
  }
  if (lane == 0) atomicAdd((unsigned long long*)&s_count, (unsigned long long)local);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s_count;
}

// single-block exclusive scan of block_counts (grid ≤ 4096). Parallel
// Hillis-Steele with ≤4 elements per thread in named scalars — the serial
// thread-0 version measured 220 µs/launch at grid 2048 (pure dependent-load
// latency), ~1 ms/step on Q3's five filter/probe scans.
__global__ void k_scan_block_counts(int64_t* counts, int nblocks,
                                    int64_t* total) {
  __shared__ int64_t s[4096];
  int i0 = threadIdx.x, i1 = i0 + 1024, i2 = i0 + 2048, i3 = i0 + 3072;
  if (i0 < nblocks) s[i0] = counts[i0];
  if (i1 < nblocks) s[i1] = counts[i1];
  if (i2 < nblocks) s[i2] = counts[i2];
  if (i3 < nblocks) s[i3] = counts[i3];
  __syncthreads();
  for (int d = 1; d < nblocks; d <<= 1) {
    int64_t v0 = (i0 < nblocks && i0 >= d) ? s[i0 - d] : 0;
    int64_t v1 = (i1 < nblocks && i1 >= d) ? s[i1 - d] : 0;
    int64_t v2 = (i2 < nblocks && i2 >= d) ? s[i2 - d] : 0;
    int64_t v3 = (i3 < nblocks && i3 >= d) ? s[i3 - d] : 0;
    __syncthreads();
    if (i0 < nblocks) s[i0] += v0;
    if (i1 < nblocks) s[i1] += v1;
    if (i2 < nblocks) s[i2] += v2;
    if (i3 < nblocks) s[i3] += v3;
    __syncthreads();
  }
  if (i0 < nblocks) counts[i0] = s[i0] - counts[i0];
  if (i1 < nblocks) counts[i1] = s[i1] - counts[i1];
  if (i2 < nblocks) counts[i2] = s[i2] - counts[i2];
  if (i3 < nblocks) counts[i3] = s[i3] - counts[i3];
  if (i0 == 0) *total = nblocks > 0 ? s[nblocks - 1] : 0;
}

__global__ void k_filter_emit(const uint64_t* mask, int64_t n,
                              const int64_t* block_offsets, uint32_t* out_sel) {
  int64_t lo, hi;
  block_range(n, 64, lo, hi);
  __shared__ int64_t s_prefix[BLOCK];
  __shared__ int64_t s_running;
  if (threadIdx.x == 0) s_running = block_offsets[blockIdx.x];
  __syncthreads();
  int64_t w0 = lo / 64;
  int64_t nw = (hi - lo + 63) / 64;
  for (int64_t base = 0; base < nw; base += BLOCK) {
    int64_t w = w0 + base + threadIdx.x;
    uint64_t m = (base + threadIdx.x < nw) ? mask[w] : 0;
    int cnt = __popcll(m);
    // block-wide exclusive scan over the 256 word-counts (Hillis-Steele)
    s_prefix[threadIdx.x] = cnt;
    __syncthreads();
    for (int d = 1; d < BLOCK; d <<= 1) {
      int64_t v = (threadIdx.x >= d) ? s_prefix[threadIdx.x - d] : 0;
      __syncthreads();
      s_prefix[threadIdx.x] += v;
      __syncthreads();
    }
    int64_t excl = s_prefix[threadIdx.x] - cnt;
    int64_t off = s_running + excl;
    while (m) {
      int b = __ffsll((unsigned long long)m) - 1;
      out_sel[off++] = (uint32_t)(w * 64 + b);
      m &= m - 1;
    }
    __syncthreads();
    if (threadIdx.x == BLOCK - 1) s_running += s_prefix[threadIdx.x];
    __syncthreads();
  }
}

// fused filter emit + materialization: like k_filter_emit but writes the
// output columns directly (FilterMatArg reuses JoinMatArg with side=0) —
// replaces the per-column gathers of `df[cond]` (filter.py:40) with one
// order-preserving pass.
struct FilterMatArg {
  const void* src[16];
  const uint8_t* srcv[16];
  void* dst[16];
  uint8_t* dstv[16];
  int32_t dtype[16];
  int32_t ncols;
};

__device__ __forceinline__ void fm_write(const FilterMatArg& M, int64_t o,
                                         int64_t r) {
  for (int ci = 0; ci < M.ncols; ci++) {
    switch (M.dtype[ci]) {
      case DSX_I64:
        ((int64_t*)M.dst[ci])[o] = ((const int64_t*)M.src[ci])[r];
        break;
      case DSX_F64:
        ((double*)M.dst[ci])[o] = ((const double*)M.src[ci])[r];
        break;
      case DSX_I32:
        ((int32_t*)M.dst[ci])[o] = ((const int32_t*)M.src[ci])[r];
        break;
      case DSX_F32:
        ((float*)M.dst[ci])[o] = ((const float*)M.src[ci])[r];
        break;
      default:
        ((int8_t*)M.dst[ci])[o] = ((const int8_t*)M.src[ci])[r];
    }
    if (M.dstv[ci]) M.dstv[ci][o] = M.srcv[ci] ? M.srcv[ci][r] : 1;
  }
}

__global__ void k_filter_emit_cols(const uint64_t* mask, int64_t n,
                                   const int64_t* block_offsets,
                                   const FilterMatArg* Mp) {
  // one row per lane, wave-ballot compaction: selected lanes of a wave
  // write CONSECUTIVE output slots in one store instruction (the
  // bit-serial per-thread walk scattered every wave store across ~64
  // cache lines — measured 1.7 ms vs this version on the Q3 filters)
  int64_t lo, hi;
  block_range(n, 64, lo, hi);  // 64-aligned lo: a wave shares one word
  __shared__ int64_t s_running;
  __shared__ int s_wave[BLOCK / 64 + 1];
  __shared__ FilterMatArg s_M;  // LDS copy (see k_hash_probe_mat note)
  if (threadIdx.x == 0) {
    s_running = block_offsets[blockIdx.x];
    s_M = *Mp;
  }
  __syncthreads();
  const FilterMatArg& M = s_M;
  int lane = threadIdx.x & 63;
  int wid = threadIdx.x >> 6;
  for (int64_t base = lo; base < hi; base += BLOCK) {
    int64_t r = base + threadIdx.x;
    bool sel = false;
    if (r < hi) sel = (mask[r >> 6] >> (r & 63)) & 1;
    uint64_t ball = __ballot(sel);
    if (lane == 0) s_wave[wid] = __popcll(ball);
    __syncthreads();
    if (threadIdx.x == 0) {
      int run = 0;
      for (int i = 0; i < BLOCK / 64; i++) {
        int v = s_wave[i];
        s_wave[i] = run;
        run += v;
      }
      s_wave[BLOCK / 64] = run;
    }
    __syncthreads();
    if (sel) {
      int64_t o = s_running + s_wave[wid] +
                  __popcll(ball & ((1ull << lane) - 1));
      fm_write(M, o, r);
    }
    __syncthreads();
    if (threadIdx.x == 0) s_running += s_wave[BLOCK / 64];
    __syncthreads();
  }
}

/* fused filter + materialization: evaluate the predicate, then write the
 * selected rows of the given columns directly (no selection vector, no
 * per-column gathers). Outputs pool-allocated like dsx_hash_probe_cols. */
extern "C" int dsx_filter_cols(DsxCtx* c, const DsxInstr* prog, int prog_len,
                               const DsxColumn* cols, int ncols, int64_t n,
                               const DsxColumn* mats, int nmats,
                               void** out_datas, uint8_t** out_valids,
                               int64_t* out_count) {
  if (prog_len > DSX_MAX_PROG || ncols > DSX_MAX_COLS)
    FAIL(-3, "filter spec too large");
  if (nmats > 16) FAIL(-3, "too many filter output columns");
  *out_count = 0;
  ProgArg P{};
  memcpy(P.ins, prog, prog_len * sizeof(DsxInstr));
  P.len = prog_len;
  ColsArg C{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    C.data[i] = cols[i].data;
    C.validity[i] = cols[i].validity;
    C.dtype[i] = cols[i].dtype;
  }
  int64_t nwords = (n + 63) / 64;
  int grid = (int)min((int64_t)MAX_GRID, (nwords + WAVES_PER_BLOCK - 1) /
                                             WAVES_PER_BLOCK);
  int64_t arg_off = nwords * 8 + (grid + 2) * 8 + 64;
  int rc = ensure_scratch(c, arg_off + (int64_t)sizeof(FilterMatArg) + 64);
  if (rc) return rc;
  uint64_t* mask = (uint64_t*)c->scratch;
  int64_t* block_counts = (int64_t*)(mask + nwords);
  int64_t* total = block_counts + grid;
  FilterMatArg* d_M =
      (FilterMatArg*)((char*)c->scratch + ((arg_off + 63) / 64) * 64);
  if (grid > 0) {
    ProfScope ps(c, "k_filter_mask");
    hipLaunchKernelGGL(vm_prog_is_lite(prog, prog_len) ? k_filter_mask<true>
                                                       : k_filter_mask<false>,
                       dim3(grid), dim3(BLOCK), 0, c->stream, P, C, n, mask,
                       block_counts);
  }
  hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream,
                     block_counts, grid, total);
  int64_t h_total = 0;
  HIP_TRY(hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  FilterMatArg M{};
  M.ncols = nmats;
  int64_t tsz = h_total > 0 ? h_total : 1;
  for (int i = 0; i < nmats; i++) {
    int esz = mats[i].dtype == DSX_I64 || mats[i].dtype == DSX_F64 ? 8
              : mats[i].dtype == DSX_I32 || mats[i].dtype == DSX_F32 ? 4 : 1;
    int rc2 = pool_alloc(c, tsz * esz, &out_datas[i]);
    if (rc2) return rc2;
    out_valids[i] = nullptr;
    if (mats[i].validity) {
      void* vp = nullptr;
      rc2 = pool_alloc(c, tsz, &vp);
      if (rc2) return rc2;
      out_valids[i] = (uint8_t*)vp;
    }
    M.src[i] = mats[i].data;
    M.srcv[i] = mats[i].validity;
    M.dst[i] = out_datas[i];
    M.dstv[i] = out_valids[i];
    M.dtype[i] = mats[i].dtype;
  }
  HIP_TRY(hipMemcpyAsync(d_M, &M, sizeof(FilterMatArg), hipMemcpyHostToDevice,
                         c->stream));
  if (h_total > 0 && grid > 0) {
    ProfScope ps(c, "k_filter_emit_cols");
    hipLaunchKernelGGL(k_filter_emit_cols, dim3(grid), dim3(BLOCK), 0,
                       c->stream, mask, n, block_counts, d_M);
  }
  HIP_TRY(hipGetLastError());
  *out_count = h_total;
  return dbg_check(c, "dsx_filter_cols");
}

extern "C" int dsx_filter(DsxCtx* c, const DsxInstr* prog, int prog_len,
                          const DsxColumn* cols, int ncols, int64_t n,
                          uint32_t** out_sel, int64_t* out_count) {
  if (prog_len > DSX_MAX_PROG || ncols > DSX_MAX_COLS)
    FAIL(-3, "program/cols too large");
  if (n > 0xFFFFFFFFll) FAIL(-3, "partition too large for u32 row ids");
  *out_sel = nullptr;
  *out_count = 0;
  if (n == 0) {
    return pool_alloc(c, 4, (void**)out_sel);
  }
  ProgArg P{};
  memcpy(P.ins, prog, prog_len * sizeof(DsxInstr));
  P.len = prog_len;
  ColsArg C{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    C.data[i] = cols[i].data;
    C.validity[i] = cols[i].validity;
    C.dtype[i] = cols[i].dtype;
  }
  int64_t nwords = (n + 63) / 64;
  int grid = (int)min((int64_t)MAX_GRID, (nwords + WAVES_PER_BLOCK - 1) /
                                             WAVES_PER_BLOCK);
  int64_t scratch_need = nwords * 8 + (grid + 1) * 8 + 8;
  int rc = ensure_scratch(c, scratch_need);
  if (rc) return rc;
  uint64_t* mask = (uint64_t*)c->scratch;
  int64_t* block_counts = (int64_t*)(mask + nwords);
  int64_t* total = block_counts + grid;
  {
    ProfScope ps(c, "k_filter_mask");
    hipLaunchKernelGGL(vm_prog_is_lite(prog, prog_len) ? k_filter_mask<true>
                                                       : k_filter_mask<false>,
                       dim3(grid), dim3(BLOCK), 0, c->stream, P, C, n, mask,
                       block_counts);
  }
  hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream,
                     block_counts, grid, total);
  int64_t h_total = 0;
  HIP_TRY(hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  { int rc2 = pool_alloc(c, (h_total > 0 ? h_total : 1) * 4, (void**)out_sel); if (rc2) return rc2; }
  if (h_total > 0) {
    ProfScope ps(c, "k_filter_emit");
    hipLaunchKernelGGL(k_filter_emit, dim3(grid), dim3(BLOCK), 0, c->stream,
                       mask, n, block_counts, *out_sel);
  }
  HIP_TRY(hipGetLastError());
  *out_count = h_total;
  return 0;
}

// ---------------------------------------------------------------------------
// dsx_gather — boolean take / merge materialization
// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_gather(const T* in, const uint8_t* in_valid,
                         const uint32_t* sel, int64_t n, T* out,
                         uint8_t* out_valid, T null_fill, int64_t n_src,
                         unsigned int* dbg) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < n; i += stride) {
    uint32_t s = sel[i];
    if (s == DSX_NULL_IDX) {  // outer-join missing row → NULL (NaN fill,
                              // test_join.py:55-65)
      out[i] = null_fill;
      if (out_valid) out_valid[i] = 0;
    } else {
      if ((int64_t)s >= n_src) {  // corrupt selection vector: report, skip
        if (atomicOr(dbg, 1u) == 0) {
          dbg[1] = s;
          dbg[2] = (unsigned int)n_src;
          dbg[3] = (unsigned int)i;
        }
        out[i] = null_fill;
        if (out_valid) out_valid[i] = 0;
        continue;
      }
      out[i] = in[s];
      uint8_t v = in_valid ? in_valid[s] : 1;
      if (out_valid) out_valid[i] = v;
    }
  }
}

extern "C" int dsx_gather(DsxCtx* c, const DsxColumn* col, const uint32_t* sel,
                          int64_t n_sel, void* out_data, uint8_t* out_validity) {
  int grid = (int)min((int64_t)MAX_GRID, (n_sel + BLOCK - 1) / BLOCK);
  if (grid == 0) return 0;
  ProfScope ps(c, "k_gather");
  switch (col->dtype) {
    case DSX_I64:
      hipLaunchKernelGGL(k_gather<int64_t>, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const int64_t*)col->data, col->validity,
                         sel, n_sel, (int64_t*)out_data, out_validity, 0ll, col->len, c->dbg_flag);
      break;
    case DSX_F64:
      hipLaunchKernelGGL(k_gather<double>, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const double*)col->data, col->validity,
                         sel, n_sel, (double*)out_data, out_validity,
                         __builtin_nan(""), col->len, c->dbg_flag);
      break;
    case DSX_I32:
      hipLaunchKernelGGL(k_gather<int32_t>, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const int32_t*)col->data, col->validity,
                         sel, n_sel, (int32_t*)out_data, out_validity, 0, col->len, c->dbg_flag);
      break;
    case DSX_F32:
      hipLaunchKernelGGL(k_gather<float>, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const float*)col->data, col->validity, sel,
                         n_sel, (float*)out_data, out_validity,
                         __builtin_nanf(""), col->len, c->dbg_flag);
      break;
    case DSX_I8:
    case DSX_BOOL8:
      hipLaunchKernelGGL(k_gather<int8_t>, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const int8_t*)col->data, col->validity,
                         sel, n_sel, (int8_t*)out_data, out_validity,
                         (int8_t)0, col->len, c->dbg_flag);
      break;
    default:
      FAIL(-3, "gather: bad dtype %d", col->dtype);
  }
  HIP_TRY(hipGetLastError());
  return dbg_check(c, "dsx_gather");
}

extern "C" int dsx_memset(DsxCtx* c, void* dev, int value, int64_t bytes) {
  HIP_TRY(hipMemsetAsync(dev, value, (size_t)bytes, c->stream));
  return 0;
}

extern "C" int dsx_copy(DsxCtx* c, void* dst, const void* src,
                        int64_t bytes) {
  HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice,
                         c->stream));
  return 0;
}

// row scatter — inverse of gather: out[sel[i]] = in[i]. Places join-back /
// window columns into original row order (sel must be a permutation or a
// subset of [0, n_out); untouched out rows keep their init value).
template <typename T>
__global__ void k_scatter_rows(const T* in, const uint8_t* in_valid,
                               const uint32_t* sel, int64_t n, T* out,
                               uint8_t* out_valid, int64_t n_out,
                               unsigned int* dbg) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < n; i += stride) {
    uint32_t s = sel[i];
    if ((int64_t)s >= n_out) {
      if (atomicOr(dbg, 1u) == 0) {
        dbg[1] = s;
        dbg[2] = (unsigned int)n_out;
        dbg[3] = (unsigned int)i;
      }
      continue;
    }
    out[s] = in[i];
    if (out_valid) out_valid[s] = in_valid ? in_valid[i] : 1;
  }
}

extern "C" int dsx_scatter_rows(DsxCtx* c, const DsxColumn* col,
                                const uint32_t* sel, int64_t n_sel,
                                int64_t n_out, void* out_data,
                                uint8_t* out_validity) {
  int grid = (int)min((int64_t)MAX_GRID, (n_sel + BLOCK - 1) / BLOCK);
  if (grid == 0) return 0;
  ProfScope ps(c, "k_scatter_rows");
  switch (col->dtype) {
    case DSX_I64:
      hipLaunchKernelGGL(k_scatter_rows<int64_t>, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const int64_t*)col->data, col->validity,
                         sel, n_sel, (int64_t*)out_data, out_validity, n_out,
                         c->dbg_flag);
      break;
    case DSX_F64:
      hipLaunchKernelGGL(k_scatter_rows<double>, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const double*)col->data, col->validity,
                         sel, n_sel, (double*)out_data, out_validity, n_out,
                         c->dbg_flag);
      break;
    case DSX_I32:
      hipLaunchKernelGGL(k_scatter_rows<int32_t>, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const int32_t*)col->data, col->validity,
                         sel, n_sel, (int32_t*)out_data, out_validity, n_out,
                         c->dbg_flag);
      break;
    case DSX_F32:
      hipLaunchKernelGGL(k_scatter_rows<float>, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const float*)col->data, col->validity,
                         sel, n_sel, (float*)out_data, out_validity, n_out,
                         c->dbg_flag);
      break;
    case DSX_I8:
    case DSX_BOOL8:
      hipLaunchKernelGGL(k_scatter_rows<int8_t>, dim3(grid), dim3(BLOCK), 0,
                         c->stream, (const int8_t*)col->data, col->validity,
                         sel, n_sel, (int8_t*)out_data, out_validity, n_out,
                         c->dbg_flag);
      break;
    default:
      FAIL(-3, "scatter_rows: bad dtype %d", col->dtype);
  }
  HIP_TRY(hipGetLastError());
  return dbg_check(c, "dsx_scatter_rows");
}

// ---------------------------------------------------------------------------
// dsx_minmax_i64
// ---------------------------------------------------------------------------
__global__ void k_minmax_i64(ColsArg C, int64_t n, int64_t* out3) {
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  int64_t mn = INT64_MAX, mx = INT64_MIN, cnt = 0;
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    Slot v;
    bool valid;
    vm_load_col(C, 0, r, v, valid);
    if (valid) {
      mn = min(mn, v.i);
      mx = max(mx, v.i);
      cnt++;
    }
  }
  // wave reduce then global atomics
  for (int d = 32; d > 0; d >>= 1) {
    mn = min(mn, __shfl_down(mn, d, 64));
    mx = max(mx, __shfl_down(mx, d, 64));
    cnt += __shfl_down(cnt, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    // order-preserving u64 transform → unsigned atomics (portable)
    atomicMin((unsigned long long*)&out3[0],
              (unsigned long long)((uint64_t)mn ^ 0x8000000000000000ull));
    atomicMax((unsigned long long*)&out3[1],
              (unsigned long long)((uint64_t)mx ^ 0x8000000000000000ull));
    atomicAdd((unsigned long long*)&out3[2], (unsigned long long)cnt);
  }
}

extern "C" int dsx_minmax_i64(DsxCtx* c, const DsxColumn* col, int64_t* out_min,
                              int64_t* out_max, int64_t* out_nonnull) {
  ColsArg C{};
  C.ncols = 1;
  C.data[0] = col->data;
  C.validity[0] = col->validity;
  C.dtype[0] = col->dtype;
  int rc = ensure_scratch(c, 24);
  if (rc) return rc;
  // slots hold the order-preserving u64 transform of min/max
  uint64_t init[3] = {0xFFFFFFFFFFFFFFFFull, 0ull, 0ull};
  HIP_TRY(hipMemcpyAsync(c->scratch, init, 24, hipMemcpyHostToDevice,
                         c->stream));
  int grid = (int)min((int64_t)MAX_GRID, (col->len + BLOCK - 1) / BLOCK);
  if (grid > 0) {
    ProfScope ps(c, "k_minmax");
    hipLaunchKernelGGL(k_minmax_i64, dim3(grid), dim3(BLOCK), 0, c->stream, C,
                       col->len, (int64_t*)c->scratch);
  }
  uint64_t out[3];
  HIP_TRY(hipMemcpyAsync(out, c->scratch, 24, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *out_min = (int64_t)(out[0] ^ 0x8000000000000000ull);
  *out_max = (int64_t)(out[1] ^ 0x8000000000000000ull);
  *out_nonnull = (int64_t)out[2];
  return 0;
}

// ---------------------------------------------------------------------------
// dsx_keypack — composite keys → u64 codes (NULL gets code slot 0 per key)
// ---------------------------------------------------------------------------
struct KeyArg {
  DsxKeySpec k[DSX_MAX_KEYS];
  uint64_t stride[DSX_MAX_KEYS];
  int32_t nkeys;
};


__device__ __forceinline__ uint64_t pack_key(const KeyArg& K, const ColsArg& C,
                                             int64_t r) {
  // fully unrolled so K's fields scalarize into registers (a runtime-indexed
  // access would re-load the spec per row / spill — §5.4 rule 20)
  uint64_t code = 0;
#pragma unroll
  for (int j = 0; j < DSX_MAX_KEYS; j++) {
    if (j >= K.nkeys) break;
    Slot v;
    bool valid;
    vm_load_col(C, K.k[j].col, r, v, valid);
    uint64_t part;
    if (K.k[j].mode == 1) {
      // f64 bit-pattern key (single key): exact equality incl. -0.0==0.0;
      // NaN and NULL share code 0 (pandas NaN key group, dropna=False)
      double x = v.f;
      part = (!valid || x != x)
                 ? 0ull
                 : (uint64_t)__double_as_longlong(x == 0.0 ? 0.0 : x) + 1;
    } else if (K.k[j].mode & 2 || K.k[j].mode & 4) {
      // ORDER BY packing (dsx_sort_perm): mode bit1 = DESC (flip value
      // part), bit2 = NULLS LAST (NULL takes the TOP slot, else slot 0)
      uint64_t vp = (uint64_t)(v.i - K.k[j].min);
      if (K.k[j].mode & 2) vp = (uint64_t)(K.k[j].range - 1) - vp;
      if (K.k[j].nullable)
        part = (K.k[j].mode & 4) ? (valid ? vp : (uint64_t)K.k[j].range)
                                 : (valid ? vp + 1 : 0);
      else
        part = vp;
    } else if (K.k[j].nullable) {
      part = valid ? (uint64_t)(v.i - K.k[j].min) + 1 : 0;
    } else {
      part = (uint64_t)(v.i - K.k[j].min);
    }
    code += part * K.stride[j];
  }
  return code;
}

// false when any key column of row r is NULL (dsx_filter_probe_cols,
// dsx_hash_build_cols: such a row neither matches nor is inserted)
__device__ __forceinline__ bool fp_key_valid(const KeyArg& K, const ColsArg& C,
                                             int64_t r) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < DSX_MAX_KEYS; j++) {
    if (j >= K.nkeys) break;
    const uint8_t* v = C.validity[K.k[j].col];
    if (v && !v[r]) ok = false;  // NULL key never matches (join.py:202-213)
  }
  return ok;
}

__global__ void k_keypack(KeyArg K, ColsArg C, int64_t n, uint64_t* out) {
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    out[r] = pack_key(K, C, r);
  }
}

// per-key strides of the packed code (shared by every entry that packs keys,
// so their codes are bit-identical)
static int make_keyarg(const DsxKeySpec* keys, int nkeys, KeyArg& K) {
  K.nkeys = nkeys;
  uint64_t stride = 1;
  for (int j = 0; j < nkeys; j++) {
    K.k[j] = keys[j];
    K.stride[j] = stride;
    if (keys[j].mode == 1) {
      if (nkeys != 1) FAIL(-3, "f64-bits key must be the only key");
      continue;  // full u64 code space; stride stays 1
    }
    uint64_t range = (uint64_t)keys[j].range + (keys[j].nullable ? 1 : 0);
    if (range == 0) FAIL(-3, "empty key range");
    if (stride > (1ull << 62) / range) FAIL(-4, "key space exceeds 2^62");
    stride *= range;
  }
  return 0;
}

extern "C" int dsx_keypack(DsxCtx* c, const DsxColumn* cols, int ncols,
                           const DsxKeySpec* keys, int nkeys, int64_t n,
                           uint64_t* out_codes) {
  if (nkeys > DSX_MAX_KEYS || ncols > DSX_MAX_COLS) FAIL(-3, "too many keys");
  KeyArg K{};
  int rc = make_keyarg(keys, nkeys, K);
  if (rc) return rc;
  ColsArg C{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    C.data[i] = cols[i].data;
    C.validity[i] = cols[i].validity;
    C.dtype[i] = cols[i].dtype;
  }
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  if (grid == 0) return 0;
  ProfScope ps(c, "k_keypack");
  hipLaunchKernelGGL(k_keypack, dim3(grid), dim3(BLOCK), 0, c->stream, K, C, n,
                     out_codes);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// hash join (join.py:241-246 per-partition hash join)
// open-addressing multimap: CAS-claim on 64-bit code, linear probe;
// duplicates occupy separate slots; probe scans to first EMPTY.
// ---------------------------------------------------------------------------
struct DsxHashTable {
  uint64_t* keys = nullptr;   // EMPTY_KEY = empty; packed: (code<<32)|rowid
  uint32_t* vals = nullptr;   // build row id (unpacked layout only)
  uint32_t* matched = nullptr;  // per-slot marks of a mark_matched probe;
                                // allocated and cleared on first such use
                                // (hash_table_ensure_matched), else NULL
  int64_t slots = 0;
  int64_t n_build = 0;
  int packed = 0;             // codes < 2^32-1 → one 8-B entry per slot,
                              // single random read per probe
  unsigned int* dup = nullptr;  // device flag: any duplicate build key; its
                                // own allocation only when there is no filter
  // key-membership filter (join_filter.h), consulted by the filter-probe mask
  // pass only: most probes of a selective join end on an EMPTY slot, and a
  // filter small enough to stay in L2 answers those without a table line
  uint32_t* filter = nullptr;
  int filter_mode = DSX_JF_NONE;
  uint64_t filter_arg = 0;    // exact: code_max; hashed: word count - 1
  int64_t filter_bytes = 0;
  DsxCtx* ctx = nullptr;
};

// DSX_DISABLE_BUILD_RUNCOMBINE=1 (read per build): one filter atomic per row,
// as before the run combine — for measuring the combine on its own
static bool build_runcombine_enabled() {
  const char* e = getenv("DSX_DISABLE_BUILD_RUNCOMBINE");
  return !(e && *e && strcmp(e, "0") != 0);
}

// The build kernels' row step after the key code is known: the filter bit,
// then the CAS claim. EVERY lane of the wave calls it (`live` false for a row
// that is past the end, filtered out or has a NULL key), because the exact
// filter's bits are combined across the wave first: neighbouring lanes whose
// codes fall in the same filter word form a run, a segmented OR by shuffles
// (6 steps) collects the run's bits in its first lane, and only that lane
// issues the atomicOr. Sorted dense build keys then cost the two or three
// atomics of the words a wave's 64 codes span instead of 64; unsorted keys
// give runs of one and the atomics of before. Two separate runs of one word each issue their own OR, and a lane
// may pick up same-word bits from past its run: both leave the bitmap as it
// would be. Returns whether the row met an equal key in the table.
template <bool COMBINE>
__device__ __forceinline__ bool hb_insert_row(
    bool live, uint64_t cde, int64_t r, uint64_t* tkeys, uint32_t* tvals,
    int64_t mask, int packed, uint32_t* filter, int filter_mode,
    uint64_t filter_arg) {
  if (filter_mode == DSX_JF_EXACT) {
    // a code past code_max cannot come from a caller that keeps its own
    // bound; it is left out of the bitmap rather than written past it, and
    // the probe side treats such codes as misses
    bool in = live && cde <= filter_arg;
    if (COMBINE) {
      // exact mode implies a packed table: the word index fits 32 bits
      uint32_t word = in ? (uint32_t)dsx_jf_exact_word(cde) : 0xFFFFFFFFu;
      uint32_t bits = in ? dsx_jf_exact_bit(cde) : 0u;
      int lane = threadIdx.x & 63;
      uint32_t prev = __shfl_up(word, 1, 64);
      bool head = lane == 0 || prev != word;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        uint32_t w2 = __shfl_down(word, d, 64);
        uint32_t b2 = __shfl_down(bits, d, 64);
        if (lane + d < 64 && w2 == word) bits |= b2;
      }
      if (in && head) atomicOr(&filter[word], bits);
    } else if (in) {
      atomicOr(&filter[dsx_jf_exact_word(cde)], dsx_jf_exact_bit(cde));
    }
  } else if (filter_mode == DSX_JF_HASHED && live) {
    uint64_t h = dsx_jf_mix64(cde);
    atomicOr(&filter[dsx_jf_hashed_word(h, filter_arg)],
             dsx_jf_hashed_bits(h));
  }
  bool saw_dup = false;
  if (live) {
    uint64_t entry = packed ? ((cde << 32) | (uint64_t)(uint32_t)r) : cde;
    int64_t s = (int64_t)(mix64(cde) & mask);
    while (true) {
      unsigned long long old = atomicCAS((unsigned long long*)&tkeys[s],
                                         EMPTY_KEY,
                                         (unsigned long long)entry);
      if (old == EMPTY_KEY) {
        if (!packed)
          tvals[s] = (uint32_t)r;  // visible to later kernels via
                                   // end-of-kernel release (same stream)
        break;
      }
      // duplicate build keys disable the single-pass probe (PK-FK check)
      if ((packed ? (old >> 32) : old) == cde) saw_dup = true;
      s = (s + 1) & mask;
    }
  }
  return saw_dup;
}

// the row loop of both build kernels keeps whole waves together (the run
// combine shuffles across the wave): a wave leaves when its FIRST lane's row
// is past the block's range
template <bool COMBINE>
__global__ void k_hash_build(const uint64_t* codes, const uint8_t* validity,
                             int64_t n, uint64_t* tkeys, uint32_t* tvals,
                             int64_t mask, int packed, unsigned int* dup,
                             uint32_t* filter, int filter_mode,
                             uint64_t filter_arg) {
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  bool saw_dup = false;
  int lane = threadIdx.x & 63;
  for (int64_t r = lo + threadIdx.x; r - lane < hi; r += BLOCK) {
    // NULL-key drop (join.py:202-213)
    bool live = r < hi && !(validity && !validity[r]);
    uint64_t cde = live ? codes[r] : 0;
    saw_dup |= hb_insert_row<COMBINE>(live, cde, r, tkeys, tvals, mask, packed,
                                      filter, filter_mode, filter_arg);
  }
  if (saw_dup) atomicOr(dup, 1u);
}

// dsx_hash_build_cols: predicate → key validity → pack → insert, one sweep
// over the source columns; the stored row id is the source row's index
// launch bounds: the full interpreter (LITE false) needs more than the 128
// registers a 1024-thread default leaves it, and would spill
template <bool LITE, bool COMBINE>
__global__ void __launch_bounds__(BLOCK) k_hash_build_cols(ProgArg prog, KeyArg K, ColsArg C, int64_t n,
                                  uint64_t* tkeys, uint32_t* tvals,
                                  int64_t mask, int packed, unsigned int* dup,
                                  uint32_t* filter, int filter_mode,
                                  uint64_t filter_arg) {
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  bool saw_dup = false;
  int lane = threadIdx.x & 63;
  for (int64_t r = lo + threadIdx.x; r - lane < hi; r += BLOCK) {
    bool live = r < hi;
    if (live && prog.len > 0) {
      Slot v;
      bool valid = vm_eval<LITE>(prog.ins, prog.len, C, r, v);
      live = valid && v.i != 0;  // NULL → False
    }
    // NULL-key drop (join.py:202-213); such a row's code is garbage
    live = live && fp_key_valid(K, C, r);
    uint64_t cde = live ? pack_key(K, C, r) : 0;
    saw_dup |= hb_insert_row<COMBINE>(live, cde, r, tkeys, tvals, mask, packed,
                                      filter, filter_mode, filter_arg);
  }
  if (saw_dup) atomicOr(dup, 1u);
}

// read per call, so one process can run both variants (A/B, tests)
static bool join_filter_enabled() {
  const char* e = getenv("DSX_DISABLE_JOINFILTER");
  return !(e && *e && strcmp(e, "0") != 0);
}

// picks the filter of a table of n build rows: exact when the table is packed
// and code_max + 1 bits fit under the byte cap; else hashed at the next power
// of two >= DSX_JF_BITS_PER_KEY bits per row, clamped to the cap; no filter
// when the cap leaves fewer than the minimum bits per row (a saturated filter
// passes everything and only costs its load).
static void join_filter_plan(int64_t n, uint64_t code_max, int packed,
                             int* mode, uint64_t* arg, int64_t* bytes) {
  *mode = DSX_JF_NONE;
  *arg = 0;
  *bytes = 0;
  if (!join_filter_enabled()) return;
  int64_t cap = DSX_JOIN_FILTER_MAX_BYTES;
  if (const char* e = getenv("DSX_JOIN_FILTER_MAX_BYTES")) cap = atoll(e);
  int64_t min_bits = DSX_JF_MIN_BITS_PER_KEY;
  if (const char* e = getenv("DSX_JOIN_FILTER_MIN_BITS")) min_bits = atoll(e);
  if (packed && (int64_t)dsx_jf_exact_words(code_max) * 4 <= cap) {
    *mode = DSX_JF_EXACT;
    *arg = code_max;
    *bytes = (int64_t)dsx_jf_exact_words(code_max) * 4;
    return;
  }
  int64_t words = 1;  // 32 bits
  while (words * 32 < DSX_JF_BITS_PER_KEY * n) words <<= 1;
  while (words > 1 && words * 4 > cap) words >>= 1;
  if (words * 4 > cap || words * 32 < min_bits * n) return;
  *mode = DSX_JF_HASHED;
  *arg = (uint64_t)(words - 1);
  *bytes = words * 4;
}

// an empty table for n build rows, cleared on the context's stream: slots from
// n, layout from code_max, the filter from join_filter_plan. With a filter
// the dup flag is the word after the filter's last, so one clear covers both.
static int hash_table_new(DsxCtx* c, int64_t n, uint64_t code_max,
                          bool want_filter, DsxHashTable** out) {
  if (n > 0xFFFFFFFEll) FAIL(-3, "build side too large for u32 row ids");
  static const double slots_mult = [] {
    const char* e = getenv("DSX_JOIN_SLOTS_MULT");
    return e ? atof(e) : 2.0;
  }();
  int64_t slots = 64;
  while (slots < (int64_t)(slots_mult * n)) slots <<= 1;
  DsxHashTable* t = new DsxHashTable();
  t->slots = slots;
  t->n_build = n;
  t->ctx = c;
  // codes bounded below 2^32-1 → pack (code,rowid) into the claim word:
  // one random 8-B read per probe instead of two, half the table bytes
  t->packed = (code_max != 0 && code_max < 0xFFFFFFFEull) ? 1 : 0;
  if (want_filter) {
    join_filter_plan(n, code_max, t->packed, &t->filter_mode, &t->filter_arg,
                     &t->filter_bytes);
    c->join_filter_builds[t->filter_mode]++;
  }
  bool with_filter = t->filter_mode != DSX_JF_NONE;  // bytes: a multiple of 4
  if (pool_alloc(c, slots * 8, (void**)&t->keys) ||
      (!t->packed && pool_alloc(c, slots * 4, (void**)&t->vals)) ||
      (with_filter ? pool_alloc(c, t->filter_bytes + 4, (void**)&t->filter)
                   : pool_alloc(c, 4, (void**)&t->dup))) {
    dsx_hash_table_free(t);
    FAIL(-2, "hash table alloc failed (%lld slots)", (long long)slots);
  }
  if (with_filter) t->dup = t->filter + t->filter_bytes / 4;
  HIP_TRY(hipMemsetAsync(t->keys, 0xFF, slots * 8, c->stream));
  HIP_TRY(hipMemsetAsync(with_filter ? (void*)t->filter : (void*)t->dup, 0,
                         with_filter ? t->filter_bytes + 4 : 4, c->stream));
  *out = t;
  return 0;
}

static int hash_build_impl(DsxCtx* c, const uint64_t* codes,
                           const uint8_t* validity, int64_t n,
                           uint64_t code_max, bool want_filter,
                           DsxHashTable** out) {
  DsxHashTable* t = nullptr;
  int rc = hash_table_new(c, n, code_max, want_filter, &t);
  if (rc) return rc;
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  if (grid > 0) {
    ProfScope ps(c, "k_hash_build");
    hipLaunchKernelGGL(build_runcombine_enabled() ? k_hash_build<true>
                                                  : k_hash_build<false>,
                       dim3(grid), dim3(BLOCK), 0, c->stream, codes, validity,
                       n, t->keys, t->vals, t->slots - 1, t->packed, t->dup,
                       t->filter, t->filter_mode, t->filter_arg);
  }
  HIP_TRY(hipGetLastError());
  *out = t;
  return 0;
}

// One sweep over source columns that builds the table dsx_hash_build_filtered
// builds over the packed codes of the rows the predicate keeps: no compacted
// columns, no code column, no combined-validity column, and no wait — the
// slots come from n, since the survivor count is not known on the host.
extern "C" int dsx_hash_build_cols(DsxCtx* c, const DsxInstr* prog,
                                   int prog_len, const DsxColumn* cols,
                                   int ncols, const DsxKeySpec* keys,
                                   int nkeys, int64_t n, uint64_t code_max,
                                   int key_filter, DsxHashTable** out) {
  if (prog_len < 0 || prog_len > DSX_MAX_PROG || ncols > DSX_MAX_COLS ||
      nkeys < 1 || nkeys > DSX_MAX_KEYS)
    FAIL(-3, "build-from-columns spec too large");
  ProgArg P{};
  if (prog_len) memcpy(P.ins, prog, prog_len * sizeof(DsxInstr));
  P.len = prog_len;
  KeyArg K{};
  int rc = make_keyarg(keys, nkeys, K);
  if (rc) return rc;
  for (int j = 0; j < nkeys; j++)
    if (keys[j].mode != 0 || keys[j].col < 0 || keys[j].col >= ncols)
      FAIL(-3, "build-from-columns takes radix-packed integer keys only");
  for (int i = 0; i < prog_len; i++)
    if (prog[i].op == DSX_OP_COL && (prog[i].arg0 < 0 || prog[i].arg0 >= ncols))
      FAIL(-3, "predicate reads no source column");
  ColsArg C{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    if (cols[i].len < n) FAIL(-3, "source column shorter than n");
    C.data[i] = cols[i].data;
    C.validity[i] = cols[i].validity;
    C.dtype[i] = cols[i].dtype;
  }
  DsxHashTable* t = nullptr;
  rc = hash_table_new(c, n, code_max, key_filter != 0, &t);
  if (rc) return rc;
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  if (grid > 0) {
    bool lite = vm_prog_is_lite(prog, prog_len);
    bool comb = build_runcombine_enabled();
    auto kern = lite ? (comb ? k_hash_build_cols<true, true>
                             : k_hash_build_cols<true, false>)
                     : (comb ? k_hash_build_cols<false, true>
                             : k_hash_build_cols<false, false>);
    ProfScope ps(c, "k_hash_build");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK), 0, c->stream, P, K, C, n,
                       t->keys, t->vals, t->slots - 1, t->packed, t->dup,
                       t->filter, t->filter_mode, t->filter_arg);
  }
  HIP_TRY(hipGetLastError());
  *out = t;
  return 0;
}

extern "C" int dsx_hash_build(DsxCtx* c, const uint64_t* codes,
                              const uint8_t* validity, int64_t n,
                              uint64_t code_max, DsxHashTable** out) {
  return hash_build_impl(c, codes, validity, n, code_max, false, out);
}

// dsx_hash_build plus, with key_filter != 0, the key-membership filter that
// dsx_filter_probe_cols consults (no other probe reads it)
extern "C" int dsx_hash_build_filtered(DsxCtx* c, const uint64_t* codes,
                                       const uint8_t* validity, int64_t n,
                                       uint64_t code_max, int key_filter,
                                       DsxHashTable** out) {
  return hash_build_impl(c, codes, validity, n, code_max, key_filter != 0,
                         out);
}

// tables built through dsx_hash_build_filtered with key_filter != 0 on this
// context so far that got a filter of `mode` (0: asked for, none built)
extern "C" int64_t dsx_join_filter_builds(DsxCtx* c, int mode) {
  return mode >= 0 && mode < 3 ? c->join_filter_builds[mode] : 0;
}

extern "C" int dsx_hash_table_filter_mode(const DsxHashTable* t) {
  return t ? t->filter_mode : DSX_JF_NONE;
}

extern "C" int64_t dsx_hash_table_filter_bytes(const DsxHashTable* t) {
  return t ? t->filter_bytes : 0;
}

extern "C" void dsx_hash_table_free(DsxHashTable* t) {
  if (!t) return;
  if (t->ctx) {
    pool_release(t->ctx, t->keys);
    pool_release(t->ctx, t->vals);
    pool_release(t->ctx, t->matched);
    // with a filter, dup is the filter allocation's last word
    if (!t->filter) pool_release(t->ctx, t->dup);
    pool_release(t->ctx, t->filter);
  }
  delete t;
}

// Only a mark_matched probe writes the marks and only dsx_hash_unmatched
// reads them, so a build does not pay for them: the first of the two
// allocates the slots x 4 B and clears them (a pool buffer comes back dirty).
static int hash_table_ensure_matched(DsxCtx* c, DsxHashTable* t) {
  if (t->matched) return 0;
  int rc = pool_alloc(c, t->slots * 4, (void**)&t->matched);
  if (rc) {
    t->matched = nullptr;
    return rc;
  }
  HIP_TRY(hipMemsetAsync(t->matched, 0, t->slots * 4, c->stream));
  return 0;
}

// PASS=0: per-block match counts (LDS reduce — a single global counter
// would serialize at ~88 wave-atomics/µs, measured 19-67 ms at C3 scale).
// PASS=1: emit at block bases from the scanned counts + LDS bump.
// PASS 0 probes the table once per row and CACHES (first match slot, match
// count) so PASS 1 only re-walks the chain for multi-match rows — for
// PK-FK joins (the common case) the emit pass does zero table probes.
template <int PASS>
__global__ void k_hash_probe(const uint64_t* codes, const uint8_t* validity,
                             int64_t n, const uint64_t* tkeys,
                             const uint32_t* tvals, uint32_t* matched,
                             int64_t mask, int join_type, int packed,
                             int mark_matched, int64_t* block_counts,
                             uint32_t* cache_slot, uint32_t* cache_cnt,
                             uint32_t* out_p, uint32_t* out_b, int64_t total,
                             unsigned int* dbg) {
  __shared__ unsigned long long s_cnt;   // PASS0: block total; PASS1: bump
  if (threadIdx.x == 0)
    s_cnt = (PASS == 1) ? (unsigned long long)block_counts[blockIdx.x] : 0;
  __syncthreads();
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  unsigned long long local = 0;
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    bool key_valid = !(validity && !validity[r]);
    if (PASS == 0) {
      uint32_t nmatch = 0;
      uint32_t first_s = DSX_NULL_IDX;
      uint32_t first_b = DSX_NULL_IDX;
      if (key_valid) {
        uint64_t cde = codes[r];
        int64_t s = (int64_t)(mix64(cde) & mask);
        while (true) {
          uint64_t k = tkeys[s];
          if (k == EMPTY_KEY) break;
          uint64_t kc = packed ? (k >> 32) : k;
          if (kc == cde) {
            if (first_s == DSX_NULL_IDX) {
              first_s = (uint32_t)s;
              first_b = packed ? (uint32_t)k : tvals[s];
            }
            nmatch++;
            if (join_type == DSX_JOIN_LEFTSEMI ||
                join_type == DSX_JOIN_LEFTANTI)
              break;  // existence only
          }
          s = (s + 1) & mask;
        }
      }
      // single-match rows with no FULL-OUTER marking need only the build id
      // in the emit pass — cache it instead of the slot (zero table reads)
      cache_slot[r] = (nmatch == 1 && !mark_matched) ? first_b : first_s;
      cache_cnt[r] = nmatch;
      if (join_type == DSX_JOIN_INNER || join_type == DSX_JOIN_LEFT)
        local += (unsigned long long)nmatch;
      if (nmatch == 0 && (join_type == DSX_JOIN_LEFT ||
                          join_type == DSX_JOIN_LEFTANTI))
        local += 1;  // NULL-fill / anti row
      if (nmatch > 0 && join_type == DSX_JOIN_LEFTSEMI) local += 1;
    } else {  // PASS 1: emit from the cache
      uint32_t nmatch = cache_cnt[r];
      uint32_t first_s = cache_slot[r];
      if (nmatch > 0 &&
          (join_type == DSX_JOIN_INNER || join_type == DSX_JOIN_LEFT)) {
        unsigned long long o =
            atomicAdd(&s_cnt, (unsigned long long)nmatch);
        if (o + nmatch > (unsigned long long)total) {
          atomicOr(dbg, 2u);
        } else if (nmatch == 1) {
          out_p[o] = (uint32_t)r;
          if (mark_matched) {  // cache holds the SLOT in this mode
            uint64_t k = tkeys[first_s];
            out_b[o] = packed ? (uint32_t)k : tvals[first_s];
            matched[first_s] = 1;  // FULL OUTER sweep only
          } else {             // cache holds the BUILD ID directly
            out_b[o] = first_s;
          }
        } else {
          // multi-match: walk the chain from the first cached slot
          uint64_t cde = codes[r];
          int64_t s = (int64_t)first_s;
          uint32_t emitted = 0;
          while (emitted < nmatch) {
            uint64_t k = tkeys[s];
            uint64_t kc = packed ? (k >> 32) : k;
            if (k == EMPTY_KEY) break;  // cannot happen if cache consistent
            if (kc == cde) {
              out_p[o + emitted] = (uint32_t)r;
              out_b[o + emitted] = packed ? (uint32_t)k : tvals[s];
              if (mark_matched) matched[s] = 1;
              emitted++;
            }
            s = (s + 1) & mask;
          }
        }
      } else if (nmatch == 0 && (join_type == DSX_JOIN_LEFT ||
                                 join_type == DSX_JOIN_LEFTANTI)) {
        unsigned long long o = atomicAdd(&s_cnt, 1ull);
        if (o >= (unsigned long long)total) atomicOr(dbg, 2u);
        else {
          out_p[o] = (uint32_t)r;
          out_b[o] = DSX_NULL_IDX;
        }
      } else if (nmatch > 0 && join_type == DSX_JOIN_LEFTSEMI) {
        unsigned long long o = atomicAdd(&s_cnt, 1ull);
        if (o >= (unsigned long long)total) atomicOr(dbg, 2u);
        else {
          out_p[o] = (uint32_t)r;
          out_b[o] = first_s;  // SEMI: nmatch==1 ⇒ cache holds the build id
        }
      }
    }
  }
  if (PASS == 0) {
    for (int d = 32; d > 0; d >>= 1) local += __shfl_down(local, d, 64);
    if ((threadIdx.x & 63) == 0 && local)
      atomicAdd(&s_cnt, local);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = (int64_t)s_cnt;
  }
}

extern "C" int dsx_hash_probe(DsxCtx* c, DsxHashTable* t, const uint64_t* codes,
                              const uint8_t* validity, int64_t n, int join_type,
                              int mark_matched,
                              uint32_t** out_probe_idx, uint32_t** out_build_idx,
                              int64_t* out_count) {
  if (n > 0xFFFFFFFEll) FAIL(-3, "probe side too large for u32 row ids");
  *out_probe_idx = nullptr;
  *out_build_idx = nullptr;
  *out_count = 0;
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  int rc = ensure_scratch(c, (grid + 2) * 8 + n * 8 + 64);
  if (rc) return rc;
  if (mark_matched) {
    rc = hash_table_ensure_matched(c, t);
    if (rc) return rc;
  }
  int64_t* block_counts = (int64_t*)c->scratch;
  int64_t* d_total = block_counts + grid;
  uint32_t* cache_slot = (uint32_t*)(d_total + 2);
  uint32_t* cache_cnt = cache_slot + n;
  if (grid > 0) {
    ProfScope ps(c, "k_hash_probe_count");
    hipLaunchKernelGGL(k_hash_probe<0>, dim3(grid), dim3(BLOCK), 0, c->stream,
                       codes, validity, n, t->keys, t->vals, t->matched,
                       t->slots - 1, join_type, t->packed, mark_matched,
                       block_counts, cache_slot, cache_cnt, nullptr, nullptr,
                       0, c->dbg_flag);
  }
  hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream,
                     block_counts, grid, d_total);
  int64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  { int rc2 = pool_alloc(c, (total > 0 ? total : 1) * 4, (void**)out_probe_idx); if (rc2) return rc2; }
  { int rc2 = pool_alloc(c, (total > 0 ? total : 1) * 4, (void**)out_build_idx); if (rc2) return rc2; }
  if (grid > 0 && total > 0) {
    ProfScope ps(c, "k_hash_probe_emit");
    hipLaunchKernelGGL(k_hash_probe<1>, dim3(grid), dim3(BLOCK), 0, c->stream,
                       codes, validity, n, t->keys, t->vals, t->matched,
                       t->slots - 1, join_type, t->packed, mark_matched,
                       block_counts, cache_slot, cache_cnt, *out_probe_idx,
                       *out_build_idx, total, c->dbg_flag);
  }
  HIP_TRY(hipGetLastError());
  *out_count = total;
  return dbg_check(c, "dsx_hash_probe");
}

// ---------------------------------------------------------------------------
// fused probe-emit + materialization (INNER/LEFT/SEMI/ANTI, no residual):
// instead of (probe, build) pair vectors + one gather per output column,
// the emit pass writes the output columns directly — one pass, no pair
// traffic (join.py:241-246 dd.merge column copy, fused).
// ---------------------------------------------------------------------------
struct JoinMatArg {
  const void* src[16];
  const uint8_t* srcv[16];
  void* dst[16];
  uint8_t* dstv[16];
  int32_t dtype[16];
  int32_t side[16];  // 0 = probe row index, 1 = build row id
  int32_t ncols;
};

__device__ __forceinline__ void jm_write(const JoinMatArg& M, int64_t o,
                                         int64_t r, uint32_t bid) {
  for (int ci = 0; ci < M.ncols; ci++) {
    int64_t idx = M.side[ci] ? (int64_t)bid : r;
    bool missing = M.side[ci] && bid == DSX_NULL_IDX;  // LEFT NULL-fill
    switch (M.dtype[ci]) {
      case DSX_I64:
        ((int64_t*)M.dst[ci])[o] = missing ? 0 : ((const int64_t*)M.src[ci])[idx];
        break;
      case DSX_F64:
        ((double*)M.dst[ci])[o] =
            missing ? __builtin_nan("") : ((const double*)M.src[ci])[idx];
        break;
      case DSX_I32:
        ((int32_t*)M.dst[ci])[o] = missing ? 0 : ((const int32_t*)M.src[ci])[idx];
        break;
      case DSX_F32:
        ((float*)M.dst[ci])[o] =
            missing ? __builtin_nanf("") : ((const float*)M.src[ci])[idx];
        break;
      default:  // I8 / BOOL8
        ((int8_t*)M.dst[ci])[o] = missing ? 0 : ((const int8_t*)M.src[ci])[idx];
    }
    if (M.dstv[ci])
      M.dstv[ci][o] = missing ? 0 : (M.srcv[ci] ? M.srcv[ci][idx] : 1);
  }
}

__global__ void k_hash_probe_mat(const uint64_t* codes,
                                 const uint8_t* validity, int64_t n,
                                 const uint64_t* tkeys, const uint32_t* tvals,
                                 int64_t mask, int join_type, int packed,
                                 const int64_t* block_counts,
                                 const uint32_t* cache_slot,
                                 const uint32_t* cache_cnt,
                                 const JoinMatArg* Mp, int64_t total,
                                 unsigned int* dbg) {
  __shared__ unsigned long long s_cnt;
  // LDS copy: through the global pointer the compiler must assume the
  // output writes alias the arg block and re-loads every pointer per
  // write; staged in LDS they load once (measured 4×)
  __shared__ JoinMatArg s_M;
  if (threadIdx.x == 0) {
    s_cnt = (unsigned long long)block_counts[blockIdx.x];
    s_M = *Mp;
  }
  __syncthreads();
  const JoinMatArg& M = s_M;
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    uint32_t nmatch = cache_cnt[r];
    uint32_t first_s = cache_slot[r];
    if (nmatch > 0 &&
        (join_type == DSX_JOIN_INNER || join_type == DSX_JOIN_LEFT)) {
      unsigned long long o = atomicAdd(&s_cnt, (unsigned long long)nmatch);
      if (o + nmatch > (unsigned long long)total) {
        atomicOr(dbg, 2u);
      } else if (nmatch == 1) {
        jm_write(M, (int64_t)o, r, first_s);  // cache holds the build id
      } else {
        uint64_t cde = codes[r];
        int64_t s = (int64_t)first_s;
        uint32_t emitted = 0;
        while (emitted < nmatch) {
          uint64_t k = tkeys[s];
          uint64_t kc = packed ? (k >> 32) : k;
          if (k == EMPTY_KEY) break;
          if (kc == cde) {
            jm_write(M, (int64_t)(o + emitted), r,
                     packed ? (uint32_t)k : tvals[s]);
            emitted++;
          }
          s = (s + 1) & mask;
        }
      }
    } else if (nmatch == 0 && (join_type == DSX_JOIN_LEFT ||
                               join_type == DSX_JOIN_LEFTANTI)) {
      unsigned long long o = atomicAdd(&s_cnt, 1ull);
      if (o >= (unsigned long long)total) atomicOr(dbg, 2u);
      else jm_write(M, (int64_t)o, r, DSX_NULL_IDX);
    } else if (nmatch > 0 && join_type == DSX_JOIN_LEFTSEMI) {
      unsigned long long o = atomicAdd(&s_cnt, 1ull);
      if (o >= (unsigned long long)total) atomicOr(dbg, 2u);
      else jm_write(M, (int64_t)o, r, first_s);
    }
  }
}

__global__ void k_hash_probe_mat_1pass(
    const uint64_t* codes, const uint8_t* validity, int64_t n,
    const uint64_t* tkeys, const uint32_t* tvals, int64_t mask, int packed,
    const JoinMatArg* Mp, unsigned long long* counter) {
  // unique build keys + INNER: probe and emit in ONE pass — no count
  // pass, no slot caches. Wave-ballot compaction gives dense, coalesced
  // writes; output order is nondeterministic across blocks (SQL imposes
  // none; the pair path stays available under DSX_DISABLE_1PASS).
  __shared__ JoinMatArg s_M;
  __shared__ int s_wave[BLOCK / 64 + 1];
  __shared__ unsigned long long s_base;
  if (threadIdx.x == 0) s_M = *Mp;
  __syncthreads();
  const JoinMatArg& M = s_M;
  int lane = threadIdx.x & 63;
  int wid = threadIdx.x >> 6;
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  for (int64_t base = lo; base < hi; base += BLOCK) {
    int64_t r = base + threadIdx.x;
    bool found = false;
    uint32_t bid = 0;
    if (r < hi && !(validity && !validity[r])) {
      uint64_t cde = codes[r];
      int64_t s = (int64_t)(mix64(cde) & mask);
      while (true) {
        uint64_t k = tkeys[s];
        if (k == EMPTY_KEY) break;
        if ((packed ? (k >> 32) : k) == cde) {
          found = true;
          bid = packed ? (uint32_t)k : tvals[s];
          break;
        }
        s = (s + 1) & mask;
      }
    }
    uint64_t ball = __ballot(found);
    if (lane == 0) s_wave[wid] = __popcll(ball);
    __syncthreads();
    if (threadIdx.x == 0) {
      int run = 0;
      for (int i = 0; i < BLOCK / 64; i++) {
        int v = s_wave[i];
        s_wave[i] = run;
        run += v;
      }
      s_base = run ? atomicAdd(counter, (unsigned long long)run) : 0;
    }
    __syncthreads();
    if (found) {
      int64_t o = (int64_t)(s_base + s_wave[wid] +
                            __popcll(ball & ((1ull << lane) - 1)));
      jm_write(M, o, r, bid);
    }
    __syncthreads();
  }
}

extern "C" int dsx_hash_probe_cols(
    DsxCtx* c, DsxHashTable* t, const uint64_t* codes,
    const uint8_t* validity, int64_t n, int join_type,
    const DsxColumn* pcols, int n_pcols, const DsxColumn* bcols, int n_bcols,
    int force_build_validity, void** out_datas, uint8_t** out_valids,
    int64_t* out_count) {
  if (n > 0xFFFFFFFEll) FAIL(-3, "probe side too large for u32 row ids");
  int ncols = n_pcols + n_bcols;
  if (ncols > 16) FAIL(-3, "too many join output columns for fused emit");
  *out_count = 0;
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  int64_t arg_off = (grid + 2) * 8 + n * 8 + 64;
  int rc = ensure_scratch(c, arg_off + (int64_t)sizeof(JoinMatArg) + 64);
  if (rc) return rc;
  int64_t* block_counts = (int64_t*)c->scratch;
  int64_t* d_total = block_counts + grid;
  uint32_t* cache_slot = (uint32_t*)(d_total + 2);
  uint32_t* cache_cnt = cache_slot + n;
  JoinMatArg* d_M = (JoinMatArg*)((char*)c->scratch + ((arg_off + 63) / 64) * 64);
  // unique build keys + INNER → single-pass probe+emit (no count pass).
  // MEASURED SLOWER than the 2-pass fused path (C3 5.59 vs 5.29 ms of
  // kernel time; Q3 1.04 vs 0.59): the chunk-synchronous ballot emission
  // stalls every 256 rows on the slowest probe chain, losing the
  // memory-level parallelism of free-running probes. Kept opt-in as the
  // recorded experiment.
  static const bool use_1pass = getenv("DSX_ENABLE_1PASS") != nullptr;
  unsigned int h_dup = 1;
  if (use_1pass && join_type == DSX_JOIN_INNER) {
    HIP_TRY(hipMemcpyAsync(&h_dup, t->dup, 4, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  if (use_1pass && join_type == DSX_JOIN_INNER && h_dup == 0) {
    JoinMatArg M{};
    M.ncols = ncols;
    for (int i = 0; i < ncols; i++) {
      const DsxColumn* src = i < n_pcols ? &pcols[i] : &bcols[i - n_pcols];
      int side = i < n_pcols ? 0 : 1;
      int esz = src->dtype == DSX_I64 || src->dtype == DSX_F64 ? 8
                : src->dtype == DSX_I32 || src->dtype == DSX_F32 ? 4 : 1;
      int rc2 = pool_alloc(c, (n > 0 ? n : 1) * esz, &out_datas[i]);
      if (rc2) return rc2;
      out_valids[i] = nullptr;
      if (src->validity) {
        void* vp = nullptr;
        rc2 = pool_alloc(c, n > 0 ? n : 1, &vp);
        if (rc2) return rc2;
        out_valids[i] = (uint8_t*)vp;
      }
      M.src[i] = src->data;
      M.srcv[i] = src->validity;
      M.dst[i] = out_datas[i];
      M.dstv[i] = out_valids[i];
      M.dtype[i] = src->dtype;
      M.side[i] = side;
    }
    HIP_TRY(hipMemcpyAsync(d_M, &M, sizeof(JoinMatArg),
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_total, 0, 8, c->stream));
    if (grid > 0) {
      ProfScope ps(c, "k_hash_probe_mat");
      hipLaunchKernelGGL(k_hash_probe_mat_1pass, dim3(grid), dim3(BLOCK), 0,
                         c->stream, codes, validity, n, t->keys, t->vals,
                         t->slots - 1, t->packed, d_M,
                         (unsigned long long*)d_total);
    }
    unsigned long long tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, d_total, 8, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    *out_count = (int64_t)tot;
    return dbg_check(c, "dsx_hash_probe_cols");
  }
  if (grid > 0) {
    ProfScope ps(c, "k_hash_probe_count");
    hipLaunchKernelGGL(k_hash_probe<0>, dim3(grid), dim3(BLOCK), 0, c->stream,
                       codes, validity, n, t->keys, t->vals, t->matched,
                       t->slots - 1, join_type, t->packed, 0,
                       block_counts, cache_slot, cache_cnt, nullptr, nullptr,
                       0, c->dbg_flag);
  }
  hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream,
                     block_counts, grid, d_total);
  int64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  JoinMatArg M{};
  M.ncols = ncols;
  int64_t tsz = total > 0 ? total : 1;
  for (int i = 0; i < ncols; i++) {
    const DsxColumn* src = i < n_pcols ? &pcols[i] : &bcols[i - n_pcols];
    int side = i < n_pcols ? 0 : 1;
    int esz = src->dtype == DSX_I64 || src->dtype == DSX_F64 ? 8
              : src->dtype == DSX_I32 || src->dtype == DSX_F32 ? 4 : 1;
    int rc2 = pool_alloc(c, tsz * esz, &out_datas[i]);
    if (rc2) return rc2;
    bool want_valid = src->validity != nullptr ||
                      (side == 1 && force_build_validity);
    out_valids[i] = nullptr;
    if (want_valid) {
      void* vp = nullptr;
      rc2 = pool_alloc(c, tsz, &vp);
      if (rc2) return rc2;
      out_valids[i] = (uint8_t*)vp;
    }
    M.src[i] = src->data;
    M.srcv[i] = src->validity;
    M.dst[i] = out_datas[i];
    M.dstv[i] = out_valids[i];
    M.dtype[i] = src->dtype;
    M.side[i] = side;
  }
  HIP_TRY(hipMemcpyAsync(d_M, &M, sizeof(JoinMatArg), hipMemcpyHostToDevice,
                         c->stream));
  if (grid > 0 && total > 0) {
    ProfScope ps(c, "k_hash_probe_mat");
    hipLaunchKernelGGL(k_hash_probe_mat, dim3(grid), dim3(BLOCK), 0,
                       c->stream, codes, validity, n, t->keys, t->vals,
                       t->slots - 1, join_type, t->packed, block_counts,
                       cache_slot, cache_cnt, d_M, total, c->dbg_flag);
  }
  HIP_TRY(hipGetLastError());
  *out_count = total;
  return dbg_check(c, "dsx_hash_probe_cols");
}

// ---------------------------------------------------------------------------
// dsx_filter_probe_cols — scan filter + key pack + PK-FK probe in one sweep
// over the UNFILTERED probe columns (INNER, unique build keys). Replaces
// dsx_filter_cols → dsx_keypack → dsx_hash_probe_cols and their three
// intermediates (compacted columns, code column, slot/count cache) with a
// one-bit-per-row match mask.
// ---------------------------------------------------------------------------
// first match of `cde` (build keys are unique on this path)
__device__ __forceinline__ bool fp_probe(const uint64_t* tkeys,
                                         const uint32_t* tvals, int64_t mask,
                                         int packed, uint64_t cde,
                                         uint32_t& bid) {
  int64_t s = (int64_t)(mix64(cde) & mask);
  while (true) {
    uint64_t k = tkeys[s];
    if (k == EMPTY_KEY) return false;
    if ((packed ? (k >> 32) : k) == cde) {
      bid = packed ? (uint32_t)k : tvals[s];
      return true;
    }
    s = (s + 1) & mask;
  }
}

// pass 1: predicate → key validity → pack → probe → ballot. Same word
// ownership as k_filter_mask (and the same round-up for idle blocks); waves
// run free, no barrier in the row loop. extra[0] receives the table's dup
// flag so the host fetches it with the total in one copy.
template <bool LITE>
__global__ void k_fprobe_mask(ProgArg prog, KeyArg K, ColsArg C, int64_t n,
                              const uint64_t* tkeys, const uint32_t* tvals,
                              int64_t tmask, int packed,
                              const unsigned int* dup, uint64_t* mask,
                              int64_t* block_counts, int64_t* extra,
                              const uint32_t* jf, int jf_mode,
                              uint64_t jf_arg) {
  int64_t lo, hi;
  block_range(n, 64, lo, hi);
  __shared__ int64_t s_count;
  if (threadIdx.x == 0) {
    s_count = 0;
    if (blockIdx.x == 0) extra[0] = (int64_t)*dup;
  }
  __syncthreads();
  int lane = threadIdx.x & 63;
  int64_t local = 0;
  for (int64_t w = (lo + 63) / 64 + threadIdx.x / 64; w * 64 < hi;
       w += WAVES_PER_BLOCK) {
    int64_t r = w * 64 + lane;
    bool hit = false;
    if (r < n) {
      Slot v;
      bool valid = vm_eval<LITE>(prog.ins, prog.len, C, r, v);
      if (valid && v.i != 0 && fp_key_valid(K, C, r)) {  // NULL → False
        // the code of a row with a NULL key is garbage and never gets here
        uint64_t cde = pack_key(K, C, r);
        if (jf_mode == DSX_JF_EXACT) {  // bit set <=> build key: no table
          hit = cde <= jf_arg &&
                (jf[dsx_jf_exact_word(cde)] & dsx_jf_exact_bit(cde)) != 0;
        } else {
          bool pass = true;
          if (jf_mode == DSX_JF_HASHED) {
            uint64_t h = dsx_jf_mix64(cde);
            uint32_t bits = dsx_jf_hashed_bits(h);
            pass = (jf[dsx_jf_hashed_word(h, jf_arg)] & bits) == bits;
          }
          uint32_t bid;
          if (pass) hit = fp_probe(tkeys, tvals, tmask, packed, cde, bid);
        }
      }
    }
    uint64_t m = __ballot(hit);
    if (lane == 0) {
      mask[w] = m;
      local += __popcll(m);
    }
  }
  if (lane == 0) atomicAdd((unsigned long long*)&s_count, (unsigned long long)local);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s_count;
}

// fp_select_bit, fp_wave_inclusive, fp_batch_row: the set bits of a batch of
// mask words handed to the lanes of a wave
#include "fprobe_lanes.h"

// pass 2: each wave takes a CONTIGUOUS quarter of the block's mask words.
// Up front the waves count their quarters and exchange the four totals
// through LDS (the only barrier); after that a wave scans 64 words at a time
// with shuffles and hands the j-th matched row of the batch to lane j, so
// lanes stay dense at any match density, output slots are consecutive across
// the wave (coalesced stores) and rows come out in increasing probe order.
// Only matched rows re-pack and re-probe to recover the build row id.
__global__ void k_fprobe_emit(KeyArg K, ColsArg C, int64_t n,
                              const uint64_t* tkeys, const uint32_t* tvals,
                              int64_t tmask, int packed, const uint64_t* mask,
                              const int64_t* block_offsets,
                              const JoinMatArg* Mp, int64_t total,
                              int need_bid, unsigned int* dbg) {
  __shared__ JoinMatArg s_M;  // LDS copy (see k_hash_probe_mat note)
  __shared__ int64_t s_tot[WAVES_PER_BLOCK];
  int64_t lo, hi;
  block_range(n, 64, lo, hi);
  int lane = threadIdx.x & 63;
  int wid = threadIdx.x >> 6;
  int64_t w0 = (lo + 63) / 64, w1 = (hi + 63) / 64;  // lo == hi ⇒ no words
  int64_t q = (w1 - w0 + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  int64_t c0 = min(w1, w0 + wid * q), c1 = min(w1, c0 + q);
  int64_t mine = 0;
  for (int64_t w = c0 + lane; w < c1; w += 64) mine += __popcll(mask[w]);
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
  if (lane == 0) s_tot[wid] = mine;
  if (threadIdx.x == 0) s_M = *Mp;
  __syncthreads();
  const JoinMatArg& M = s_M;
  int64_t base = block_offsets[blockIdx.x];
  for (int i = 0; i < wid; i++) base += s_tot[i];
  for (int64_t wb = c0; wb < c1; wb += 64) {
    uint64_t m = (wb + lane < c1) ? mask[wb + lane] : 0;
    int cnt = __popcll(m);
    int inc = fp_wave_inclusive(cnt);  // of the batch's word counts
    int T = __shfl(inc, 63, 64);
    for (int j0 = 0; j0 < T; j0 += 64) {
      // lanes past the batch total search for its last row and then sit out
      int j = min(j0 + lane, T - 1);
      int64_t r = fp_batch_row(m, inc, cnt, wb, j);
      if (j0 + lane < T) {
        int64_t o = base + j;
        uint32_t bid = DSX_NULL_IDX;
        // a call that materializes no build-side column needs no build row
        // id: the mask bit already says that the row matched
        bool hit = r < n && (!need_bid ||
                             fp_probe(tkeys, tvals, tmask, packed,
                                      pack_key(K, C, r), bid));
        if (!hit || o >= total) atomicOr(dbg, 2u);
        else jm_write(M, o, r, bid);
      }
    }
    base += T;
  }
}

// the per-shape generated form of k_fprobe_mask (jit_kernels.inc)
static hipFunction_t fprobe_mask_jit_fn(DsxCtx* c, const ProgArg& P,
                                        const KeyArg& K, const ColsArg& C,
                                        int packed, int jf_mode);
static void fprobe_mask_jit_launch(DsxCtx* c, hipFunction_t f, int grid,
                                   const ColsArg& C, int64_t n,
                                   const uint64_t* tkeys, int64_t tmask,
                                   const unsigned int* dup, uint64_t* mask,
                                   int64_t* block_counts, int64_t* extra,
                                   const uint32_t* jf, uint64_t jf_arg);

extern "C" int64_t dsx_fprobe_jit_launches(DsxCtx* c) {
  return c->fprobe_jit_launches;
}

// the mask pass of dsx_filter_probe_cols and dsx_filter_probe_groupby:
// generated kernel first; the interpreter is the fallback (JIT off,
// DSX_DISABLE_JIT_FPROBE=1, predicate rejected, hipRTC failure).
// DSX_DISABLE_JOINFILTER=1 (read per call) also ignores a filter the table
// already has. extra[0] receives the table's dup flag.
static void fprobe_mask_pass(DsxCtx* c, DsxHashTable* t, const DsxInstr* prog,
                             int prog_len, const ProgArg& P, const KeyArg& K,
                             const ColsArg& C, int64_t n, int grid,
                             uint64_t* mask, int64_t* block_counts,
                             int64_t* extra) {
  int jf_mode = join_filter_enabled() ? t->filter_mode : DSX_JF_NONE;
  hipFunction_t fj = fprobe_mask_jit_fn(c, P, K, C, t->packed, jf_mode);
  ProfScope ps(c, "k_fprobe_mask");
  if (fj) {
    fprobe_mask_jit_launch(c, fj, grid, C, n, t->keys, t->slots - 1, t->dup,
                           mask, block_counts, extra, t->filter,
                           t->filter_arg);
  } else {
    auto kern = vm_prog_is_lite(prog, prog_len) ? k_fprobe_mask<true>
                                                : k_fprobe_mask<false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK), 0, c->stream, P, K, C, n,
                       t->keys, t->vals, t->slots - 1, t->packed, t->dup, mask,
                       block_counts, extra, t->filter, jf_mode, t->filter_arg);
  }
}

extern "C" int dsx_filter_probe_cols(
    DsxCtx* c, DsxHashTable* t, const DsxInstr* prog, int prog_len,
    const DsxColumn* cols, int ncols, const DsxKeySpec* keys, int nkeys,
    int64_t n, const DsxColumn* pcols, int n_pcols, const DsxColumn* bcols,
    int n_bcols, void** out_datas, uint8_t** out_valids, int64_t* out_count) {
  if (prog_len > DSX_MAX_PROG || ncols > DSX_MAX_COLS || nkeys > DSX_MAX_KEYS)
    FAIL(-3, "filter-probe spec too large");
  int nmats = n_pcols + n_bcols;
  if (nmats > 16) FAIL(-3, "too many join output columns for fused emit");
  *out_count = 0;
  ProgArg P{};
  memcpy(P.ins, prog, prog_len * sizeof(DsxInstr));
  P.len = prog_len;
  KeyArg K{};
  int rc = make_keyarg(keys, nkeys, K);
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
  int64_t nwords = (n + 63) / 64;
  int grid = (int)min((int64_t)MAX_GRID, (nwords + WAVES_PER_BLOCK - 1) /
                                             WAVES_PER_BLOCK);
  int64_t arg_off = nwords * 8 + (grid + 2) * 8 + 64;
  rc = ensure_scratch(c, arg_off + (int64_t)sizeof(JoinMatArg) + 64);
  if (rc) return rc;
  uint64_t* mask = (uint64_t*)c->scratch;
  int64_t* block_counts = (int64_t*)(mask + nwords);
  int64_t* d_total = block_counts + grid;  // [0] total, [1] dup flag
  JoinMatArg* d_M =
      (JoinMatArg*)((char*)c->scratch + ((arg_off + 63) / 64) * 64);
  int64_t h_res[2] = {0, 0};
  if (grid > 0) {
    fprobe_mask_pass(c, t, prog, prog_len, P, K, C, n, grid, mask,
                     block_counts, d_total + 1);
    hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream,
                       block_counts, grid, d_total);
    HIP_TRY(hipMemcpyAsync(h_res, d_total, 16, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // duplicate build keys: one match bit per row is not enough
    if (h_res[1] != 0) return DSX_NOT_APPLICABLE;
  }
  int64_t total = h_res[0];
  JoinMatArg M{};
  M.ncols = nmats;
  int64_t tsz = total > 0 ? total : 1;
  for (int i = 0; i < nmats; i++) {
    const DsxColumn* src = i < n_pcols ? &pcols[i] : &bcols[i - n_pcols];
    int esz = src->dtype == DSX_I64 || src->dtype == DSX_F64 ? 8
              : src->dtype == DSX_I32 || src->dtype == DSX_F32 ? 4 : 1;
    int rc2 = pool_alloc(c, tsz * esz, &out_datas[i]);
    if (rc2) return rc2;
    out_valids[i] = nullptr;
    if (src->validity) {
      void* vp = nullptr;
      rc2 = pool_alloc(c, tsz, &vp);
      if (rc2) return rc2;
      out_valids[i] = (uint8_t*)vp;
    }
    M.src[i] = src->data;
    M.srcv[i] = src->validity;
    M.dst[i] = out_datas[i];
    M.dstv[i] = out_valids[i];
    M.dtype[i] = src->dtype;
    M.side[i] = i < n_pcols ? 0 : 1;
  }
  if (grid > 0 && total > 0) {
    HIP_TRY(hipMemcpyAsync(d_M, &M, sizeof(JoinMatArg), hipMemcpyHostToDevice,
                           c->stream));
    ProfScope ps(c, "k_fprobe_emit");
    hipLaunchKernelGGL(k_fprobe_emit, dim3(grid), dim3(BLOCK), 0, c->stream,
                       K, C, n, t->keys, t->vals, t->slots - 1, t->packed,
                       mask, block_counts, d_M, total, n_bcols > 0 ? 1 : 0,
                       c->dbg_flag);
  }
  HIP_TRY(hipGetLastError());
  *out_count = total;
  return dbg_check(c, "dsx_filter_probe_cols");
}

template <int PASS>
__global__ void k_unmatched(const uint64_t* tkeys, const uint32_t* tvals,
                            const uint32_t* matched, int64_t slots,
                            int packed, unsigned long long* counter,
                            uint32_t* out_b) {
  int64_t lo, hi;
  block_range(slots, 1, lo, hi);
  for (int64_t s = lo + threadIdx.x; s < hi; s += BLOCK) {
    if (tkeys[s] != EMPTY_KEY && !matched[s]) {
      unsigned long long o = atomicAdd(counter, 1ull);
      if (PASS == 1)
        out_b[o] = packed ? (uint32_t)tkeys[s] : tvals[s];
    }
  }
}

extern "C" int dsx_hash_unmatched(DsxCtx* c, DsxHashTable* t,
                                  uint32_t** out_build_idx, int64_t* out_count) {
  *out_build_idx = nullptr;
  *out_count = 0;
  int rc = ensure_scratch(c, 8);
  if (rc) return rc;
  // a table no mark_matched probe has touched: all marks 0, every build row
  rc = hash_table_ensure_matched(c, t);
  if (rc) return rc;
  unsigned long long* counter = (unsigned long long*)c->scratch;
  HIP_TRY(hipMemsetAsync(counter, 0, 8, c->stream));
  int grid = (int)min((int64_t)MAX_GRID, (t->slots + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(k_unmatched<0>, dim3(grid), dim3(BLOCK), 0, c->stream,
                     t->keys, t->vals, t->matched, t->slots, t->packed,
                     counter, nullptr);
  unsigned long long total = 0;
  HIP_TRY(hipMemcpyAsync(&total, counter, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  { int rc2 = pool_alloc(c, (total > 0 ? total : 1) * 4, (void**)out_build_idx); if (rc2) return rc2; }
  HIP_TRY(hipMemsetAsync(counter, 0, 8, c->stream));
  if (total > 0)
    hipLaunchKernelGGL(k_unmatched<1>, dim3(grid), dim3(BLOCK), 0, c->stream,
                       t->keys, t->vals, t->matched, t->slots, t->packed,
                       counter, *out_build_idx);
  HIP_TRY(hipGetLastError());
  *out_count = (int64_t)total;
  return 0;
}

// ---------------------------------------------------------------------------
// hash groupby-aggregate (aggregate.py:575-581 + fused filter)
// two-level: LDS direct-indexed accumulation for small key spaces, global
// CAS-claim table otherwise.
// ---------------------------------------------------------------------------
struct AggArg {
  int32_t op[DSX_MAX_AGGS];
  int32_t never_null[DSX_MAX_AGGS];  // input prog cannot yield NULL: the
                                     // per-agg non-null count equals the
                                     // group row count → skip its atomic
  int32_t naggs;
};

// order-preserving transform for f64 atomic min/max on u64 bits
__device__ __forceinline__ uint64_t f64_ordered(double d) {
  uint64_t b = __double_as_longlong(d);
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double f64_unordered(uint64_t b) {
  uint64_t raw = (b & 0x8000000000000000ull) ? (b & 0x7FFFFFFFFFFFFFFFull) : ~b;
  return __longlong_as_double(raw);
}
// i64 → order-preserving u64 (for atomicMin/Max on unsigned)
__device__ __forceinline__ uint64_t i64_ordered(int64_t v) {
  return (uint64_t)v ^ 0x8000000000000000ull;
}

// per-agg accumulator update into (vals u64-typed, cnts)
__device__ __forceinline__ void agg_update_global(int op, int never_null,
                                                  uint64_t* val,
                                                  unsigned long long* cnt,
                                                  Slot v, bool valid) {
  if (!valid) return;
  switch (op) {
    case DSX_AGG_SUM_F64:
      unsafeAtomicAdd((double*)val, v.f);
      break;
    case DSX_AGG_SUM_I64:
      atomicAdd((unsigned long long*)val, (unsigned long long)v.i);
      break;
    case DSX_AGG_COUNT:
      break;
    case DSX_AGG_MIN_F64:
      atomicMin((unsigned long long*)val,
                (unsigned long long)f64_ordered(v.f));
      break;
    case DSX_AGG_MAX_F64:
      atomicMax((unsigned long long*)val,
                (unsigned long long)f64_ordered(v.f));
      break;
    case DSX_AGG_MIN_I64:
      atomicMin((unsigned long long*)val,
                (unsigned long long)i64_ordered(v.i));
      break;
    case DSX_AGG_MAX_I64:
      atomicMax((unsigned long long*)val,
                (unsigned long long)i64_ordered(v.i));
      break;
  }
  if (!never_null) atomicAdd(cnt, 1ull);
}

__host__ __device__ __forceinline__ uint64_t agg_identity(int op) {
  switch (op) {
    case DSX_AGG_MIN_F64:
    case DSX_AGG_MIN_I64:
      return 0xFFFFFFFFFFFFFFFFull;  // ordered-max
    case DSX_AGG_MAX_F64:
    case DSX_AGG_MAX_I64:
      return 0;  // ordered-min
    default:
      return 0;  // sums
  }
}

#include "jit.inc"
#include "jit_kernels.inc"

// ---- LDS direct-index path -------------------------------------------------
// LDS layout: [key_space × naggs] u64 vals, [key_space × naggs] u32 cnts,
// [key_space] u32 gcnt. Host guarantees it fits (≤ LDS budget).
__global__ void __launch_bounds__(BLOCK)
k_groupby_direct(ColsArg C, int64_t n, const KeyArg* Kp,
                 int key_space, ProgArg pred, const DsxInstr* agg_progs,
                 const int32_t* agg_lens, const AggArg* Ap,
                 uint64_t* g_vals /*[naggs][key_space]*/,
                 unsigned long long* g_cnts /*[naggs][key_space]*/,
                 unsigned long long* g_gcnt /*[key_space]*/) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* s_vals = (uint64_t*)smem;                       // naggs*ks
  uint32_t* s_cnts = (uint32_t*)(s_vals + Ap->naggs * key_space);  // naggs*ks
  uint32_t* s_gcnt = (uint32_t*)(s_cnts + Ap->naggs * key_space); // ks
  for (int i = threadIdx.x; i < Ap->naggs * key_space; i += BLOCK) {
    s_vals[i] = agg_identity(Ap->op[i / key_space]);
    s_cnts[i] = 0;
  }
  for (int i = threadIdx.x; i < key_space; i += BLOCK) s_gcnt[i] = 0;
  __syncthreads();

  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    if (pred.len) {
      Slot pv;
      bool pvalid = vm_eval(pred.ins, pred.len, C, r, pv);
      if (!(pvalid && pv.i != 0)) continue;  // NULL→False (filter.py:39)
    }
    int k = (int)pack_key(*Kp, C, r);
    atomicAdd(&s_gcnt[k], 1u);
    const DsxInstr* p = agg_progs;
    for (int a = 0; a < Ap->naggs; a++) {
      Slot v;
      bool valid = vm_eval(p, agg_lens[a], C, r, v);
      p += DSX_MAX_PROG;
      if (!valid) continue;
      int idx = a * key_space + k;
      switch (Ap->op[a]) {
        case DSX_AGG_SUM_F64:
          unsafeAtomicAdd((double*)&s_vals[idx], v.f);
          break;
        case DSX_AGG_SUM_I64:
          atomicAdd((unsigned long long*)&s_vals[idx],
                    (unsigned long long)v.i);
          break;
        case DSX_AGG_COUNT:
          break;
        case DSX_AGG_MIN_F64:
          atomicMin((unsigned long long*)&s_vals[idx],
                    (unsigned long long)f64_ordered(v.f));
          break;
        case DSX_AGG_MAX_F64:
          atomicMax((unsigned long long*)&s_vals[idx],
                    (unsigned long long)f64_ordered(v.f));
          break;
        case DSX_AGG_MIN_I64:
          atomicMin((unsigned long long*)&s_vals[idx],
                    (unsigned long long)i64_ordered(v.i));
          break;
        case DSX_AGG_MAX_I64:
          atomicMax((unsigned long long*)&s_vals[idx],
                    (unsigned long long)i64_ordered(v.i));
          break;
      }
      if (!Ap->never_null[a]) atomicAdd(&s_cnts[idx], 1u);
    }
  }
  __syncthreads();
  // merge block partials into global direct arrays
  for (int i = threadIdx.x; i < key_space; i += BLOCK) {
    if (s_gcnt[i])
      atomicAdd(&g_gcnt[i], (unsigned long long)s_gcnt[i]);
  }
  for (int i = threadIdx.x; i < Ap->naggs * key_space; i += BLOCK) {
    int a = i / key_space;
    int k = i - a * key_space;
    if (Ap->never_null[a] ? (s_gcnt[k] == 0) : (s_cnts[i] == 0)) continue;
    switch (Ap->op[a]) {
      case DSX_AGG_SUM_F64:
        unsafeAtomicAdd((double*)&g_vals[i],
                        __longlong_as_double((long long)s_vals[i]));
        break;
      case DSX_AGG_SUM_I64:
        atomicAdd((unsigned long long*)&g_vals[i],
                  (unsigned long long)s_vals[i]);
        break;
      case DSX_AGG_COUNT:
        break;
      case DSX_AGG_MIN_F64:
      case DSX_AGG_MIN_I64:
        atomicMin((unsigned long long*)&g_vals[i],
                  (unsigned long long)s_vals[i]);
        break;
      case DSX_AGG_MAX_F64:
      case DSX_AGG_MAX_I64:
        atomicMax((unsigned long long*)&g_vals[i],
                  (unsigned long long)s_vals[i]);
        break;
    }
    atomicAdd(&g_cnts[i], (unsigned long long)s_cnts[i]);
  }
}

// ---- global CAS-claim path --------------------------------------------------
__global__ void k_groupby_global(ColsArg C, int64_t n, const KeyArg* Kp,
                                 ProgArg pred, const DsxInstr* agg_progs,
                                 const int32_t* agg_lens, const AggArg* Ap,
                                 uint64_t* tkeys, int64_t mask,
                                 uint64_t* g_vals /*[naggs][slots]*/,
                                 unsigned long long* g_cnts,
                                 unsigned long long* g_gcnt,
                                 int* overflow) {
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  int64_t slots = mask + 1;
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    if (pred.len) {
      Slot pv;
      bool pvalid = vm_eval(pred.ins, pred.len, C, r, pv);
      if (!(pvalid && pv.i != 0)) continue;
    }
    uint64_t cde = pack_key(*Kp, C, r);
    int64_t s = (int64_t)(mix64(cde) & mask);
    int64_t probes = 0;
    while (true) {
      uint64_t k = tkeys[s];
      if (k == cde) break;
      if (k == EMPTY_KEY) {
        unsigned long long old = atomicCAS((unsigned long long*)&tkeys[s],
                                           EMPTY_KEY, (unsigned long long)cde);
        if (old == EMPTY_KEY || old == cde) break;
      }
      s = (s + 1) & mask;
      if (++probes > slots) {
        *overflow = 1;
        return;
      }
    }
    atomicAdd(&g_gcnt[s], 1ull);
    const DsxInstr* p = agg_progs;
    for (int a = 0; a < Ap->naggs; a++) {
      Slot v;
      bool valid = vm_eval(p, agg_lens[a], C, r, v);
      p += DSX_MAX_PROG;
      agg_update_global(Ap->op[a], Ap->never_null[a],
                        &g_vals[(int64_t)a * slots + s],
                        &g_cnts[(int64_t)a * slots + s], v, valid);
    }
  }
}


// ---------------------------------------------------------------------------
// partition-based groupby (the large-cardinality path):
// global atomics cap at ~23 RMW/ns on gfx950 (measured, probe_groupby.hip)
// while streaming runs at 6.3 TB/s — so instead of one CAS table we
//   (1) histogram rows into NB key-hash buckets per block (LDS counters),
//   (2) scan → deterministic per-(block,bucket) bases,
//   (3) scatter compact records (key + agg inputs, AoS) bucket-major —
//       block-contiguous runs merge in the XCD's L2 so the scattered writes
//       leave near-coalesced,
//   (4) one block per bucket aggregates its contiguous run in an LDS
//       open-addressing table (LDS atomics only), bump-appends compacted
//       groups,
//   (5) finalize into the [naggs][G] output slabs.
// Requires: all agg inputs never-null (the common case; else the CAS path).
// ---------------------------------------------------------------------------

__device__ __forceinline__ int gb_bucket(uint64_t code, int nb_mask) {
  return (int)((mix64(code ^ 0xC2B2AE3D27D4EB4Full) >> 32) & (uint64_t)nb_mask);
}

__global__ void k_gbpart_hist(ColsArg C, int64_t n, const KeyArg* Kp,
                              ProgArg pred, int nb,
                              int64_t* hist /*[grid][nb]*/) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* s_hist = (uint32_t*)smem;
  for (int i = threadIdx.x; i < nb; i += BLOCK) s_hist[i] = 0;
  __syncthreads();
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    if (pred.len) {
      Slot pv;
      bool pvalid = vm_eval(pred.ins, pred.len, C, r, pv);
      if (!(pvalid && pv.i != 0)) continue;
    }
    uint64_t code = pack_key(*Kp, C, r);
    atomicAdd(&s_hist[gb_bucket(code, nb - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += BLOCK)
    hist[(int64_t)blockIdx.x * nb + i] = (int64_t)s_hist[i];
}

// 8 buckets per block, transposed: lanes j=0..7 of one chunk read
// hist[g][8b..8b+7] — a full 64-B line — instead of the one-bucket-per-block
// version's 8-B strided walk (which the PMC counters showed fetching 143 MB
// per launch, 8.5× the algorithmic bytes). Exclusive scan over the grid
// dimension per bucket; bases written back in place, totals[b] per bucket.
__global__ void k_gbpart_scan(int64_t* hist, int grid, int nb,
                              int64_t* totals) {
  const int J = 8;            // buckets per block (one 64-B line)
  const int C = BLOCK / J;    // grid-chunks per bucket
  int j = threadIdx.x % J;
  int cidx = threadIdx.x / J;
  int b = blockIdx.x * J + j;
  __shared__ int64_t s_sum[BLOCK];  // [chunk][bucket-lane]
  int64_t per = ((int64_t)grid + C - 1) / C;
  int64_t g0 = cidx * per;
  int64_t g1 = min((int64_t)grid, g0 + per);
  int64_t local = 0;
  for (int64_t g = g0; g < g1; g++) local += hist[g * nb + b];
  s_sum[cidx * J + j] = local;
  __syncthreads();
  // Hillis-Steele over the chunk dimension, per bucket lane
  for (int d = 1; d < C; d <<= 1) {
    int64_t v = (cidx >= d) ? s_sum[(cidx - d) * J + j] : 0;
    __syncthreads();
    s_sum[cidx * J + j] += v;
    __syncthreads();
  }
  int64_t run = s_sum[cidx * J + j] - local;
  for (int64_t g = g0; g < g1; g++) {
    int64_t v = hist[g * nb + b];
    hist[g * nb + b] = run;
    run += v;
  }
  if (cidx == C - 1) totals[b] = s_sum[(C - 1) * J + j];
}

// 1 block: exclusive scan of bucket totals → absolute bases. Parallel
// Hillis-Steele (the serial loop measured 137 µs/step at nb=1024 — pure
// dependent-load latency; this runs in ~5 µs).
__global__ void k_gbpart_bases(int64_t* totals, int nb, int64_t* bases) {
  // launched with 1024 threads; nb ≤ 4096 → ≤4 elements per thread, kept
  // in named scalars (runtime-indexed locals would spill to scratch,
  // cdna guide §5.4)
  __shared__ int64_t s[4096];
  int i0 = threadIdx.x, i1 = i0 + 1024, i2 = i0 + 2048, i3 = i0 + 3072;
  if (i0 < nb) s[i0] = totals[i0];
  if (i1 < nb) s[i1] = totals[i1];
  if (i2 < nb) s[i2] = totals[i2];
  if (i3 < nb) s[i3] = totals[i3];
  __syncthreads();
  for (int d = 1; d < nb; d <<= 1) {
    int64_t v0 = (i0 < nb && i0 >= d) ? s[i0 - d] : 0;
    int64_t v1 = (i1 < nb && i1 >= d) ? s[i1 - d] : 0;
    int64_t v2 = (i2 < nb && i2 >= d) ? s[i2 - d] : 0;
    int64_t v3 = (i3 < nb && i3 >= d) ? s[i3 - d] : 0;
    __syncthreads();
    if (i0 < nb) s[i0] += v0;
    if (i1 < nb) s[i1] += v1;
    if (i2 < nb) s[i2] += v2;
    if (i3 < nb) s[i3] += v3;
    __syncthreads();
  }
  // s is the inclusive scan; subtract own total for exclusive bases
  if (i0 < nb) bases[i0] = s[i0] - totals[i0];
  if (i1 < nb) bases[i1] = s[i1] - totals[i1];
  if (i2 < nb) bases[i2] = s[i2] - totals[i2];
  if (i3 < nb) bases[i3] = s[i3] - totals[i3];
  if (i0 == 0) bases[nb] = s[nb - 1];
}

// scatter records (key u64 + nvals f64/i64 values) bucket-major
__global__ void k_gbpart_scatter(ColsArg C, int64_t n, const KeyArg* Kp,
                                 ProgArg pred, const DsxInstr* agg_progs,
                                 const int32_t* agg_lens,
                                 const int32_t* val_of /*[naggs] or -1*/,
                                 int naggs, int nvals, int nb,
                                 const int64_t* hist /*bases per blk*/,
                                 const int64_t* bases, uint64_t* out_rec) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // running absolute offset per bucket for THIS block
  int64_t* s_off = (int64_t*)smem;
  for (int i = threadIdx.x; i < nb; i += BLOCK)
    s_off[i] = bases[i] + hist[(int64_t)blockIdx.x * nb + i];
  __syncthreads();
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  int rec = 1 + nvals;
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    if (pred.len) {
      Slot pv;
      bool pvalid = vm_eval(pred.ins, pred.len, C, r, pv);
      if (!(pvalid && pv.i != 0)) continue;
    }
    uint64_t code = pack_key(*Kp, C, r);
    int b = gb_bucket(code, nb - 1);
    int64_t o = (int64_t)atomicAdd((unsigned long long*)&s_off[b], 1ull);
    uint64_t* dst = out_rec + o * rec;
    dst[0] = code;
    const DsxInstr* p = agg_progs;
    for (int a = 0; a < naggs; a++) {
      if (val_of[a] >= 0) {
        Slot v;
        vm_eval(p, agg_lens[a], C, r, v);  // never-null guaranteed by host
        dst[1 + val_of[a]] = (uint64_t)v.i;
      }
      p += DSX_MAX_PROG;
    }
  }
}

// one block per bucket: LDS open-addressing aggregate over the bucket's
// contiguous record run; bump-append compacted groups (AoS temporaries)
__global__ void __launch_bounds__(BLOCK)
k_gbpart_aggregate(const uint64_t* recs, const int64_t* bases, int nvals,
                   const AggArg* Ap, int lds_slots,
                   unsigned long long* g_counter, uint64_t* tmp_codes,
                   uint64_t* tmp_vals /*[G][nvals]*/,
                   unsigned long long* tmp_gcnt, int* overflow) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* l_keys = (uint64_t*)smem;                       // [slots]
  uint64_t* l_vals = l_keys + lds_slots;                    // [slots][nvals]
  uint32_t* l_gcnt = (uint32_t*)(l_vals + (int64_t)lds_slots * nvals);
  int naggs = Ap->naggs;
  for (int i = threadIdx.x; i < lds_slots; i += BLOCK) {
    l_keys[i] = EMPTY_KEY;
    l_gcnt[i] = 0;
  }
  // per-value-slot identity: value slots are the non-COUNT aggs in order
  for (int i = threadIdx.x; i < lds_slots * nvals; i += BLOCK) {
    int vslot = i % nvals;
    int seen = 0;
    uint64_t ident = 0;
    for (int a = 0; a < naggs; a++) {
      int op = Ap->op[a];
      if (op == DSX_AGG_COUNT) continue;
      if (seen == vslot) {
        ident = agg_identity(op);
        break;
      }
      seen++;
    }
    l_vals[i] = ident;
  }
  __syncthreads();

  int64_t r0 = bases[blockIdx.x];
  int64_t r1 = bases[blockIdx.x + 1];
  int rec = 1 + nvals;
  int mask = lds_slots - 1;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += BLOCK) {
    const uint64_t* src = recs + r * rec;
    uint64_t code = src[0];
    int s = (int)(mix64(code) & (uint64_t)mask);
    int probes = 0;
    while (true) {
      unsigned long long k = l_keys[s];
      if (k == code) break;
      if (k == EMPTY_KEY) {
        unsigned long long old = atomicCAS(
            (unsigned long long*)&l_keys[s], EMPTY_KEY,
            (unsigned long long)code);
        if (old == EMPTY_KEY || old == code) break;
      }
      s = (s + 1) & mask;
      if (++probes > lds_slots) {
        *overflow = 1;
        return;
      }
    }
    atomicAdd(&l_gcnt[s], 1u);
    int vs = 0;
    for (int a = 0; a < naggs; a++) {
      int op = Ap->op[a];
      if (op == DSX_AGG_COUNT) continue;
      uint64_t raw = src[1 + vs];
      uint64_t* dst = &l_vals[(int64_t)s * nvals + vs];
      switch (op) {
        case DSX_AGG_SUM_F64:
          unsafeAtomicAdd((double*)dst, __longlong_as_double((long long)raw));
          break;
        case DSX_AGG_SUM_I64:
          atomicAdd((unsigned long long*)dst, (unsigned long long)raw);
          break;
        case DSX_AGG_MIN_F64:
          atomicMin((unsigned long long*)dst,
                    (unsigned long long)f64_ordered(
                        __longlong_as_double((long long)raw)));
          break;
        case DSX_AGG_MAX_F64:
          atomicMax((unsigned long long*)dst,
                    (unsigned long long)f64_ordered(
                        __longlong_as_double((long long)raw)));
          break;
        case DSX_AGG_MIN_I64:
          atomicMin((unsigned long long*)dst,
                    (unsigned long long)i64_ordered((int64_t)raw));
          break;
        case DSX_AGG_MAX_I64:
          atomicMax((unsigned long long*)dst,
                    (unsigned long long)i64_ordered((int64_t)raw));
          break;
      }
      vs++;
    }
  }
  __syncthreads();
  // count live slots, reserve output range, append
  __shared__ unsigned long long s_base;
  __shared__ unsigned int s_local;
  if (threadIdx.x == 0) s_local = 0;
  __syncthreads();
  unsigned int my_rank = 0;
  bool live = false;
  // each thread owns slots i = tid, tid+256, ... — two-phase rank
  for (int i = threadIdx.x; i < lds_slots; i += BLOCK)
    if (l_keys[i] != EMPTY_KEY) my_rank++;  // count per thread
  unsigned int my_count = my_rank;
  // block scan of per-thread counts
  __shared__ unsigned int s_scan[BLOCK];
  s_scan[threadIdx.x] = my_count;
  __syncthreads();
  for (int d = 1; d < BLOCK; d <<= 1) {
    unsigned int v = (threadIdx.x >= d) ? s_scan[threadIdx.x - d] : 0;
    __syncthreads();
    s_scan[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned int my_excl = s_scan[threadIdx.x] - my_count;
  if (threadIdx.x == BLOCK - 1) {
    unsigned int tot = s_scan[BLOCK - 1];
    s_base = tot ? atomicAdd(g_counter, (unsigned long long)tot) : 0;
    s_local = tot;
  }
  __syncthreads();
  if (s_local == 0) return;
  unsigned long long base = s_base;
  unsigned int o = my_excl;
  for (int i = threadIdx.x; i < lds_slots; i += BLOCK) {
    if (l_keys[i] == EMPTY_KEY) continue;
    int64_t dst = (int64_t)(base + o);
    tmp_codes[dst] = l_keys[i];
    tmp_gcnt[dst] = (unsigned long long)l_gcnt[i];
    for (int v = 0; v < nvals; v++)
      tmp_vals[dst * nvals + v] = l_vals[(int64_t)i * nvals + v];
    o++;
  }
  (void)live;
}

// finalize: AoS temporaries → the [naggs][G] output slabs (emit format)
__global__ void k_gbpart_finalize(const uint64_t* tmp_codes,
                                  const uint64_t* tmp_vals,
                                  const unsigned long long* tmp_gcnt,
                                  int64_t G, int nvals, AggArg A,
                                  uint64_t* out_codes, uint64_t* out_vals,
                                  uint64_t* out_counts) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < G; i += stride) {
    out_codes[i] = tmp_codes[i];
    int vs = 0;
    for (int a = 0; a < A.naggs; a++) {
      uint64_t raw = 0;
      if (A.op[a] != DSX_AGG_COUNT) {
        raw = tmp_vals[i * nvals + vs];
        switch (A.op[a]) {
          case DSX_AGG_MIN_F64:
          case DSX_AGG_MAX_F64:
            raw = (uint64_t)__double_as_longlong(f64_unordered(raw));
            break;
          case DSX_AGG_MIN_I64:
          case DSX_AGG_MAX_I64:
            raw = raw ^ 0x8000000000000000ull;
            break;
        }
        vs++;
      }
      out_vals[(int64_t)a * G + i] = raw;
      out_counts[(int64_t)a * G + i] = (uint64_t)tmp_gcnt[i];
    }
  }
}

__global__ void k_init_aggs(uint64_t* g_vals, AggArg A, int64_t slots) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < (int64_t)A.naggs * slots; i += stride)
    g_vals[i] = agg_identity(A.op[(int)(i / slots)]);
}

// compaction with per-agg output pointers; G known after the count pass
template <int DIRECT>
__global__ void k_groupby_emit(const uint64_t* tkeys, int64_t slots,
                               const uint64_t* g_vals,
                               const unsigned long long* g_cnts,
                               const unsigned long long* g_gcnt, AggArg A,
                               int64_t G, unsigned long long* counter,
                               uint64_t* out_codes, uint64_t* out_vals_flat,
                               uint64_t* out_counts_flat) {
  int64_t lo, hi;
  block_range(slots, 1, lo, hi);
  for (int64_t s = lo + threadIdx.x; s < hi; s += BLOCK) {
    bool live = DIRECT ? (g_gcnt[s] > 0) : (tkeys[s] != EMPTY_KEY);
    if (!live) continue;
    unsigned long long o = atomicAdd(counter, 1ull);
    out_codes[o] = DIRECT ? (uint64_t)s : tkeys[s];
    for (int a = 0; a < A.naggs; a++) {
      uint64_t raw = g_vals[(int64_t)a * slots + s];
      switch (A.op[a]) {
        case DSX_AGG_MIN_F64:
        case DSX_AGG_MAX_F64:
          raw = (uint64_t)__double_as_longlong(f64_unordered(raw));
          break;
        case DSX_AGG_MIN_I64:
        case DSX_AGG_MAX_I64:
          raw = raw ^ 0x8000000000000000ull;
          break;
      }
      out_vals_flat[(int64_t)a * G + (int64_t)o] = raw;
      out_counts_flat[(int64_t)a * G + (int64_t)o] = A.never_null[a]
          ? (uint64_t)g_gcnt[s]
          : (uint64_t)g_cnts[(int64_t)a * slots + s];
    }
  }
}

// ---- finish: every group-by output column in one launch --------------------
// (dsx_hash_groupby_cols; arithmetic in gb_finish.h). The argument block is
// passed BY VALUE: through a global pointer the compiler reloads every
// destination pointer per store (note at k_hash_probe_mat); as a kernel
// argument its launch-uniform fields sit in SGPRs, and the loops below are
// fully unrolled so each field is read at a compile-time index.
struct GbFinishArg {
  DsxGbKeyPlan key[DSX_MAX_KEYS];
  uint64_t* kdata[DSX_MAX_KEYS];
  uint8_t* kvalid[DSX_MAX_KEYS];  // nullptr: the key cannot be NULL
  uint64_t* adata[DSX_MAX_AGGS];
  uint8_t* avalid[DSX_MAX_AGGS];  // nullptr for COUNT
  int32_t kind[DSX_MAX_AGGS];     // DSX_GBF_*
  int32_t vidx[DSX_MAX_AGGS];     // accumulator index in the source layout
  int32_t nn[DSX_MAX_AGGS];       // never-NULL input: count = group rows
  int32_t nkeys, ncalls;
};

template <class Src>
__device__ __forceinline__ void gb_finish_row(const GbFinishArg& F, int64_t o,
                                              uint64_t code, const Src& src) {
#pragma unroll
  for (int j = 0; j < DSX_MAX_KEYS; j++) {
    if (j >= F.nkeys) break;
    uint64_t bits;
    int valid = dsx_gbf_key_value(code, F.key[j], &bits);
    F.kdata[j][o] = bits;
    if (F.kvalid[j]) F.kvalid[j][o] = (uint8_t)valid;
  }
#pragma unroll
  for (int a = 0; a < DSX_MAX_AGGS; a++) {
    if (a >= F.ncalls) break;
    uint64_t cnt = src.count(F.vidx[a], F.nn[a]);
    uint64_t raw = F.kind[a] == DSX_GBF_COUNT ? 0ull : src.raw(F.vidx[a]);
    uint64_t bits;
    int valid = dsx_gbf_finalize(F.kind[a], raw, cnt, &bits);
    F.adata[a][o] = bits;
    if (F.avalid[a]) F.avalid[a][o] = (uint8_t)valid;
  }
}

// partition path: reads the aggregate's AoS temporaries as they are (all
// inputs never-NULL there, so every count is the group's row count)
struct GbSrcAos {
  const uint64_t* vals;  // this group's [nvals] record
  uint64_t gcnt;
  __device__ __forceinline__ uint64_t raw(int v) const { return vals[v]; }
  __device__ __forceinline__ uint64_t count(int, int) const { return gcnt; }
};

__global__ void __launch_bounds__(BLOCK)
k_gb_finish_aos(GbFinishArg F, const uint64_t* tmp_codes,
                const uint64_t* tmp_vals, const unsigned long long* tmp_gcnt,
                int64_t G, int nvals) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (; i < G; i += stride) {
    GbSrcAos src{tmp_vals + i * nvals, (uint64_t)tmp_gcnt[i]};
    gb_finish_row(F, i, tmp_codes[i], src);
  }
}

// direct / global paths: the compaction of k_groupby_emit with the column
// writes fused in — reads the accumulator tables, no [naggs][G] slabs
struct GbSrcTable {
  const uint64_t* g_vals;
  const unsigned long long* g_cnts;
  uint64_t gcnt;
  int64_t slots, s;
  __device__ __forceinline__ uint64_t raw(int a) const {
    return g_vals[(int64_t)a * slots + s];
  }
  __device__ __forceinline__ uint64_t count(int a, int nn) const {
    return nn ? gcnt : (uint64_t)g_cnts[(int64_t)a * slots + s];
  }
};

template <int DIRECT>
__global__ void __launch_bounds__(BLOCK)
k_gb_finish_table(GbFinishArg F, const uint64_t* tkeys, int64_t slots,
                  const uint64_t* g_vals, const unsigned long long* g_cnts,
                  const unsigned long long* g_gcnt, int64_t G,
                  unsigned long long* counter) {
  int64_t lo, hi;
  block_range(slots, 1, lo, hi);
  for (int64_t s = lo + threadIdx.x; s < hi; s += BLOCK) {
    bool live = DIRECT ? (g_gcnt[s] > 0) : (tkeys[s] != EMPTY_KEY);
    if (!live) continue;
    int64_t o = (int64_t)atomicAdd(counter, 1ull);
    if (o >= G) continue;  // cannot happen: G counted with the same test
    GbSrcTable src{g_vals, g_cnts, (uint64_t)g_gcnt[s], slots, s};
    gb_finish_row(F, o, DIRECT ? (uint64_t)s : tkeys[s], src);
  }
}

// what dsx_hash_groupby_cols asks of the group-by drivers below
struct GbFinishReq {
  const DsxGbFinishCall* calls;
  int ncalls;
  void** out_datas;      // [nkeys + ncalls], keys first
  uint8_t** out_valids;
};

// allocate the output columns for G groups and fill F. On failure nothing
// stays allocated.
static int gb_finish_alloc(DsxCtx* c, const GbFinishReq& R, const KeyArg& K,
                           const AggArg& A, int64_t G, GbFinishArg* F) {
  memset(F, 0, sizeof(*F));
  F->nkeys = K.nkeys;
  F->ncalls = R.ncalls;
  int nout = K.nkeys + R.ncalls;
  for (int i = 0; i < nout; i++) {
    R.out_datas[i] = nullptr;
    R.out_valids[i] = nullptr;
  }
  int64_t g1 = G > 0 ? G : 1;
  int rc = 0;
  for (int i = 0; i < nout && !rc; i++) {
    bool want_valid;
    if (i < K.nkeys) {
      const DsxKeySpec& k = K.k[i];
      uint64_t space = k.mode == 1
                           ? 1
                           : (uint64_t)k.range + (k.nullable ? 1 : 0);
      F->key[i] = dsx_gbf_key_plan(K.stride[i], space, k.min, k.nullable,
                                   k.mode);
      want_valid = k.mode == 1 || k.nullable;
    } else {
      const DsxGbFinishCall& cl = R.calls[i - K.nkeys];
      F->kind[i - K.nkeys] = cl.kind;
      F->vidx[i - K.nkeys] = cl.agg;
      F->nn[i - K.nkeys] = A.never_null[cl.agg];
      want_valid = cl.kind != DSX_GBF_COUNT;
    }
    rc = pool_alloc(c, g1 * 8, &R.out_datas[i]);
    if (!rc && want_valid) rc = pool_alloc(c, g1, (void**)&R.out_valids[i]);
  }
  if (rc) {
    for (int i = 0; i < nout; i++) {
      if (R.out_datas[i]) pool_release(c, R.out_datas[i]);
      if (R.out_valids[i]) pool_release(c, R.out_valids[i]);
      R.out_datas[i] = nullptr;
      R.out_valids[i] = nullptr;
    }
    return rc;
  }
  for (int i = 0; i < K.nkeys; i++) {
    F->kdata[i] = (uint64_t*)R.out_datas[i];
    F->kvalid[i] = R.out_valids[i];
  }
  for (int i = 0; i < R.ncalls; i++) {
    F->adata[i] = (uint64_t*)R.out_datas[K.nkeys + i];
    F->avalid[i] = R.out_valids[K.nkeys + i];
  }
  return 0;
}

__global__ void k_count_live(const uint64_t* tkeys,
                             const unsigned long long* g_gcnt, int64_t slots,
                             int direct, unsigned long long* counter) {
  int64_t lo, hi;
  block_range(slots, 1, lo, hi);
  unsigned long long local = 0;
  for (int64_t s = lo + threadIdx.x; s < hi; s += BLOCK) {
    bool live = direct ? (g_gcnt[s] > 0) : (tkeys[s] != EMPTY_KEY);
    if (live) local++;
  }
  for (int d = 32; d > 0; d >>= 1) local += __shfl_down(local, d, 64);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(counter, local);
}


// host driver for the partition path; *fell_back=true → caller uses the CAS
// path (LDS table overflow from key skew, or shapes it does not cover)
// direct_shift ≥ 0 selects RANGE bucketing + the direct-index aggregate
// (no hash table in LDS); pick_direct_shift decides, the wrapper retries
// with hashing when the range histogram turns out skewed (*redo).
static void gb_hist_evict_ptr(DsxCtx* c, void* p) {
  if (c->gb_hist_cache.empty()) return;
  for (size_t i = 0; i < c->gb_hist_cache.size();) {
    bool dead = false;
    for (int j = 0; j < c->gb_hist_cache[i].nsrc; j++)
      if (c->gb_hist_cache[i].srcs[j] == p) dead = true;
    if (dead) {
      // NOTE: release the entry's own buffers WITHOUT re-entering the
      // eviction hook (they are never key sources)
      DsxCtx::GbHist h = c->gb_hist_cache[i];
      c->gb_hist_cache.erase(c->gb_hist_cache.begin() + i);
      pool_release(c, h.hist);
      pool_release(c, h.bases);
    } else {
      i++;
    }
  }
}

static int pick_direct_shift(uint64_t key_space, int nvals) {
  static const bool off = getenv("DSX_GB_NO_DIRECT") != nullptr;
  if (off || !jit_enabled() || key_space == 0) return -1;
  if (key_space > (4ull << 20)) return -1;  // nb would exceed 2048
  int64_t slot_b = 8 * (int64_t)(nvals ? nvals : 0) + 4;
  static const int ds_cfg = [] {
    const char* e = getenv("DSX_GB_DS");
    return e ? atoi(e) : 12;  // measured best at C2 (scatter likes fewer,
                              // longer bucket runs; aggregate flat 10..12)
  }();
  int ds = ds_cfg;  // 4096 slots default
  while (ds > 6 && ((1ll << ds) * slot_b) > 88 * 1024) ds--;
  // keep the aggregate grid >=128 blocks when the space allows
  while (ds > 6 &&
         (int64_t)((key_space + (1ull << ds) - 1) >> ds) < 128)
    ds--;
  int64_t nbd = (int64_t)((key_space + (1ull << ds) - 1) >> ds);
  if (nbd > 4096) return -1;
  return ds;
}

static int groupby_partition_impl(
    DsxCtx* c, ColsArg& C, int64_t n, KeyArg& K, ProgArg& P, AggArg& A,
    const DsxAggSpec* aggs_arr, std::vector<DsxInstr>& progs,
    std::vector<int32_t>& lens, int naggs, int64_t g_est, uint64_t key_space,
    uint64_t** out_codes, void** out_vals, uint64_t** out_counts,
    int64_t* out_groups, bool* fell_back, int direct_shift, bool* redo,
    const GbFinishReq* fin) {
  *fell_back = false;
  // SoA u32-code records (u32 codes + u64 vals) — MEASURED REGRESSION at C2
  // (35.0 vs 45.8 G rows/s): splitting the record doubles the number of
  // distinct cache lines each scattered append touches, and line touches,
  // not bytes, dominate the scatter cost. Kept behind an opt-in knob as the
  // recorded experiment; AoS 16-B records are the default.
  static const bool code32_enabled = getenv("DSX_CODE32") != nullptr;
  bool code32 = code32_enabled && key_space > 0 &&
                key_space <= (1ull << 32);
  int32_t val_of[DSX_MAX_AGGS];
  int nvals = 0;
  for (int a = 0; a < naggs; a++)
    val_of[a] = (A.op[a] == DSX_AGG_COUNT) ? -1 : nvals++;
  // bucket-count tradeoff (measured): fewer buckets lengthen write runs
  // (less 16-B-store line-merge loss in L2) but shrink the aggregate grid
  // and grow its LDS table; 1024 targets the best total at C2 shape
  // (512: scatter −0.17 ms but aggregate +0.81 ms)
  static const int nb_target = [] {
    const char* e = getenv("DSX_GB_NB_TARGET");
    return e ? atoi(e) : 1024;  // groups per bucket (tradeoff note above)
  }();
  int nb;
  int lds_slots;
  size_t lds_bytes;
  if (direct_shift >= 0) {
    // one bucket covers 2^shift consecutive codes; aggregate LDS =
    // [slots][nvals] vals + [slots] gcnt, direct-indexed by code low bits
    int64_t nbd =
        (int64_t)((key_space + (1ull << direct_shift) - 1) >> direct_shift);
    nb = (int)((nbd + 7) & ~7ll);  // k_gbpart_scan wants a multiple of 8
    lds_slots = 1 << direct_shift;
    lds_bytes = (size_t)lds_slots * (8 * (size_t)nvals + 4);
  } else {
    nb = 64;
    while (nb < 4096 && g_est / nb > nb_target) nb <<= 1;
    int64_t per_bucket = (g_est + nb - 1) / nb;
    lds_slots = 256;
    while (lds_slots < 2 * per_bucket) lds_slots <<= 1;
    int64_t slot_bytes = 8 + 8 * (int64_t)nvals + 4;
    lds_bytes = (size_t)lds_slots * slot_bytes;
  }
  if (lds_bytes > 96 * 1024) {
    *fell_back = true;
    return 0;
  }
  static const int max_grid = [] {
    const char* e = getenv("DSX_GB_GRID");
    return e ? atoi(e) : MAX_GRID;
  }();
  // Rows-per-block bound: the per-block histogram is
  // grid × nb counters, which the scan reads and writes and the scatter
  // reads again — at Q3 (3 M rows, nb 4096) 2048 blocks make it larger than
  // the input. So a block owns at least nb rows: the largest power of two g
  // with g·nb ≤ n, floored at one block per CU (256; hist and scatter lose
  // more below it than the scan gains) and capped as before. C2 (100 M rows,
  // nb 248) keeps 2048. DSX_GB_GRID stays an upper cap.
  int64_t g_rows = 256;
  while (g_rows < MAX_GRID && g_rows * 2 * nb <= n) g_rows <<= 1;
  int grid = (int)min(min((int64_t)max_grid, (n + BLOCK - 1) / BLOCK), g_rows);
  if (grid == 0 && fin) {
    GbFinishArg F;
    *out_groups = 0;
    return gb_finish_alloc(c, *fin, K, A, 0, &F);
  }
  if (grid == 0) {  // empty input → empty output
    int rc2 = pool_alloc(c, 8, (void**)out_codes);
    if (!rc2) rc2 = pool_alloc(c, 8, out_vals);
    if (!rc2) rc2 = pool_alloc(c, 8, (void**)out_counts);
    *out_groups = 0;
    return rc2;
  }
  int64_t prog_bytes = (int64_t)progs.size() * sizeof(DsxInstr);
  int64_t lens_bytes = naggs * 4;
  int64_t Gcap = g_est;
  int rec = 1 + nvals;
  // records live in the persistent scratch arena: a per-call hipMalloc/Free
  // of ~GBs costs tens of ms (measured); the arena amortizes it
  int64_t n1 = n > 0 ? n : 1;
  int64_t rec_bytes = n1 * (int64_t)rec * 8;
  {  // SoA (code32) view may need slightly more at tiny n (256-B alignment)
    int64_t soa = ((n1 * 4 + 255) / 256) * 256 + n1 * (int64_t)nvals * 8;
    if (soa > rec_bytes) rec_bytes = soa;
  }
  int64_t need = prog_bytes + ((lens_bytes + 15) / 16) * 16 + 64 +
                 sizeof(KeyArg) + sizeof(AggArg) + 32 +
                 (int64_t)grid * nb * 8 + (nb + 2) * 8 + nb * 8 +
                 (int64_t)grid * nb * 4 + 16 +
                 Gcap * 8 + Gcap * (int64_t)(nvals ? nvals : 1) * 8 +
                 Gcap * 8 + ((naggs * 4 + 15) / 16) * 16 + 256 + rec_bytes;
  int rc = ensure_scratch(c, need);
  if (rc) return rc;
  char* base = (char*)c->scratch;
  DsxInstr* d_progs = (DsxInstr*)base;
  base += prog_bytes;
  int32_t* d_lens = (int32_t*)base;
  base += ((lens_bytes + 15) / 16) * 16;
  int32_t* d_val_of = (int32_t*)base;
  base += ((naggs * 4 + 15) / 16) * 16;
  unsigned long long* d_counter = (unsigned long long*)base;
  base += 16;
  int* d_ovf = (int*)base;
  base += 16;
  KeyArg* d_K = (KeyArg*)base;
  base += ((sizeof(KeyArg) + 15) / 16) * 16;
  AggArg* d_A = (AggArg*)base;
  base += ((sizeof(AggArg) + 15) / 16) * 16;
  int64_t* d_hist = (int64_t*)base;
  base += (int64_t)grid * nb * 8;
  int64_t* d_totals = (int64_t*)base;
  base += nb * 8;
  int64_t* d_bases = (int64_t*)base;
  base += (nb + 2) * 8;
  uint32_t* d_selcnt = (uint32_t*)base;
  base += (((int64_t)grid * nb * 4 + 15) / 16) * 16;
  uint64_t* d_tmp_codes = (uint64_t*)base;
  base += Gcap * 8;
  uint64_t* d_tmp_vals = (uint64_t*)base;
  base += Gcap * (int64_t)(nvals ? nvals : 1) * 8;
  unsigned long long* d_tmp_gcnt = (unsigned long long*)base;
  base += Gcap * 8;
  uint64_t* d_recs = (uint64_t*)base;

  HIP_TRY(hipMemcpyAsync(d_progs, progs.data(), prog_bytes,
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_lens, lens.data(), lens_bytes,
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_val_of, val_of, naggs * 4, hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipMemcpyAsync(d_K, &K, sizeof(KeyArg), hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipMemcpyAsync(d_A, &A, sizeof(AggArg), hipMemcpyHostToDevice,
                         c->stream));
  // d_counter and d_ovf are adjacent 16-byte cells: one memset, and one
  // copy back after the aggregate kernel
  HIP_TRY(hipMemsetAsync(d_counter, 0, 32, c->stream));

  // staged-scatter tile size: largest multiple of 1024 whose LDS footprint
  // (s_off + counters + bucket tags + AoS stage) fits the CU's 160 KiB,
  // leaving headroom; 0 disables (fallback to the plain scatter)
  static const int sthreads_cfg = [] {
    const char* e = getenv("DSX_SCATTER_THREADS");
    return e ? atoi(e) : 1024;  // measured best at C2 (1.24→1.04 ms)
  }();
  static const long tile_cfg = [] {
    const char* e = getenv("DSX_SCATTER_TILE");
    // default 0 = plain scatter: the staged variant measured SLOWER at
    // every feasible tile (LDS cost + double-eval beat the write-merge
    // gain; see DESIGN.md negative results) — kept as an opt-in knob
    return e ? atol(e) : 0;
  }();
  int tile = 0;
  if (tile_cfg != 0 && nb <= sthreads_cfg) {
    const long LDS_BUDGET = 148 * 1024;
    long fixed = (long)nb * 8 + (long)nb * 4 + ((long)nb + 1) * 4 + 16;
    long per_row = 2 + (long)rec * 8;
    long t = tile_cfg > 0 ? tile_cfg
                          : (LDS_BUDGET - fixed) / per_row / 1024 * 1024;
    if (t > 8192) t = 8192;
    if (t >= sthreads_cfg) tile = (int)t;
  }
  JitEntry* je = jit_source_entry(
      c, jit_gbpart_source(C, K, P, aggs_arr, A, val_of, naggs, nvals,
                           lds_slots, code32, tile, direct_shift));
  hipFunction_t f_hist = je ? jit_fn(c, je, "j_hist") : nullptr;
  hipFunction_t f_scat = je ? jit_fn(c, je, "j_scatter") : nullptr;
  hipFunction_t f_scat_staged =
      (je && tile > 0) ? jit_fn(c, je, "j_scatter_staged") : nullptr;
  hipFunction_t f_aggr = je ? jit_fn(c, je, "j_aggregate") : nullptr;
  if (!(f_hist && f_scat && f_aggr)) {
    if (direct_shift >= 0) {
      // direct mode exists only as JIT; retry hashed (static fallback ok)
      *redo = true;
      return 0;
    }
    // all-or-nothing: scatter and aggregate must agree on record layout
    f_hist = f_scat = f_scat_staged = f_aggr = nullptr;
    code32 = false;
  }
  // SoA views over the record arena (code32): u32 codes, then u64 vals
  uint32_t* d_rcodes = (uint32_t*)d_recs;
  uint64_t* d_rvals =
      (uint64_t*)((char*)d_recs + (((int64_t)(n > 0 ? n : 1) * 4 + 255) / 256) *
                                      256);
  if (f_hist && f_scat) {
    // per-table (hist, bases) cache: the JIT histogram is predicate-free,
    // a pure function of the key column — repeat steps skip hist+scan
    uint64_t hsig = ((uint64_t)n * 0x9E3779B97F4A7C15ull) ^ key_space ^
                    ((uint64_t)nb << 1) ^ ((uint64_t)grid << 17) ^
                    (uint64_t)(direct_shift + 2);
    auto hmix = [](uint64_t x) {
      x += 0x9E3779B97F4A7C15ull;
      x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
      x ^= x >> 27; x *= 0x94D049BB133111EBull;
      return x ^ (x >> 31);
    };
    for (int j = 0; j < K.nkeys; j++) {
      hsig = hmix(hsig ^ (uint64_t)(uintptr_t)C.data[K.k[j].col]);
      hsig = hmix(hsig ^ (uint64_t)K.k[j].min ^
                  ((uint64_t)K.k[j].range << 8));
    }
    DsxCtx::GbHist* hit = nullptr;
    if (c->gb_hist_cache_on)
      for (auto& h : c->gb_hist_cache)
        if (h.sig == hsig) hit = &h;
    if (hit != nullptr) {
      d_hist = (int64_t*)hit->hist;
      d_bases = (int64_t*)hit->bases;
    } else {
      DsxCtx::GbHist ch{};
      ch.sig = hsig;
      ch.nsrc = K.nkeys;
      for (int j = 0; j < K.nkeys; j++) ch.srcs[j] = C.data[K.k[j].col];
      int rc2 = pool_alloc(c, (int64_t)grid * nb * 8, &ch.hist);
      if (!rc2) rc2 = pool_alloc(c, ((int64_t)nb + 2) * 8, &ch.bases);
      if (rc2) return rc2;
      d_hist = (int64_t*)ch.hist;
      d_bases = (int64_t*)ch.bases;
      {
        ProfScope ps(c, "k_gbpart_hist");
        struct { ColsArg C; int64_t n; int nb; int64_t* hist; } a1{
            C, n, nb, d_hist};
        void* args[] = {&a1.C, &a1.n, &a1.nb, &a1.hist};
        hipModuleLaunchKernel(f_hist, grid, 1, 1, BLOCK, 1, 1,
                              (unsigned)(nb * 4), c->stream, args, nullptr);
      }
      {
        ProfScope ps(c, "k_gbpart_scan");
        hipLaunchKernelGGL(k_gbpart_scan, dim3(nb / 8), dim3(BLOCK), 0,
                           c->stream, d_hist, grid, nb, d_totals);
        hipLaunchKernelGGL(k_gbpart_bases, dim3(1), dim3(1024), 0, c->stream,
                           d_totals, nb, d_bases);
      }
      if (c->gb_hist_cache_on) {
        if (c->gb_hist_cache.size() >= 6) {
          pool_release(c, c->gb_hist_cache.front().hist);
          pool_release(c, c->gb_hist_cache.front().bases);
          c->gb_hist_cache.erase(c->gb_hist_cache.begin());
        }
        c->gb_hist_cache.push_back(ch);
      } else {
        // uncached: hand the buffers back once the call completes — they
        // are read by the aggregate later on the same stream, so release
        // into the stream-ordered pool is safe
        pool_release(c, ch.hist);
        pool_release(c, ch.bases);
      }
    }
    if (hit == nullptr && direct_shift >= 0) {
      // balance guard: a skewed key distribution overloads range buckets
      // (one aggregate block per bucket) — fall back to hash bucketing.
      // Verdict cached per (key data ptr, n, space): repeat steps of the
      // same query skip the totals sync entirely.
      uint64_t sig = (uint64_t)(uintptr_t)C.data[K.k[0].col] ^
                     ((uint64_t)n * 0x9E3779B97F4A7C15ull) ^ key_space;
      auto it = c->gb_guard_cache.find(sig);
      if (it != c->gb_guard_cache.end()) {
        if (it->second != direct_shift) {
          *redo = true;
          return 0;
        }
      } else {
        std::vector<int64_t> h_tot((size_t)nb);
        HIP_TRY(hipMemcpyAsync(h_tot.data(), d_totals, (size_t)nb * 8,
                               hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        int64_t mx = 0, sum = 0;
        for (int i = 0; i < nb; i++) {
          if (h_tot[i] > mx) mx = h_tot[i];
          sum += h_tot[i];
        }
        bool skewed = mx > 8 * (sum / nb) + 65536;
        if (c->gb_guard_cache.size() > 4096) c->gb_guard_cache.clear();
        c->gb_guard_cache[sig] = skewed ? -1 : direct_shift;
        if (skewed) {
          *redo = true;
          return 0;
        }
      }
    }
    {
      ProfScope ps(c, "k_gbpart_scatter");
      static const int sthreads = [] {
        const char* e = getenv("DSX_SCATTER_THREADS");
        return e ? atoi(e) : 1024;  // measured best at C2 (1.24→1.04 ms)
      }();
      // occupancy throttle: padding the dynamic LDS ask caps resident
      // blocks per CU, shrinking the (resident blocks × nb × 64 B) set of
      // open write lines toward the 4 MB/XCD L2 — knob for measuring the
      // scattered-write eviction amplification
      static const unsigned lds_pad = [] {
        const char* e = getenv("DSX_SCATTER_LDS_PAD");
        return e ? (unsigned)atoi(e) : 0u;
      }();
      // NB: grid MUST match the hist pass (per-block bucket bases are keyed
      // by blockIdx); only the thread count may vary.
      hipFunction_t f_use = f_scat_staged ? f_scat_staged : f_scat;
      unsigned smem = (unsigned)(nb * 8) + lds_pad;
      if (f_scat_staged)
        smem = (unsigned)((size_t)nb * 8 + (size_t)nb * 4 +
                          ((size_t)nb + 1) * 4 + 16 + (size_t)tile * 2 +
                          (size_t)tile * rec * 8);
      if (code32) {
        struct {
          ColsArg C; int64_t n; int nb; const int64_t* hist;
          const int64_t* bases; uint32_t* selcnt; uint32_t* oc;
          uint64_t* ov;
        } a2{C, n, nb, d_hist, d_bases, d_selcnt, d_rcodes, d_rvals};
        void* args[] = {&a2.C, &a2.n, &a2.nb, &a2.hist, &a2.bases,
                        &a2.selcnt, &a2.oc, &a2.ov};
        hipModuleLaunchKernel(f_use, grid, 1, 1, sthreads, 1, 1,
                              smem, c->stream, args, nullptr);
      } else {
        struct {
          ColsArg C; int64_t n; int nb; const int64_t* hist;
          const int64_t* bases; uint32_t* selcnt; uint64_t* out;
        } a2{C, n, nb, d_hist, d_bases, d_selcnt, d_recs};
        void* args[] = {&a2.C, &a2.n, &a2.nb, &a2.hist, &a2.bases,
                        &a2.selcnt, &a2.out};
        hipModuleLaunchKernel(f_use, grid, 1, 1, sthreads, 1, 1,
                              smem, c->stream, args, nullptr);
      }
    }
  } else {
    {
      ProfScope ps(c, "k_gbpart_hist");
      hipLaunchKernelGGL(k_gbpart_hist, dim3(grid), dim3(BLOCK),
                         (size_t)nb * 4, c->stream, C, n, d_K, P, nb, d_hist);
    }
    {
      ProfScope ps(c, "k_gbpart_scan");
      hipLaunchKernelGGL(k_gbpart_scan, dim3(nb / 8), dim3(BLOCK), 0,
                         c->stream, d_hist, grid, nb, d_totals);
      hipLaunchKernelGGL(k_gbpart_bases, dim3(1), dim3(1024), 0, c->stream,
                         d_totals, nb, d_bases);
    }
    {
      ProfScope ps(c, "k_gbpart_scatter");
      hipLaunchKernelGGL(k_gbpart_scatter, dim3(grid), dim3(BLOCK),
                         (size_t)nb * 8, c->stream, C, n, d_K, P, d_progs,
                         d_lens, d_val_of, naggs, nvals, nb, d_hist, d_bases,
                         d_recs);
    }
  }
  {
    ProfScope ps(c, "k_gbpart_aggregate");
    if (f_aggr) {
      static const int athreads = [] {
        const char* e = getenv("DSX_AGG_THREADS");
        return e ? atoi(e) : 1024;  // measured best at C2 (0.84→0.46 ms)
      }();
      if (code32) {
        struct {
          const uint32_t* rc; const uint64_t* rv; const int64_t* bases;
          const int64_t* hist; const uint32_t* selcnt; int sgrid;
          unsigned long long* counter; uint64_t* tc; uint64_t* tv;
          unsigned long long* tg; int* ovf;
        } a3{d_rcodes, d_rvals, d_bases, d_hist, d_selcnt, grid, d_counter,
             d_tmp_codes, (uint64_t*)d_tmp_vals, d_tmp_gcnt, d_ovf};
        void* args[] = {&a3.rc, &a3.rv, &a3.bases, &a3.hist, &a3.selcnt,
                        &a3.sgrid, &a3.counter, &a3.tc, &a3.tv, &a3.tg,
                        &a3.ovf};
        hipModuleLaunchKernel(f_aggr, nb, 1, 1, athreads, 1, 1,
                              (unsigned)lds_bytes, c->stream, args, nullptr);
      } else {
        struct {
          const uint64_t* recs; const int64_t* bases; const int64_t* hist;
          const uint32_t* selcnt; int sgrid;
          unsigned long long* counter; uint64_t* tc; uint64_t* tv;
          unsigned long long* tg; int* ovf;
        } a3{d_recs, d_bases, d_hist, d_selcnt, grid, d_counter,
             d_tmp_codes, (uint64_t*)d_tmp_vals, d_tmp_gcnt, d_ovf};
        void* args[] = {&a3.recs, &a3.bases, &a3.hist, &a3.selcnt,
                        &a3.sgrid, &a3.counter, &a3.tc, &a3.tv, &a3.tg,
                        &a3.ovf};
        hipModuleLaunchKernel(f_aggr, nb, 1, 1, athreads, 1, 1,
                              (unsigned)lds_bytes, c->stream, args, nullptr);
      }
    } else {
      hipLaunchKernelGGL(k_gbpart_aggregate, dim3(nb), dim3(BLOCK),
                         lds_bytes, c->stream, d_recs, d_bases,
                         nvals ? nvals : 0, d_A, lds_slots, d_counter,
                         d_tmp_codes, d_tmp_vals, d_tmp_gcnt, d_ovf);
    }
  }
  // the group count and the overflow flag sit 16 bytes apart: one copy
  unsigned long long h_res[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h_res, d_counter, 24, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  unsigned long long G = h_res[0];
  int h_ovf = (int)(uint32_t)h_res[2];
  if (h_ovf) {
    *fell_back = true;
    return 0;
  }
  if (fin) {
    // one launch reads the AoS temporaries and writes every output column;
    // no slabs, and no synchronize after it: the scratch arena it reads is
    // reused only by later work on the same stream
    GbFinishArg F;
    int rc2 = gb_finish_alloc(c, *fin, K, A, (int64_t)G, &F);
    if (rc2) return rc2;
    for (int i = 0; i < F.ncalls; i++)
      F.vidx[i] = val_of[F.vidx[i]] < 0 ? 0 : val_of[F.vidx[i]];
    if (G > 0) {
      int g2 = (int)min((int64_t)MAX_GRID, ((int64_t)G + BLOCK - 1) / BLOCK);
      ProfScope ps(c, "k_gbpart_finalize");
      hipLaunchKernelGGL(k_gb_finish_aos, dim3(g2), dim3(BLOCK), 0, c->stream,
                         F, d_tmp_codes, d_tmp_vals, d_tmp_gcnt, (int64_t)G,
                         nvals ? nvals : 1);
    }
    HIP_TRY(hipGetLastError());
    *out_groups = (int64_t)G;
    return 0;
  }
  {
    int rc2 = pool_alloc(c, (G > 0 ? G : 1) * 8, (void**)out_codes);
    if (!rc2) rc2 = pool_alloc(c, (G > 0 ? G : 1) * 8 * naggs, out_vals);
    if (!rc2) rc2 = pool_alloc(c, (G > 0 ? G : 1) * 8 * naggs,
                               (void**)out_counts);
    if (rc2) return rc2;
  }
  if (G > 0) {
    int g2 = (int)min((int64_t)MAX_GRID, ((int64_t)G + BLOCK - 1) / BLOCK);
    ProfScope ps(c, "k_gbpart_finalize");
    hipLaunchKernelGGL(k_gbpart_finalize, dim3(g2), dim3(BLOCK), 0, c->stream,
                       d_tmp_codes, d_tmp_vals, d_tmp_gcnt, (int64_t)G,
                       nvals ? nvals : 1, A, *out_codes,
                       (uint64_t*)*out_vals, *out_counts);
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipGetLastError());
  *out_groups = (int64_t)G;
  return 0;
}

static int groupby_partition(DsxCtx* c, ColsArg& C, int64_t n, KeyArg& K,
                             ProgArg& P, AggArg& A, const DsxAggSpec* aggs_arr,
                             std::vector<DsxInstr>& progs,
                             std::vector<int32_t>& lens, int naggs,
                             int64_t g_est, uint64_t key_space,
                             uint64_t** out_codes,
                             void** out_vals, uint64_t** out_counts,
                             int64_t* out_groups, bool* fell_back,
                             const GbFinishReq* fin) {
  int nvals_probe = 0;
  for (int a = 0; a < naggs; a++)
    if (A.op[a] != DSX_AGG_COUNT) nvals_probe++;
  int ds = pick_direct_shift(key_space, nvals_probe);
  if (ds >= 0) {
    bool redo = false;
    int rc = groupby_partition_impl(c, C, n, K, P, A, aggs_arr, progs, lens,
                                    naggs, g_est, key_space, out_codes,
                                    out_vals, out_counts, out_groups,
                                    fell_back, ds, &redo, fin);
    if (rc != 0 || !redo) return rc;
  }
  bool redo = false;
  return groupby_partition_impl(c, C, n, K, P, A, aggs_arr, progs, lens,
                                naggs, g_est, key_space, out_codes, out_vals,
                                out_counts, out_groups, fell_back, -1, &redo,
                                fin);
}

/* Toggle the per-table histogram cache (off for externally-backed key
 * columns whose pointers recycle outside the pool's eviction hook). */
extern "C" int dsx_gb_hist_cache_enable(DsxCtx* c, int enable) {
  c->gb_hist_cache_on = enable != 0;
  return 0;
}

static int hash_groupby_impl(DsxCtx* c, const DsxColumn* cols, int ncols,
                             int64_t n, const DsxKeySpec* keys, int nkeys,
                             const DsxInstr* pred, int pred_len,
                             const DsxAggSpec* aggs, int naggs,
                             uint64_t** out_codes, void** out_vals,
                             uint64_t** out_counts, int64_t* out_groups,
                             const GbFinishReq* fin) {
  if (naggs > DSX_MAX_AGGS || ncols > DSX_MAX_COLS || pred_len > DSX_MAX_PROG ||
      nkeys > DSX_MAX_KEYS)
    FAIL(-3, "groupby spec too large");
  KeyArg K{};
  K.nkeys = nkeys;
  uint64_t key_space = 1;
  bool bits_key = false;
  for (int j = 0; j < nkeys; j++) {
    K.k[j] = keys[j];
    K.stride[j] = key_space;
    if (keys[j].mode == 1) {
      if (nkeys != 1) FAIL(-3, "f64-bits key must be the only key");
      bits_key = true;
      continue;
    }
    uint64_t range = (uint64_t)keys[j].range + (keys[j].nullable ? 1 : 0);
    if (range == 0) FAIL(-3, "empty key range");
    if (key_space > (1ull << 62) / range) FAIL(-4, "key space exceeds 2^62");
    key_space *= range;
  }
  if (bits_key) key_space = 0;  // unbounded: CAS hash path only
  ColsArg C{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    C.data[i] = cols[i].data;
    C.validity[i] = cols[i].validity;
    C.dtype[i] = cols[i].dtype;
  }
  ProgArg P{};
  if (pred_len) memcpy(P.ins, pred, pred_len * sizeof(DsxInstr));
  P.len = pred_len;
  AggArg A{};
  A.naggs = naggs;
  for (int a = 0; a < naggs; a++) {
    A.op[a] = aggs[a].op;
    int nn = 1;
    for (int i = 0; i < aggs[a].prog_len; i++) {
      const DsxInstr& in = aggs[a].prog[i];
      if (in.op == DSX_OP_LIT_NULL) nn = 0;
      if (in.op == DSX_OP_COL && cols[in.arg0].validity != nullptr) nn = 0;
    }
    A.never_null[a] = nn;
  }

  // agg programs live in device memory (too big for kernel args)
  std::vector<DsxInstr> progs((size_t)naggs * DSX_MAX_PROG);
  std::vector<int32_t> lens(naggs);
  for (int a = 0; a < naggs; a++) {
    memcpy(&progs[(size_t)a * DSX_MAX_PROG], aggs[a].prog,
           aggs[a].prog_len * sizeof(DsxInstr));
    lens[a] = aggs[a].prog_len;
  }
  int64_t prog_bytes = (int64_t)progs.size() * sizeof(DsxInstr);
  int64_t lens_bytes = naggs * 4;

  // LDS-direct path feasibility: vals(8)+cnts(4) per agg per slot + gcnt(4)
  int64_t lds_per_slot = naggs * 12 + 4;
  bool direct = key_space > 0 && (int64_t)key_space * lds_per_slot <= 64 * 1024;

  int64_t g_est = (int64_t)(key_space && key_space < (uint64_t)n
                                ? (int64_t)key_space
                                : n);
  if (!direct) {
    bool all_nn = true;
    for (int a = 0; a < naggs; a++) all_nn &= (A.never_null[a] != 0);
    static const bool part_disabled = getenv("DSX_DISABLE_PART") != nullptr;
    if (!part_disabled && all_nn && naggs <= 6 && g_est > 0 &&
        key_space > 0) {
      bool fell_back = false;
      int prc = groupby_partition(c, C, n, K, P, A, aggs, progs, lens, naggs,
                                  g_est, key_space, out_codes, out_vals,
                                  out_counts, out_groups, &fell_back, fin);
      if (prc != 0) return prc;
      if (!fell_back) return 0;
    }
  }

  int64_t slots;
  if (direct) {
    slots = (int64_t)key_space;
  } else {
    int64_t est = g_est;
    if (est > (1ll << 26)) est = 1ll << 26;
    slots = 64;
    while (slots < 2 * est) slots <<= 1;
  }

  for (int attempt = 0;; attempt++) {
    // device buffers: tkeys (global path), g_vals, g_cnts, g_gcnt, programs,
    // counter, overflow flag
    int64_t need = prog_bytes + lens_bytes + 8 /*counter*/ + 8 /*ovf*/ +
                   (int64_t)sizeof(KeyArg) + (int64_t)sizeof(AggArg) + 32 +
                   (direct ? 0 : slots * 8) + (int64_t)naggs * slots * 8 +
                   (int64_t)naggs * slots * 8 + slots * 8 + 64;
    int rc = ensure_scratch(c, need);
    if (rc) return rc;
    char* base = (char*)c->scratch;
    DsxInstr* d_progs = (DsxInstr*)base;
    base += prog_bytes;
    int32_t* d_lens = (int32_t*)base;
    base += ((lens_bytes + 15) / 16) * 16;
    unsigned long long* d_counter = (unsigned long long*)base;
    base += 8;
    int* d_ovf = (int*)base;
    base += 8;
    KeyArg* d_K = (KeyArg*)base;
    base += ((sizeof(KeyArg) + 15) / 16) * 16;
    AggArg* d_A = (AggArg*)base;
    base += ((sizeof(AggArg) + 15) / 16) * 16;
    uint64_t* d_tkeys = nullptr;
    if (!direct) {
      d_tkeys = (uint64_t*)base;
      base += slots * 8;
    }
    uint64_t* d_vals = (uint64_t*)base;
    base += (int64_t)naggs * slots * 8;
    unsigned long long* d_cnts = (unsigned long long*)base;
    base += (int64_t)naggs * slots * 8;
    unsigned long long* d_gcnt = (unsigned long long*)base;

    HIP_TRY(hipMemcpyAsync(d_progs, progs.data(), prog_bytes,
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_lens, lens.data(), lens_bytes,
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_K, &K, sizeof(KeyArg), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(d_A, &A, sizeof(AggArg), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemsetAsync(d_counter, 0, 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_ovf, 0, 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_cnts, 0, (size_t)naggs * slots * 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_gcnt, 0, (size_t)slots * 8, c->stream));
    if (!direct) HIP_TRY(hipMemsetAsync(d_tkeys, 0xFF, slots * 8, c->stream));
    {
      int g = (int)min((int64_t)MAX_GRID,
                       ((int64_t)naggs * slots + BLOCK - 1) / BLOCK);
      if (g > 0)
        hipLaunchKernelGGL(k_init_aggs, dim3(g), dim3(BLOCK), 0, c->stream,
                           d_vals, A, slots);
    }

    int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
    if (grid > 0) {
      if (direct) {
        size_t lds_bytes =
            (size_t)(naggs * (int64_t)key_space * 8 +
                     naggs * (int64_t)key_space * 4 + (int64_t)key_space * 4);
        JitEntry* je = jit_source_entry(
            c, jit_direct_source(C, K, P, aggs, A, naggs, (int)key_space));
        hipFunction_t fd = je ? jit_fn(c, je, "j_direct") : nullptr;
        ProfScope ps(c, "k_groupby_direct");
        if (fd) {
          struct {
            ColsArg C; int64_t n; uint64_t* v; unsigned long long* cn;
            unsigned long long* gc;
          } a0{C, n, d_vals, d_cnts, d_gcnt};
          void* args[] = {&a0.C, &a0.n, &a0.v, &a0.cn, &a0.gc};
          hipModuleLaunchKernel(fd, grid, 1, 1, BLOCK, 1, 1,
                                (unsigned)lds_bytes, c->stream, args,
                                nullptr);
        } else {
          hipLaunchKernelGGL(k_groupby_direct, dim3(grid), dim3(BLOCK),
                             lds_bytes, c->stream, C, n, d_K,
                             (int)key_space, P, d_progs, d_lens, d_A, d_vals,
                             d_cnts, d_gcnt);
        }
      } else {
        ProfScope ps(c, "k_groupby_global");
        hipLaunchKernelGGL(k_groupby_global, dim3(grid), dim3(BLOCK), 0,
                           c->stream, C, n, d_K, P, d_progs, d_lens, d_A,
                           d_tkeys, slots - 1, d_vals, d_cnts, d_gcnt, d_ovf);
      }
    }
    HIP_TRY(hipGetLastError());

    int h_ovf = 0;
    HIP_TRY(hipMemcpyAsync(&h_ovf, d_ovf, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h_ovf) {
      if (attempt > 6) FAIL(-5, "groupby table overflow after retries");
      slots <<= 1;
      continue;
    }

    // count live groups
    HIP_TRY(hipMemsetAsync(d_counter, 0, 8, c->stream));
    {
      int g = (int)min((int64_t)MAX_GRID, (slots + BLOCK - 1) / BLOCK);
      hipLaunchKernelGGL(k_count_live, dim3(g), dim3(BLOCK), 0, c->stream,
                         d_tkeys, d_gcnt, slots, direct ? 1 : 0, d_counter);
    }
    unsigned long long G = 0;
    HIP_TRY(hipMemcpyAsync(&G, d_counter, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));

    if (fin) {
      // compaction and column writes in one launch, straight from the
      // accumulator tables; returns with it queued (see the partition path)
      GbFinishArg F;
      int rc2 = gb_finish_alloc(c, *fin, K, A, (int64_t)G, &F);
      if (rc2) return rc2;
      HIP_TRY(hipMemsetAsync(d_counter, 0, 8, c->stream));
      if (G > 0) {
        int g = (int)min((int64_t)MAX_GRID, (slots + BLOCK - 1) / BLOCK);
        ProfScope ps(c, "k_groupby_finish");
        if (direct)
          hipLaunchKernelGGL(k_gb_finish_table<1>, dim3(g), dim3(BLOCK), 0,
                             c->stream, F, d_tkeys, slots, d_vals, d_cnts,
                             d_gcnt, (int64_t)G, d_counter);
        else
          hipLaunchKernelGGL(k_gb_finish_table<0>, dim3(g), dim3(BLOCK), 0,
                             c->stream, F, d_tkeys, slots, d_vals, d_cnts,
                             d_gcnt, (int64_t)G, d_counter);
      }
      HIP_TRY(hipGetLastError());
      *out_groups = (int64_t)G;
      return 0;
    }
    {
      int rc2 = pool_alloc(c, (G > 0 ? G : 1) * 8, (void**)out_codes);
      if (!rc2) rc2 = pool_alloc(c, (G > 0 ? G : 1) * 8 * naggs, out_vals);
      if (!rc2) rc2 = pool_alloc(c, (G > 0 ? G : 1) * 8 * naggs,
                                 (void**)out_counts);
      if (rc2) return rc2;
    }
    HIP_TRY(hipMemsetAsync(d_counter, 0, 8, c->stream));
    if (G > 0) {
      int g = (int)min((int64_t)MAX_GRID, (slots + BLOCK - 1) / BLOCK);
      ProfScope ps(c, "k_groupby_emit");
      if (direct)
        hipLaunchKernelGGL(k_groupby_emit<1>, dim3(g), dim3(BLOCK), 0,
                           c->stream, d_tkeys, slots, d_vals, d_cnts, d_gcnt,
                           A, (int64_t)G, d_counter, *out_codes,
                           (uint64_t*)*out_vals, *out_counts);
      else
        hipLaunchKernelGGL(k_groupby_emit<0>, dim3(g), dim3(BLOCK), 0,
                           c->stream, d_tkeys, slots, d_vals, d_cnts, d_gcnt,
                           A, (int64_t)G, d_counter, *out_codes,
                           (uint64_t*)*out_vals, *out_counts);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out_groups = (int64_t)G;
    return 0;
  }
}

extern "C" int dsx_hash_groupby(DsxCtx* c, const DsxColumn* cols, int ncols,
                                int64_t n, const DsxKeySpec* keys, int nkeys,
                                const DsxInstr* pred,
                                int pred_len, const DsxAggSpec* aggs, int naggs,
                                uint64_t** out_codes, void** out_vals,
                                uint64_t** out_counts, int64_t* out_groups) {
  return hash_groupby_impl(c, cols, ncols, n, keys, nkeys, pred, pred_len,
                           aggs, naggs, out_codes, out_vals, out_counts,
                           out_groups, nullptr);
}

static int gb_finish_calls_check(const DsxAggSpec* aggs, int naggs,
                                 const DsxGbFinishCall* calls, int ncalls);

extern "C" int dsx_hash_groupby_cols(
    DsxCtx* c, const DsxColumn* cols, int ncols, int64_t n,
    const DsxKeySpec* keys, int nkeys, const DsxInstr* pred, int pred_len,
    const DsxAggSpec* aggs, int naggs, const DsxGbFinishCall* calls,
    int ncalls, void** out_datas, uint8_t** out_valids, int64_t* out_groups) {
  if (nkeys < 1 || nkeys > DSX_MAX_KEYS || naggs > DSX_MAX_AGGS ||
      ncalls < 0 || ncalls > DSX_MAX_AGGS)
    FAIL(-3, "groupby finish spec too large or without keys");
  int rc = gb_finish_calls_check(aggs, naggs, calls, ncalls);
  if (rc) return rc;
  GbFinishReq R{calls, ncalls, out_datas, out_valids};
  uint64_t* oc = nullptr;
  void* ov = nullptr;
  uint64_t* on = nullptr;
  return hash_groupby_impl(c, cols, ncols, n, keys, nkeys, pred, pred_len,
                           aggs, naggs, &oc, &ov, &on, out_groups, &R);
}

// every finish call names an accumulator whose op fits its kind
static int gb_finish_calls_check(const DsxAggSpec* aggs, int naggs,
                                 const DsxGbFinishCall* calls, int ncalls) {
  for (int i = 0; i < ncalls; i++) {
    int a = calls[i].agg;
    if (a < 0 || a >= naggs) FAIL(-3, "finish call names no accumulator");
    int want;
    switch (calls[i].kind) {
      case DSX_GBF_COUNT: want = -1; break;  // any accumulator has a count
      case DSX_GBF_SUM_I: want = DSX_AGG_SUM_I64; break;
      case DSX_GBF_SUM_F:
      case DSX_GBF_AVG: want = DSX_AGG_SUM_F64; break;
      case DSX_GBF_MIN_I: want = DSX_AGG_MIN_I64; break;
      case DSX_GBF_MAX_I: want = DSX_AGG_MAX_I64; break;
      case DSX_GBF_MIN_F: want = DSX_AGG_MIN_F64; break;
      case DSX_GBF_MAX_F: want = DSX_AGG_MAX_F64; break;
      default: FAIL(-3, "unknown finish kind %d", calls[i].kind);
    }
    if (want >= 0 && aggs[a].op != want)
      FAIL(-3, "finish kind %d does not fit accumulator op %d",
           calls[i].kind, aggs[a].op);
  }
  return 0;
}

// ---------------------------------------------------------------------------
// dsx_partition — stable bucket split for the RCCL shuffle
// ---------------------------------------------------------------------------
#define PART_SALT 0xA5A5A5A55A5A5A5Aull

__global__ void k_part_hist(const uint64_t* codes, const uint8_t* validity,
                            int64_t n, int nbuckets,
                            int64_t* hist /*[grid][nb]*/) {
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int64_t* s_hist = (int64_t*)smem;
  for (int i = threadIdx.x; i < nbuckets; i += BLOCK) s_hist[i] = 0;
  __syncthreads();
  for (int64_t r = lo + threadIdx.x; r < hi; r += BLOCK) {
    uint64_t cde = (validity && !validity[r]) ? 0 : codes[r];
    int b = (int)(mix64(cde ^ PART_SALT) % (uint64_t)nbuckets);
    atomicAdd((unsigned long long*)&s_hist[b], 1ull);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbuckets; i += BLOCK)
    hist[(int64_t)blockIdx.x * nbuckets + i] = s_hist[i];
}

// single block: column-major scan hist[grid][nb] → per-block per-bucket base
__global__ void k_part_scan(int64_t* hist, int grid, int nbuckets,
                            int64_t* bucket_offsets /*[nb+1]*/) {
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int b = 0; b < nbuckets; b++) {
      bucket_offsets[b] = run;
      for (int g = 0; g < grid; g++) {
        int64_t v = hist[(int64_t)g * nbuckets + b];
        hist[(int64_t)g * nbuckets + b] = run;
        run += v;
      }
    }
    bucket_offsets[nbuckets] = run;
  }
}

__global__ void k_part_scatter(const uint64_t* codes, const uint8_t* validity,
                               int64_t n, int nbuckets,
                               int64_t* hist /*[grid][nb] = running bases*/,
                               uint32_t* out_sel) {
  int64_t lo, hi;
  block_range(n, 1, lo, hi);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int64_t* s_base = (int64_t*)smem;            // [nb]
  int64_t* s_wave = s_base + nbuckets;         // [waves][nb]
  for (int i = threadIdx.x; i < nbuckets; i += BLOCK)
    s_base[i] = hist[(int64_t)blockIdx.x * nbuckets + i];
  __syncthreads();
  int wave = threadIdx.x / 64, lane = threadIdx.x & 63;
  for (int64_t base_r = lo; base_r < hi; base_r += BLOCK) {
    int64_t r = base_r + threadIdx.x;
    int b = -1;
    if (r < hi) {
      uint64_t cde = (validity && !validity[r]) ? 0 : codes[r];
      b = (int)(mix64(cde ^ PART_SALT) % (uint64_t)nbuckets);
    }
    // per-wave histogram + in-wave rank (stable: lanes ordered)
    int rank = 0;
    for (int k = 0; k < nbuckets; k++) {
      uint64_t m = __ballot(b == k);
      if (b == k) rank = __popcll(m & ((1ull << lane) - 1));
      if (lane == 0) s_wave[wave * nbuckets + k] = (int64_t)__popcll(m);
    }
    __syncthreads();
    if (b >= 0) {
      int64_t off = s_base[b];
      for (int w = 0; w < wave; w++) off += s_wave[w * nbuckets + b];
      out_sel[off + rank] = (uint32_t)r;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)nbuckets) {
      int64_t tot = 0;
      for (int w = 0; w < WAVES_PER_BLOCK; w++)
        tot += s_wave[w * nbuckets + threadIdx.x];
      s_base[threadIdx.x] += tot;
    }
    __syncthreads();
  }
}

extern "C" int dsx_partition(DsxCtx* c, const uint64_t* codes,
                             const uint8_t* validity, int64_t n, int nbuckets,
                             uint32_t* out_sel, int64_t* out_offsets) {
  if (nbuckets > BLOCK) FAIL(-3, "nbuckets > %d unsupported", BLOCK);
  if (n > 0xFFFFFFFFll) FAIL(-3, "partition too large for u32 row ids");
  int grid = (int)min((int64_t)MAX_GRID, (n + BLOCK - 1) / BLOCK);
  if (grid == 0) {
    for (int b = 0; b <= nbuckets; b++) out_offsets[b] = 0;
    return 0;
  }
  int64_t need = (int64_t)grid * nbuckets * 8 + (nbuckets + 1) * 8;
  int rc = ensure_scratch(c, need);
  if (rc) return rc;
  int64_t* d_hist = (int64_t*)c->scratch;
  int64_t* d_offsets = d_hist + (int64_t)grid * nbuckets;
  size_t lds1 = (size_t)nbuckets * 8;
  {
    ProfScope ps(c, "k_part_hist");
    hipLaunchKernelGGL(k_part_hist, dim3(grid), dim3(BLOCK), lds1, c->stream,
                       codes, validity, n, nbuckets, d_hist);
  }
  hipLaunchKernelGGL(k_part_scan, dim3(1), dim3(64), 0, c->stream, d_hist,
                     grid, nbuckets, d_offsets);
  size_t lds2 = (size_t)nbuckets * 8 * (1 + WAVES_PER_BLOCK);
  {
    ProfScope ps(c, "k_part_scatter");
    hipLaunchKernelGGL(k_part_scatter, dim3(grid), dim3(BLOCK), lds2,
                       c->stream, codes, validity, n, nbuckets, d_hist,
                       out_sel);
  }
  HIP_TRY(hipMemcpyAsync(out_offsets, d_offsets, (nbuckets + 1) * 8,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

void jit_cache_destroy(DsxCtx* c) {
  if (!c->jit_cache) return;
  for (auto& kv : ((JitCacheMap*)c->jit_cache)->m)
    if (kv.second.mod) hipModuleUnload(kv.second.mod);
  delete (JitCacheMap*)c->jit_cache;
  c->jit_cache = nullptr;
}

#include "radix_join.inc"
#include "sort.inc"
#include "radix_sort.inc"
#include "window.inc"
#include "window_rows.inc"
#include "window_range.inc"
#include "window_words.inc"
#include "topk.inc"
#include "group_join.inc"

// ---------------------------------------------------------------------------
// dsx_jit_expr_source — TEST INFRASTRUCTURE: emit the JIT expression
// evaluator's generated C for a program (the exact text the kernels
// compile via hipRTC) into buf, so the CPU differential suite can compile
// it with gcc and pin codegen semantics against the interpreter VM without
// a GPU. Host-only: no HIP calls. Returns 1 if the result kind is double,
// 0 for i64, <0 on error.
extern "C" int dsx_jit_expr_source(const DsxInstr* prog, int prog_len,
                                   const int32_t* dtypes,
                                   const uint8_t* has_validity, int ncols,
                                   char* buf, int64_t cap) {
  if (prog_len <= 0 || prog_len > DSX_MAX_PROG || ncols < 0 ||
      ncols > DSX_MAX_COLS)
    return -3;
  ColsArg C{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    C.dtype[i] = dtypes[i];
    C.validity[i] = has_validity[i] ? (const uint8_t*)1 : nullptr;
  }
  std::ostringstream os;
  char k = 'l';
  if (!jit_emit_fn(os, "j_expr", prog, prog_len, &C, &k)) return -1;
  std::string src = os.str();
  if ((int64_t)src.size() + 1 > cap) return -2;
  memcpy(buf, src.c_str(), src.size() + 1);
  return k == 'd' ? 1 : 0;
}

// dsx_jit_pack_source — TEST INFRASTRUCTURE (like dsx_jit_expr_source):
// emit the JIT key-pack source for a key spec so CPU tests can gcc-compile
// it and differential-test it against the pack_key spec. Host-only.
// Returns 0, or <0 on error.
extern "C" int dsx_jit_pack_source(const DsxKeySpec* keys, int nkeys,
                                   const int32_t* dtypes,
                                   const uint8_t* has_validity, int ncols,
                                   char* buf, int64_t cap) {
  if (nkeys <= 0 || nkeys > DSX_MAX_KEYS || ncols < 0 ||
      ncols > DSX_MAX_COLS)
    return -3;
  KeyArg K{};
  K.nkeys = nkeys;
  for (int j = 0; j < nkeys; j++) K.k[j] = keys[j];
  ColsArg C{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    C.dtype[i] = dtypes[i];
    C.validity[i] = has_validity[i] ? (const uint8_t*)1 : nullptr;
  }
  std::ostringstream os;
  jit_emit_pack(os, K, &C);
  std::string src = os.str();
  if ((int64_t)src.size() + 1 > cap) return -2;
  memcpy(buf, src.c_str(), src.size() + 1);
  return 0;
}

// dsx_jit_fprobe_source — TEST INFRASTRUCTURE (like dsx_jit_expr_source):
// the generated filter-probe mask kernel's full source for a shape, exactly
// the text dsx_filter_probe_cols compiles. Only the PRESENCE of validity
// buffers enters; pointers, n and the table mask are kernel arguments.
// words <= 0 selects the shipped value. Host-only: no HIP calls.
// Returns 0; -1 when the generator rejects the predicate (the caller's
// interpreter fallback), -2 when buf is too small, -3 on a malformed spec.
// dsx_jit_fprobe_source_mode is the same for a table with a key-membership
// filter of mode jf_mode (join_filter.h); mode 0 is dsx_jit_fprobe_source.
// The filter's pointer, size and cap never enter the text.
extern "C" int dsx_jit_fprobe_source_mode(const DsxInstr* prog, int prog_len,
                                          const DsxKeySpec* keys, int nkeys,
                                          const int32_t* dtypes,
                                          const uint8_t* has_validity,
                                          int ncols, int packed, int words,
                                          int jf_mode, char* buf,
                                          int64_t cap) {
  if (prog_len < 0 || prog_len > DSX_MAX_PROG || nkeys <= 0 ||
      nkeys > DSX_MAX_KEYS || ncols < 0 || ncols > DSX_MAX_COLS || words > 8 ||
      jf_mode < DSX_JF_NONE || jf_mode > DSX_JF_HASHED)
    return -3;
  ProgArg P{};
  memcpy(P.ins, prog, prog_len * sizeof(DsxInstr));
  P.len = prog_len;
  KeyArg K{};
  if (make_keyarg(keys, nkeys, K)) return -3;
  for (int j = 0; j < nkeys; j++)
    if (keys[j].mode != 0 || keys[j].col < 0 || keys[j].col >= ncols)
      return -3;
  ColsArg C{};
  C.ncols = ncols;
  for (int i = 0; i < ncols; i++) {
    C.dtype[i] = dtypes[i];
    C.validity[i] = has_validity[i] ? (const uint8_t*)1 : nullptr;
  }
  std::string src =
      jit_fprobe_source(C, K, P, packed != 0,
                        words <= 0 ? DSX_FPROBE_JIT_WORDS : words, jf_mode);
  if (src.empty()) return -1;
  if ((int64_t)src.size() + 1 > cap) return -2;
  memcpy(buf, src.c_str(), src.size() + 1);
  return 0;
}

extern "C" int dsx_jit_fprobe_source(const DsxInstr* prog, int prog_len,
                                     const DsxKeySpec* keys, int nkeys,
                                     const int32_t* dtypes,
                                     const uint8_t* has_validity, int ncols,
                                     int packed, int words, char* buf,
                                     int64_t cap) {
  return dsx_jit_fprobe_source_mode(prog, prog_len, keys, nkeys, dtypes,
                                    has_validity, ncols, packed, words,
                                    DSX_JF_NONE, buf, cap);
}

// dsx_jit_compile_check — TEST INFRASTRUCTURE: hipRTC-compile a generated
// source for gfx950 with the options the runtime uses. Needs no GPU (nothing
// is loaded). Returns 0, or 1 with the compiler log on stderr.
extern "C" int dsx_jit_compile_check(const char* src) {
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src, "dsx_check.cu", 0, nullptr, nullptr) !=
      HIPRTC_SUCCESS)
    return 1;
  const char* opts[] = {"-O3", "--offload-arch=gfx950", "-std=c++17",
                        "-munsafe-fp-atomics"};
  hiprtcResult rc = hiprtcCompileProgram(prog, 4, opts);
  if (rc != HIPRTC_SUCCESS) {
    size_t lsz = 0;
    hiprtcGetProgramLogSize(prog, &lsz);
    std::string log(lsz, '\0');
    if (lsz) hiprtcGetProgramLog(prog, &log[0]);
    fprintf(stderr, "[dsxhip] JIT compile check FAILED:\n%s\n", log.c_str());
  }
  hiprtcDestroyProgram(&prog);
  return rc == HIPRTC_SUCCESS ? 0 : 1;
}

// dsx_jit_fprobe_selftest — compile-check the generated filter-probe kernel
// for the Q3 probe shapes (i32 date vs constant, one i64 key, packed) and an
// unpacked composite with a nullable key, at R = 1, 2, 4 and 8, WITHOUT a GPU
// (like dsx_jit_selftest). Returns 0, or 100·(shape + 1) + R of the first
// failure.
extern "C" int dsx_jit_fprobe_selftest(void) {
  DsxInstr pred[3] = {{DSX_OP_COL, 0, 0}, {DSX_OP_LIT_I64, 0, 9204},
                      {DSX_OP_GT_I64, 0, 0}};
  for (int shape = 0; shape < 2; shape++) {
    int32_t dtypes[3] = {DSX_I32, DSX_I64, DSX_I32};
    uint8_t hv[3] = {0, 0, (uint8_t)shape};
    DsxKeySpec keys[2]{};
    keys[0].col = 1;
    keys[0].range = shape ? (int64_t)1 << 40 : 60'000'000;
    keys[1].col = 2;
    keys[1].range = 1000;
    keys[1].nullable = 1;
    static char buf[1 << 17];
    for (int R : {1, 2, 4, 8}) {
      int rc = dsx_jit_fprobe_source(pred, 3, keys, shape ? 2 : 1, dtypes, hv,
                                     3, shape ? 0 : 1, R, buf, sizeof buf);
      if (rc || dsx_jit_compile_check(buf)) return 100 * (shape + 1) + R;
    }
  }
  return 0;
}

// dsx_jit_selftest — hiprtc-compile a representative C2-shaped partition
// groupby source (incl. j_scatter_staged) WITHOUT a GPU. Test harness only:
// catches JIT codegen syntax breakage in the CPU container instead of a
// silent interpreter fallback on the GPU box.
// ---------------------------------------------------------------------------
extern "C" int dsx_jit_selftest(void) {
  ColsArg C{};
  C.ncols = 2;
  C.dtype[0] = DSX_I64;  // key
  C.dtype[1] = DSX_F64;  // x
  KeyArg K{};
  K.nkeys = 1;
  K.k[0].col = 0;
  K.k[0].min = 0;
  K.k[0].range = 1'000'000;
  K.stride[0] = 1;
  ProgArg P{};  // x < 0.5
  P.ins[0] = {DSX_OP_COL, 1, 0};
  P.ins[1] = {DSX_OP_LIT_F64, 0, (int64_t)0};
  {
    double half = 0.5;
    memcpy(&P.ins[1].imm, &half, 8);
  }
  P.ins[2] = {DSX_OP_LT_F64, 0, 0};
  P.len = 3;
  DsxAggSpec aggs[2]{};
  aggs[0].op = DSX_AGG_SUM_F64;
  aggs[0].prog_len = 1;
  aggs[0].prog[0] = {DSX_OP_COL, 1, 0};
  aggs[1].op = DSX_AGG_COUNT;
  aggs[1].prog_len = 1;
  aggs[1].prog[0] = {DSX_OP_LIT_I64, 0, 1};
  AggArg A{};
  A.naggs = 2;
  A.op[0] = DSX_AGG_SUM_F64;
  A.op[1] = DSX_AGG_COUNT;
  A.never_null[0] = A.never_null[1] = 1;
  int32_t val_of[2] = {0, -1};
  ProgArg P0{};  // predicate-free shape: the contiguous aggregate variant
  for (int tile : {0, 4096}) {
    for (int code32 : {0, 1}) {
     for (int ds : {-1, 11}) {
      for (int pf : {0, 1}) {
      std::string src = jit_gbpart_source(C, K, pf ? P0 : P, aggs, A,
                                          val_of, 2, 1,
                                          ds >= 0 ? (1 << ds) : 2048,
                                          code32 != 0, tile, ds);
      if (src.empty()) {
        fprintf(stderr, "[selftest] empty source (tile=%d code32=%d)\n",
                tile, code32);
        return 1;
      }
      hiprtcProgram prog;
      if (hiprtcCreateProgram(&prog, src.c_str(), "dsx_selftest.cu", 0,
                              nullptr, nullptr) != HIPRTC_SUCCESS)
        return 2;
      const char* opts[] = {"-O3", "--offload-arch=gfx950", "-std=c++17",
                            "-munsafe-fp-atomics"};
      hiprtcResult rc = hiprtcCompileProgram(prog, 4, opts);
      if (rc != HIPRTC_SUCCESS) {
        size_t lsz = 0;
        hiprtcGetProgramLogSize(prog, &lsz);
        std::string log(lsz, '\0');
        if (lsz) hiprtcGetProgramLog(prog, &log[0]);
        fprintf(stderr,
                "[selftest] JIT compile FAILED (tile=%d code32=%d ds=%d):"
                "\n%s\n", tile, code32, ds, log.c_str());
        hiprtcDestroyProgram(&prog);
        return 3;
      }
      hiprtcDestroyProgram(&prog);
      }
     }
    }
  }
  // radix-join JIT shapes (C3 inner; LEFT with nullable build payload)
  for (int jt : {DSX_JOIN_INNER, DSX_JOIN_LEFT, DSX_JOIN_LEFTANTI}) {
    ColsArg CB2{}, CP2{};
    CB2.ncols = 2;
    CB2.dtype[0] = DSX_I64;
    CB2.dtype[1] = DSX_F64;
    CB2.validity[1] = (const uint8_t*)1;  // metadata-only probe
    CP2.ncols = 2;
    CP2.dtype[0] = DSX_I64;
    CP2.dtype[1] = DSX_F64;
    KeyArg KB2{}, KP2{};
    KB2.nkeys = KP2.nkeys = 1;
    KB2.k[0].col = KP2.k[0].col = 0;
    KB2.k[0].range = KP2.k[0].range = 10'000'000;
    KB2.stride[0] = KP2.stride[0] = 1;
    DsxInstr bp2[2] = {{DSX_OP_COL, 0, 0}, {DSX_OP_IS_NOT_NULL, 0, 0}};
    int32_t bpay[1] = {1}, ppay[2] = {0, 1};
    int32_t oside[3] = {0, 0, 1}, oslot2[3] = {0, 1, 0};
    int32_t odt[3] = {DSX_I64, DSX_F64, DSX_F64};
    int32_t onv[3] = {0, 0, jt == DSX_JOIN_LEFT ? 1 : 0};
    std::string src = jit_radix_source(CB2, KB2, bp2, 2, bpay, 1, 1, CP2,
                                       KP2, ppay, 2, 0, 8192, jt, oside,
                                       oslot2, odt, onv, 3);
    if (const char* dump = getenv("DSX_JIT_DUMP")) {
      char fn[512];
      snprintf(fn, sizeof fn, "%s/selftest_rj_%d.cu", dump, jt);
      FILE* f = fopen(fn, "w");
      if (f) { fwrite(src.data(), 1, src.size(), f); fclose(f); }
    }
    if (src.empty()) {
      fprintf(stderr, "[selftest] empty radix source (jt=%d)\n", jt);
      return 4;
    }
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "dsx_rj.cu", 0, nullptr,
                            nullptr) != HIPRTC_SUCCESS)
      return 4;
    const char* opts[] = {"-O3", "--offload-arch=gfx950", "-std=c++17",
                          "-munsafe-fp-atomics"};
    if (hiprtcCompileProgram(prog, 4, opts) != HIPRTC_SUCCESS) {
      size_t lsz = 0;
      hiprtcGetProgramLogSize(prog, &lsz);
      std::string log(lsz, '\0');
      if (lsz) hiprtcGetProgramLog(prog, &log[0]);
      fprintf(stderr, "[selftest] radix JIT FAILED (jt=%d):\n%s\n", jt,
              log.c_str());
      hiprtcDestroyProgram(&prog);
      return 5;
    }
    hiprtcDestroyProgram(&prog);
  }
  return 0;
}
