// jit_kernels.inc — kernel-source builders + launchers for the JIT'd
// groupby paths (see jit.inc header comment). Included by dsxhip.hip.

// agg update line for the DIRECT (LDS) kernel, fully inlined per agg
static void jit_emit_direct_agg(std::ostringstream& os, int a, int op,
                                int never_null, int key_space, char kind) {
  std::string idx = "(" + std::to_string(a) + " * " +
                    std::to_string(key_space) + " + k)";
  os << "    { ";
  if (op == DSX_AGG_COUNT) {
    if (!never_null)
      os << "i64 v; bool ok = eval_agg" << a << "(C, r, v); (void)v; "
         << "if (ok) atomicAdd(&s_cnts[" << idx << "], 1u);";
    // never-null COUNT: derived from gcnt, nothing per-row
  } else {
    const char* ty = kind == 'd' ? "double" : "i64";
    os << ty << " v; bool ok = eval_agg" << a << "(C, r, v); if (ok) {\n      ";
    switch (op) {
      case DSX_AGG_SUM_F64:
        os << "atomicAdd((double*)&s_vals[" << idx << "], (double)v);";
        break;
      case DSX_AGG_SUM_I64:
        os << "atomicAdd((u64*)&s_vals[" << idx << "], (u64)(i64)v);";
        break;
      case DSX_AGG_MIN_F64:
        os << "atomicMin((u64*)&s_vals[" << idx
           << "], f64_ordered((double)v));";
        break;
      case DSX_AGG_MAX_F64:
        os << "atomicMax((u64*)&s_vals[" << idx
           << "], f64_ordered((double)v));";
        break;
      case DSX_AGG_MIN_I64:
        os << "atomicMin((u64*)&s_vals[" << idx << "], i64_ordered((i64)v));";
        break;
      case DSX_AGG_MAX_I64:
        os << "atomicMax((u64*)&s_vals[" << idx << "], i64_ordered((i64)v));";
        break;
    }
    if (!never_null)
      os << "\n      atomicAdd(&s_cnts[" << idx << "], 1u);";
    os << "\n    }";
  }
  os << " }\n";
}

// builds j_hist + j_scatter + j_aggregate for the partition path;
// "" on unsupported shape. code32: the packed key space fits u32, so
// records are SoA (u32 codes + u64 vals) — 12 B/row instead of 16 on the
// scatter write and aggregate read (the partition path's own traffic).
static std::string jit_gbpart_source(const ColsArg& C, const KeyArg& K,
                                     const ProgArg& P, const DsxAggSpec* aggs,
                                     const AggArg& A, const int32_t* val_of,
                                     int naggs, int nvals, int lds_slots,
                                     bool code32, int tile,
                                     int direct_shift) {
  std::ostringstream os;
  os << JIT_PRELUDE;
  char k;
  if (!jit_emit_fn(os, "eval_pred", P.ins, P.len, &C, &k)) return "";
  std::vector<char> kinds(naggs, 'l');
  for (int a = 0; a < naggs; a++) {
    if (val_of[a] < 0) continue;  // COUNT: no stored value
    char name[32];
    snprintf(name, sizeof name, "eval_agg%d", a);
    if (!jit_emit_fn(os, name, aggs[a].prog, aggs[a].prog_len, &C,
                     &kinds[a]))
      return "";
  }
  jit_emit_pack(os, K, &C);
  int rec = 1 + nvals;
  // direct_shift >= 0: RANGE bucketing (bucket = code >> shift) so the
  // aggregate can DIRECT-INDEX its LDS slots (no hash table, no CAS probe
  // loop, no key storage — keys reconstruct as bucket<<shift | slot).
  // Balance-guarded by the host (skewed distributions fall back to hash).
  if (direct_shift >= 0)
    os << "#define GB_BUCKET(code, nbm) ((int)((code) >> " << direct_shift
       << "))\n";
  else
    os << "#define GB_BUCKET(code, nbm) gb_bucket((code), (nbm))\n";
  // nontemporal record stores (measurable knob; records are consumed once
  // by j_aggregate, so L2 residency buys nothing and eviction write
  // amplification may cost)
  static const bool nt = getenv("DSX_SCATTER_NT") != nullptr;
  auto store = [](const char* ptr, const char* val) {
    if (getenv("DSX_SCATTER_NT"))
      return std::string("__builtin_nontemporal_store(") + val + ", &" +
             ptr + ");";
    return std::string(ptr) + " = " + val + ";";
  };
  (void)nt;
  os << R"(
extern "C" __global__ void j_hist(ColsArg C, i64 n, int nb, i64* hist) {
  extern __shared__ char smem[];
  u32* s_hist = (u32*)smem;
  for (int i = threadIdx.x; i < nb; i += BLOCK) s_hist[i] = 0;
  __syncthreads();
  i64 lo, hi; block_range(n, 1, lo, hi);
  // NO predicate here: the histogram is a pure function of the key column,
  // so the host caches (hist, bases) per table and steps 2+ skip this pass
  // entirely; the scatter publishes per-segment SELECTED counts instead
  for (i64 r = lo + threadIdx.x; r < hi; r += BLOCK) {
    atomicAdd(&s_hist[GB_BUCKET(jit_pack(C, r), nb - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += BLOCK)
    hist[(i64)blockIdx.x * nb + i] = (i64)s_hist[i];
}
)";
  if (code32)
    os << "extern \"C\" __global__ void j_scatter(ColsArg C, i64 n, int nb,\n"
          "    const i64* hist, const i64* bases, u32* selcnt,\n"
          "    u32* out_code, u64* out_val) {\n";
  else
    os << "extern \"C\" __global__ void j_scatter(ColsArg C, i64 n, int nb,\n"
          "    const i64* hist, const i64* bases, u32* selcnt,\n"
          "    u64* out_rec) {\n";
  os << R"(  extern __shared__ char smem[];
  i64* s_off = (i64*)smem;
  for (int i = threadIdx.x; i < nb; i += blockDim.x)
    s_off[i] = bases[i] + hist[(i64)blockIdx.x * nb + i];
  __syncthreads();
  i64 lo, hi; block_range(n, 1, lo, hi);
  for (i64 r = lo + threadIdx.x; r < hi; r += blockDim.x) {
    i64 pv; if (!(eval_pred(C, r, pv) && pv)) continue;
    u64 code = jit_pack(C, r);
    int b = GB_BUCKET(code, nb - 1);
    i64 o = (i64)atomicAdd((u64*)&s_off[b], 1ull);
)";
  if (code32) {
    os << "    " << store("out_code[o]", "(u32)code") << "\n";
    for (int a = 0; a < naggs; a++) {
      if (val_of[a] < 0) continue;
      std::string dst = nvals == 1
          ? "out_val[o]"
          : ("out_val[o * " + std::to_string(nvals) + " + " +
             std::to_string(val_of[a]) + "]");
      if (kinds[a] == 'd')
        os << "    { double v; eval_agg" << a << "(C, r, v); "
           << store(dst.c_str(), "(u64)__double_as_longlong(v)") << " }\n";
      else
        os << "    { i64 v; eval_agg" << a << "(C, r, v); "
           << store(dst.c_str(), "(u64)v") << " }\n";
    }
  } else if (rec == 2 && !getenv("DSX_SCATTER_NOVEC")) {
    // one 16-B store per record (explicit ulonglong2 — the separate 8-B
    // code/value stores rely on the backend merging them)
    int a0 = 0;
    while (a0 < naggs && val_of[a0] < 0) a0++;
    os << "    ulonglong2 rv2;\n    rv2.x = code;\n";
    if (kinds[a0] == 'd')
      os << "    { double v; eval_agg" << a0
         << "(C, r, v); rv2.y = (u64)__double_as_longlong(v); }\n";
    else
      os << "    { i64 v; eval_agg" << a0 << "(C, r, v); rv2.y = (u64)v; }\n";
    os << "    ((ulonglong2*)out_rec)[o] = rv2;\n";
  } else {
    os << "    u64* dst = out_rec + o * " << rec << ";\n"
       << "    " << store("dst[0]", "code") << "\n";
    for (int a = 0; a < naggs; a++) {
      if (val_of[a] < 0) continue;
      std::string dst = "dst[1 + " + std::to_string(val_of[a]) + "]";
      if (kinds[a] == 'd')
        os << "    { double v; eval_agg" << a << "(C, r, v); "
           << store(dst.c_str(), "(u64)__double_as_longlong(v)") << " }\n";
      else
        os << "    { i64 v; eval_agg" << a << "(C, r, v); "
           << store(dst.c_str(), "(u64)v") << " }\n";
    }
  }
  os << "  }\n"
        "  __syncthreads();\n"
        "  for (int i = threadIdx.x; i < nb; i += blockDim.x)\n"
        "    selcnt[(i64)blockIdx.x * nb + i] =\n"
        "        (u32)(s_off[i] - bases[i] - hist[(i64)blockIdx.x * nb + i]);"
        "\n}\n";

  // j_scatter_staged — the record-batched variant (VERDICT r1 #2): the
  // plain scatter's 16-B appends touch one 64-B line EACH and the line is
  // re-opened much later for its neighbors (write amplification ≈2×,
  // line touches dominate — the measured SoA regression proved bytes
  // don't). Here each block processes its range in LDS tiles: count
  // buckets, scan, place records bucket-sorted in LDS, then flush with
  // CONSECUTIVE threads writing CONSECUTIVE records of the same bucket —
  // full-line bursts, and successive tiles continue each bucket run while
  // its tail line is still L2-hot.
  if (tile > 0) {
    os << "#define JT " << tile << "\n";
    if (code32)
      os << "extern \"C\" __global__ void j_scatter_staged(ColsArg C, i64 n,"
            " int nb,\n    const i64* hist, const i64* bases, u32* selcnt,"
            " u32* out_code, u64* out_val) {\n";
    else
      os << "extern \"C\" __global__ void j_scatter_staged(ColsArg C, i64 n,"
            " int nb,\n    const i64* hist, const i64* bases, u32* selcnt,"
            " u64* out_rec) {\n";
    os << R"(  extern __shared__ char smem[];
  i64* s_off = (i64*)smem;                 // [nb] absolute dest per bucket
  u32* t_cnt = (u32*)(s_off + nb);         // [nb] tile counts / run ctr
  u32* t_base = t_cnt + nb;                // [nb+1] tile-local bases
  unsigned short* s_bk = (unsigned short*)(t_base + nb + 1);  // [JT]
  u64* stage = (u64*)(((size_t)(s_bk + JT) + 15) & ~(size_t)15);
  for (int i = threadIdx.x; i < nb; i += blockDim.x)
    s_off[i] = bases[i] + hist[(i64)blockIdx.x * nb + i];
  i64 lo, hi; block_range(n, 1, lo, hi);
  for (i64 t0 = lo; t0 < hi; t0 += JT) {
    i64 t1 = t0 + JT < hi ? t0 + JT : hi;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) t_cnt[i] = 0;
    __syncthreads();
    for (i64 r = t0 + threadIdx.x; r < t1; r += blockDim.x) {
      i64 pv; if (!(eval_pred(C, r, pv) && pv)) continue;
      atomicAdd(&t_cnt[GB_BUCKET(jit_pack(C, r), nb - 1)], 1u);
    }
    __syncthreads();
    {  // exclusive scan of t_cnt into t_base (nb <= blockDim, host-checked)
      int i = threadIdx.x;
      u32 cnt = (i < nb) ? t_cnt[i] : 0;
      if (i < nb) t_base[i] = cnt;
      __syncthreads();
      for (int d = 1; d < nb; d <<= 1) {
        u32 add = (i >= d && i < nb) ? t_base[i - d] : 0;
        __syncthreads();
        if (i < nb) t_base[i] += add;
        __syncthreads();
      }
      u32 incl = (i < nb) ? t_base[i] : 0;
      __syncthreads();
      if (i < nb) { t_base[i] = incl - cnt; t_cnt[i] = 0; }
      if (i == nb - 1) t_base[nb] = incl;
      __syncthreads();
    }
    for (i64 r = t0 + threadIdx.x; r < t1; r += blockDim.x) {
      i64 pv; if (!(eval_pred(C, r, pv) && pv)) continue;
      u64 code = jit_pack(C, r);
      int b = GB_BUCKET(code, nb - 1);
      u32 pos = t_base[b] + atomicAdd(&t_cnt[b], 1u);
      s_bk[pos] = (unsigned short)b;
)";
    // staged records are AoS in LDS either way; the code32 flush splits
    // them SoA to global
    os << "      u64* sd = stage + (i64)pos * " << rec << ";\n"
       << "      sd[0] = code;\n";
    for (int a = 0; a < naggs; a++) {
      if (val_of[a] < 0) continue;
      std::string dst = "sd[1 + " + std::to_string(val_of[a]) + "]";
      if (kinds[a] == 'd')
        os << "      { double v; eval_agg" << a << "(C, r, v); " << dst
           << " = (u64)__double_as_longlong(v); }\n";
      else
        os << "      { i64 v; eval_agg" << a << "(C, r, v); " << dst
           << " = (u64)v; }\n";
    }
    os << R"(    }
    __syncthreads();
    u32 total = t_base[nb];
    for (u32 i = threadIdx.x; i < total; i += blockDim.x) {
      int b = (int)s_bk[i];
      i64 o = s_off[b] + (i64)(i - t_base[b]);
)";
    // flush stores are nontemporal: records are consumed once by
    // j_aggregate (0.8 GB never fits L2) and keeping them OUT of L2
    // preserves the tile's phase-3 re-read hits (PMC: +64% fetch without)
    if (code32) {
      os << "      const u64* src = stage + (i64)i * " << rec << ";\n"
         << "      __builtin_nontemporal_store((u32)src[0], &out_code[o]);\n";
      if (nvals == 1)
        os << "      __builtin_nontemporal_store(src[1], &out_val[o]);\n";
      else
        for (int v = 0; v < nvals; v++)
          os << "      __builtin_nontemporal_store(src[" << (1 + v)
             << "], &out_val[o * " << nvals << " + " << v << "]);\n";
    } else if (rec == 2) {
      os << "      __builtin_nontemporal_store("
            "((const __uint128_t*)stage)[i],"
            " &((__uint128_t*)out_rec)[o]);\n";
    } else {
      os << "      u64* dst = out_rec + o * " << rec << ";\n"
         << "      const u64* src = stage + (i64)i * " << rec << ";\n";
      for (int j = 0; j < rec; j++)
        os << "      __builtin_nontemporal_store(src[" << j << "], &dst["
           << j << "]);\n";
    }
    os << R"(    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += blockDim.x) s_off[i] += t_cnt[i];
    __syncthreads();
  }
  for (int i = threadIdx.x; i < nb; i += blockDim.x)
    selcnt[(i64)blockIdx.x * nb + i] =
        (u32)(s_off[i] - bases[i] - hist[(i64)blockIdx.x * nb + i]);
}
)";
  }

  // j_aggregate: the per-bucket LDS aggregation with ops/layout inlined
  int SLOTS = lds_slots, NV = nvals ? nvals : 0;
  static const int AB = [] {
    const char* e = getenv("DSX_AGG_THREADS");
    return e ? atoi(e) : 1024;
  }();
  if (direct_shift >= 0) {
    // DIRECT-INDEX aggregate: bucket = code >> shift, slot = code & mask.
    // No hash table, no CAS loop, no key storage; keys reconstruct as
    // (bucket << shift) | slot. SLOTS here = 1 << direct_shift.
    int DS = 1 << direct_shift;
    os << "#undef BLOCK\n#define BLOCK " << AB << "\n"
       << "extern \"C\" __global__ void __launch_bounds__(BLOCK) "
          "j_aggregate(\n";
    if (code32)
      os << "    const u32* r_codes, const u64* r_vals, const i64* bases,\n"
         << "    const i64* hist, const u32* selcnt, int sgrid,\n"
         << "    u64* g_counter,\n";
    else
      os << "    const u64* recs, const i64* bases, const i64* hist,\n"
         << "    const u32* selcnt, int sgrid, u64* g_counter,\n";
    os << "    u64* tmp_codes, u64* tmp_vals, u64* tmp_gcnt, int* overflow)"
          " {\n"
       << "  extern __shared__ char smem[];\n"
       << "  u64* l_vals = (u64*)smem;\n"
       << "  u32* l_gcnt = (u32*)(l_vals + " << DS * NV << ");\n"
       << "  for (int i = threadIdx.x; i < " << DS
       << "; i += BLOCK) l_gcnt[i] = 0;\n";
    {
      int vs = 0;
      for (int a = 0; a < naggs; a++) {
        if (val_of[a] < 0) continue;
        os << "  for (int i = threadIdx.x; i < " << DS
           << "; i += BLOCK) l_vals[i * " << NV << " + " << vs << "] = "
           << agg_identity(A.op[a]) << "ull;\n";
        vs++;
      }
    }
    os << "  __syncthreads();\n";
    if (P.len == 0) {
      // no predicate → selected == counted: the bucket's records are one
      // CONTIGUOUS run, no segment walk needed
      os << "  {\n  {\n"
         << "  i64 st = bases[blockIdx.x];\n"
         << "  i64 en = bases[blockIdx.x + 1];\n"
         << "  for (i64 r = st + threadIdx.x; r < en; r += BLOCK) {\n";
    } else {
      // one WAVE per segment (block-sequential segments serialized the
      // two per-segment loads: 2048 segments x ~0.5 us = +1 ms measured)
      os << "  i64 rbase = bases[blockIdx.x];\n"
       << "  {\n"
       << "  int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;\n"
       << "  int nw = BLOCK >> 6;\n"
       << "  for (int sg = wid; sg < sgrid; sg += nw) {\n"
       << "   i64 st = rbase + hist[(i64)sg * gridDim.x + blockIdx.x];\n"
       << "   i64 en = st + (i64)selcnt[(i64)sg * gridDim.x +"
          " blockIdx.x];\n"
       << "   for (i64 r = st + lane; r < en; r += 64) {\n";
    }
    if (code32)
      os << "    u64 code = (u64)r_codes[r];\n";
    else if (rec == 2)
      os << "    ulonglong2 rv = ((const ulonglong2*)recs)[r];\n"
         << "    u64 code = rv.x;\n";
    else
      os << "    const u64* src = recs + r * " << rec << ";\n"
         << "    u64 code = src[0];\n";
    os << "    int s = (int)(code & " << (DS - 1) << "u);\n"
       << "    atomicAdd(&l_gcnt[s], 1u);\n";
    {
      int vs = 0;
      for (int a = 0; a < naggs; a++) {
        if (val_of[a] < 0) continue;
        std::string raw =
            code32 ? (NV == 1 ? std::string("r_vals[r]")
                              : ("r_vals[r * " + std::to_string(NV) + " + " +
                                 std::to_string(vs) + "]"))
            : (rec == 2) ? std::string("rv.y")
                         : ("src[1 + " + std::to_string(vs) + "]");
        std::string dst = "l_vals[s * " + std::to_string(NV) + " + " +
                          std::to_string(vs) + "]";
        switch (A.op[a]) {
          case DSX_AGG_SUM_F64:
            os << "    atomicAdd((double*)&" << dst
               << ", __longlong_as_double((i64)" << raw << "));\n";
            break;
          case DSX_AGG_SUM_I64:
            os << "    atomicAdd((u64*)&" << dst << ", " << raw << ");\n";
            break;
          case DSX_AGG_MIN_F64:
            os << "    atomicMin((u64*)&" << dst
               << ", f64_ordered(__longlong_as_double((i64)" << raw
               << ")));\n";
            break;
          case DSX_AGG_MAX_F64:
            os << "    atomicMax((u64*)&" << dst
               << ", f64_ordered(__longlong_as_double((i64)" << raw
               << ")));\n";
            break;
          case DSX_AGG_MIN_I64:
            os << "    atomicMin((u64*)&" << dst << ", i64_ordered((i64)"
               << raw << "));\n";
            break;
          case DSX_AGG_MAX_I64:
            os << "    atomicMax((u64*)&" << dst << ", i64_ordered((i64)"
               << raw << "));\n";
            break;
        }
        vs++;
      }
    }
    os << "   }\n  }\n  }\n  __syncthreads();\n"
       << "  __shared__ u64 s_base;\n"
       << "  __shared__ unsigned int s_local;\n"
       << "  __shared__ unsigned int s_scan[BLOCK];\n"
       << "  unsigned int my_count = 0;\n"
       << "  for (int i = threadIdx.x; i < " << DS << "; i += BLOCK)\n"
       << "    if (l_gcnt[i]) my_count++;\n"
       << "  s_scan[threadIdx.x] = my_count;\n  __syncthreads();\n"
       << "  for (int d = 1; d < BLOCK; d <<= 1) {\n"
       << "    unsigned int v = (threadIdx.x >= d) ?"
          " s_scan[threadIdx.x - d] : 0;\n"
       << "    __syncthreads();\n    s_scan[threadIdx.x] += v;\n"
       << "    __syncthreads();\n  }\n"
       << "  unsigned int my_excl = s_scan[threadIdx.x] - my_count;\n"
       << "  if (threadIdx.x == BLOCK - 1) {\n"
       << "    unsigned int tot = s_scan[BLOCK - 1];\n"
       << "    s_base = tot ? atomicAdd(g_counter, (u64)tot) : 0;\n"
       << "    s_local = tot;\n  }\n  __syncthreads();\n"
       << "  if (s_local == 0) return;\n"
       << "  u64 base = s_base;\n"
       << "  unsigned int o = my_excl;\n"
       << "  for (int i = threadIdx.x; i < " << DS << "; i += BLOCK) {\n"
       << "    if (!l_gcnt[i]) continue;\n"
       << "    i64 dsti = (i64)(base + o);\n"
       << "    tmp_codes[dsti] = ((u64)blockIdx.x << " << direct_shift
       << ") | (u64)i;\n"
       << "    tmp_gcnt[dsti] = (u64)l_gcnt[i];\n";
    for (int v = 0; v < NV; v++)
      os << "    tmp_vals[dsti * " << NV << " + " << v << "] = l_vals[i * "
         << NV << " + " << v << "];\n";
    os << "    o++;\n  }\n}\n";
    return os.str();
  }
  os << "#undef BLOCK\n#define BLOCK " << AB << "\n"
     << "extern \"C\" __global__ void __launch_bounds__(BLOCK) j_aggregate(\n";
  if (code32)
    os << "    const u32* r_codes, const u64* r_vals, const i64* bases,\n"
       << "    const i64* hist, const u32* selcnt, int sgrid,\n"
       << "    u64* g_counter,\n";
  else
    os << "    const u64* recs, const i64* bases, const i64* hist,\n"
       << "    const u32* selcnt, int sgrid, u64* g_counter,\n";
  os << "    u64* tmp_codes, u64* tmp_vals, u64* tmp_gcnt, int* overflow) {\n"
     << "  extern __shared__ char smem[];\n"
     << "  u64* l_keys = (u64*)smem;\n"
     << "  u64* l_vals = l_keys + " << SLOTS << ";\n"
     << "  u32* l_gcnt = (u32*)(l_vals + " << SLOTS * NV << ");\n"
     << "  for (int i = threadIdx.x; i < " << SLOTS << "; i += BLOCK) {\n"
     << "    l_keys[i] = ~0ull; l_gcnt[i] = 0;\n  }\n";
  {
    int vs = 0;
    for (int a = 0; a < naggs; a++) {
      if (val_of[a] < 0) continue;
      os << "  for (int i = threadIdx.x; i < " << SLOTS
         << "; i += BLOCK) l_vals[i * " << NV << " + " << vs << "] = "
         << agg_identity(A.op[a]) << "ull;\n";
      vs++;
    }
  }
  os << "  __syncthreads();\n";
  if (P.len == 0) {
    os << "  {\n  {\n"
       << "  i64 st = bases[blockIdx.x];\n"
       << "  i64 en = bases[blockIdx.x + 1];\n"
       << "  for (i64 r = st + threadIdx.x; r < en; r += BLOCK) {\n";
  } else {
    os << "  i64 rbase = bases[blockIdx.x];\n"
     << "  {\n"
     << "  int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;\n"
     << "  int nw = BLOCK >> 6;\n"
     << "  for (int sg = wid; sg < sgrid; sg += nw) {\n"
     << "   i64 st = rbase + hist[(i64)sg * gridDim.x + blockIdx.x];\n"
     << "   i64 en = st + (i64)selcnt[(i64)sg * gridDim.x + blockIdx.x];\n"
     << "   for (i64 r = st + lane; r < en; r += 64) {\n";
  }
  if (code32) {
    os << "    u64 code = (u64)r_codes[r];\n";
  } else if (rec == 2) {
    os << "    ulonglong2 rv = ((const ulonglong2*)recs)[r];\n"
       << "    u64 code = rv.x;\n";
  } else {
    os << "    const u64* src = recs + r * " << rec << ";\n"
       << "    u64 code = src[0];\n";
  }
  os << "    int s = (int)(mix64(code) & " << (SLOTS - 1) << "u);\n"
     << "    int probes = 0;\n"
     << "    while (true) {\n"
     << "      u64 k = l_keys[s];\n"
     << "      if (k == code) break;\n"
     << "      if (k == ~0ull) {\n"
     << "        u64 old = atomicCAS((u64*)&l_keys[s], ~0ull, code);\n"
     << "        if (old == ~0ull || old == code) break;\n"
     << "      }\n"
     << "      s = (s + 1) & " << (SLOTS - 1) << ";\n"
     << "      if (++probes > " << SLOTS << ") { *overflow = 1; return; }\n"
     << "    }\n"
     << "    atomicAdd(&l_gcnt[s], 1u);\n";
  {
    int vs = 0;
    for (int a = 0; a < naggs; a++) {
      if (val_of[a] < 0) continue;
      std::string raw =
          code32 ? (NV == 1 ? std::string("r_vals[r]")
                            : ("r_vals[r * " + std::to_string(NV) + " + " +
                               std::to_string(vs) + "]"))
          : (rec == 2) ? std::string("rv.y")
                       : ("src[1 + " + std::to_string(vs) + "]");
      std::string dst = "l_vals[s * " + std::to_string(NV) + " + " +
                        std::to_string(vs) + "]";
      switch (A.op[a]) {
        case DSX_AGG_SUM_F64:
          os << "    atomicAdd((double*)&" << dst
             << ", __longlong_as_double((i64)" << raw << "));\n";
          break;
        case DSX_AGG_SUM_I64:
          os << "    atomicAdd((u64*)&" << dst << ", " << raw << ");\n";
          break;
        case DSX_AGG_MIN_F64:
          os << "    atomicMin((u64*)&" << dst
             << ", f64_ordered(__longlong_as_double((i64)" << raw << ")));\n";
          break;
        case DSX_AGG_MAX_F64:
          os << "    atomicMax((u64*)&" << dst
             << ", f64_ordered(__longlong_as_double((i64)" << raw << ")));\n";
          break;
        case DSX_AGG_MIN_I64:
          os << "    atomicMin((u64*)&" << dst << ", i64_ordered((i64)" << raw
             << "));\n";
          break;
        case DSX_AGG_MAX_I64:
          os << "    atomicMax((u64*)&" << dst << ", i64_ordered((i64)" << raw
             << "));\n";
          break;
      }
      vs++;
    }
  }
  os << "   }\n  }\n  }\n  __syncthreads();\n"
     << "  __shared__ u64 s_base;\n"
     << "  __shared__ unsigned int s_local;\n"
     << "  __shared__ unsigned int s_scan[BLOCK];\n"
     << "  unsigned int my_count = 0;\n"
     << "  for (int i = threadIdx.x; i < " << SLOTS << "; i += BLOCK)\n"
     << "    if (l_keys[i] != ~0ull) my_count++;\n"
     << "  s_scan[threadIdx.x] = my_count;\n  __syncthreads();\n"
     << "  for (int d = 1; d < BLOCK; d <<= 1) {\n"
     << "    unsigned int v = (threadIdx.x >= d) ? s_scan[threadIdx.x - d] : 0;\n"
     << "    __syncthreads();\n    s_scan[threadIdx.x] += v;\n"
     << "    __syncthreads();\n  }\n"
     << "  unsigned int my_excl = s_scan[threadIdx.x] - my_count;\n"
     << "  if (threadIdx.x == BLOCK - 1) {\n"
     << "    unsigned int tot = s_scan[BLOCK - 1];\n"
     << "    s_base = tot ? atomicAdd(g_counter, (u64)tot) : 0;\n"
     << "    s_local = tot;\n  }\n  __syncthreads();\n"
     << "  if (s_local == 0) return;\n"
     << "  u64 base = s_base;\n"
     << "  unsigned int o = my_excl;\n"
     << "  for (int i = threadIdx.x; i < " << SLOTS << "; i += BLOCK) {\n"
     << "    if (l_keys[i] == ~0ull) continue;\n"
     << "    i64 dsti = (i64)(base + o);\n"
     << "    tmp_codes[dsti] = l_keys[i];\n"
     << "    tmp_gcnt[dsti] = (u64)l_gcnt[i];\n";
  for (int v = 0; v < NV; v++)
    os << "    tmp_vals[dsti * " << NV << " + " << v << "] = l_vals[i * "
       << NV << " + " << v << "];\n";
  os << "    o++;\n  }\n}\n";
  return os.str();
}

// builds j_direct for the small-key-space LDS path; "" on unsupported shape
static std::string jit_direct_source(const ColsArg& C, const KeyArg& K,
                                     const ProgArg& P, const DsxAggSpec* aggs,
                                     const AggArg& A, int naggs,
                                     int key_space) {
  std::ostringstream os;
  os << JIT_PRELUDE;
  char k;
  if (!jit_emit_fn(os, "eval_pred", P.ins, P.len, &C, &k)) return "";
  std::vector<char> kinds(naggs, 'l');
  for (int a = 0; a < naggs; a++) {
    char name[32];
    snprintf(name, sizeof name, "eval_agg%d", a);
    if (!jit_emit_fn(os, name, aggs[a].prog, aggs[a].prog_len, &C,
                     &kinds[a]))
      return "";
  }
  jit_emit_pack(os, K, &C);
  int KS = key_space;
  os << "extern \"C\" __global__ void __launch_bounds__(BLOCK) j_direct("
     << "ColsArg C, i64 n, u64* g_vals, u64* g_cnts, u64* g_gcnt) {\n"
     << "  extern __shared__ char smem[];\n"
     << "  u64* s_vals = (u64*)smem;\n"
     << "  u32* s_cnts = (u32*)(s_vals + " << naggs * KS << ");\n"
     << "  u32* s_gcnt = (u32*)(s_cnts + " << naggs * KS << ");\n";
  // identities inlined per agg block
  for (int a = 0; a < naggs; a++) {
    uint64_t ident = agg_identity(A.op[a]);
    os << "  for (int i = threadIdx.x; i < " << KS << "; i += BLOCK) "
       << "s_vals[" << a * KS << " + i] = " << ident << "ull;\n";
  }
  os << "  for (int i = threadIdx.x; i < " << naggs * KS
     << "; i += BLOCK) s_cnts[i] = 0;\n"
     << "  for (int i = threadIdx.x; i < " << KS
     << "; i += BLOCK) s_gcnt[i] = 0;\n"
     << "  __syncthreads();\n"
     << "  i64 lo, hi; block_range(n, 1, lo, hi);\n"
     << "  for (i64 r = lo + threadIdx.x; r < hi; r += BLOCK) {\n"
     << "    i64 pv; if (!(eval_pred(C, r, pv) && pv)) continue;\n"
     << "    int k = (int)jit_pack(C, r);\n"
     << "    atomicAdd(&s_gcnt[k], 1u);\n";
  for (int a = 0; a < naggs; a++)
    jit_emit_direct_agg(os, a, A.op[a], A.never_null[a], KS, kinds[a]);
  os << "  }\n  __syncthreads();\n";
  // merge partials into the global direct arrays (same contract as the
  // interpreter kernel)
  os << "  for (int i = threadIdx.x; i < " << KS << "; i += BLOCK)\n"
     << "    if (s_gcnt[i]) atomicAdd(&g_gcnt[i], (u64)s_gcnt[i]);\n";
  for (int a = 0; a < naggs; a++) {
    std::string live = A.never_null[a]
        ? ("s_gcnt[i]")
        : ("s_cnts[" + std::to_string(a * KS) + " + i]");
    os << "  for (int i = threadIdx.x; i < " << KS << "; i += BLOCK) {\n"
       << "    if (!(" << live << ")) continue;\n";
    std::string sv = "s_vals[" + std::to_string(a * KS) + " + i]";
    std::string gv = "g_vals[" + std::to_string(a * KS) + " + i]";
    switch (A.op[a]) {
      case DSX_AGG_SUM_F64:
        os << "    atomicAdd((double*)&" << gv
           << ", __longlong_as_double((i64)" << sv << "));\n";
        break;
      case DSX_AGG_SUM_I64:
        os << "    atomicAdd((u64*)&" << gv << ", (u64)" << sv << ");\n";
        break;
      case DSX_AGG_COUNT:
        break;
      case DSX_AGG_MIN_F64:
      case DSX_AGG_MIN_I64:
        os << "    atomicMin((u64*)&" << gv << ", (u64)" << sv << ");\n";
        break;
      case DSX_AGG_MAX_F64:
      case DSX_AGG_MAX_I64:
        os << "    atomicMax((u64*)&" << gv << ", (u64)" << sv << ");\n";
        break;
    }
    if (A.op[a] != DSX_AGG_COUNT || !A.never_null[a])
      os << "    atomicAdd(&g_cnts[" << a * KS << " + i], (u64)s_cnts["
         << a * KS << " + i]);\n";
    os << "  }\n";
  }
  os << "}\n";
  return os.str();
}

static bool jit_enabled() {
  static const bool dis = getenv("DSX_DISABLE_JIT") != nullptr;
  return !dis;
}

// compile-or-get; returns nullptr on any failure (caller falls back)
static JitEntry* jit_source_entry(DsxCtx* c, const std::string& src) {
  if (src.empty() || !jit_enabled()) return nullptr;
  static const char* dump = getenv("DSX_JIT_DUMP");
  if (dump) {
    static int seq = 0;
    char fn[512];
    snprintf(fn, sizeof fn, "%s/jit_%03d.cu", dump, seq++);
    FILE* f = fopen(fn, "w");
    if (f) {
      fwrite(src.data(), 1, src.size(), f);
      fclose(f);
    }
  }
  if (!c->jit_cache) c->jit_cache = new JitCacheMap();
  JitEntry* e = jit_lookup(c, src);
  if (e) return e->mod ? e : nullptr;  // negative-cached failures
  e = jit_compile(c, src);
  if (!e) {  // negative-cache so we compile-fail once per shape
    ((JitCacheMap*)c->jit_cache)->m[src] = JitEntry();
    return nullptr;
  }
  return e;
}

// ---------------------------------------------------------------------------
// j_fprobe_mask — the filter-probe mask pass (k_fprobe_mask's contract,
// dsxhip.hip) specialized per query shape: predicate, key pack, key-validity
// presence, table layout and R (64-row words per wave iteration) are inlined;
// pointers, n and tmask are kernel arguments so the source text — the cache
// key — is stable from call to call.
//
// The interpreter kernel waits for every load before it issues the next
// (validity → predicate column → key → first slot → chain: five dependent
// round trips per word) and spends ~11 500 instructions on its switches.
// Here a wave takes R consecutive words and the body runs in phases so that
// independent loads are in flight together:
//   A  every predicate/validity/key load of the R words, unconditionally
//      (the row index is clamped on the tail — a per-word "load or not"
//      would make the compiler branch and wait per word);
//   B  predicates, codes, hashes;
//   C  the R first-slot loads back to back (rows that failed the predicate
//      read slot 0: one broadcast line, no branch);
//   D  chain continuation, live lanes only, one word's chain after another.
// Load factor ≤ 0.5, so an EMPTY slot always ends a chain.
//
// Measured on Q3 SF10 (DESIGN.md §8 Round 4): the specialization halves the
// pass; every R above 1 is slower than R = 1 (as was a lock-step chain walk
// with R loads per round), so R = 1 ships and DSX_FPROBE_R re-measures.
// ---------------------------------------------------------------------------
#define DSX_FPROBE_JIT_WORDS 1  // shipped R

// join_filter.h once more, as text for the generated source (the header
// explains the DSX_JF_CODE form)
#undef DSX_JF_CODE
#define DSX_JF_CODE(...) #__VA_ARGS__
static const char* JIT_JOIN_FILTER =
#include "join_filter.h"
    ;
#undef DSX_JF_CODE
#define DSX_JF_CODE(...) __VA_ARGS__

// jf_mode (join_filter.h) is part of the text, so each mode compiles once per
// shape; the filter pointer and its code_max / word mask are arguments.
//   exact:  phase C loads one filter word per row instead of a slot, and
//           hit = alive & bit. No slot load, no chain, tkeys untouched.
//   hashed: the filter word is loaded first; only lanes that pass it load
//           their first slot and walk the chain.
// Both keep the branch-free load shape: a dead lane (failed predicate, NULL
// key, tail row) reads filter word 0 as it reads slot 0 without a filter, and
// so does a live lane whose code is past code_max (a miss). The code of a row
// under a NULL key is garbage and never indexes the filter.
static std::string jit_fprobe_source(const ColsArg& C, const KeyArg& K,
                                     const ProgArg& P, bool packed, int R,
                                     int jf_mode = DSX_JF_NONE) {
  if (R < 1 || R > 8 || K.nkeys < 1) return "";
  if (jf_mode < DSX_JF_NONE || jf_mode > DSX_JF_HASHED) return "";
  std::ostringstream os;
  os << JIT_PRELUDE;
  if (jf_mode != DSX_JF_NONE)
    os << "#define DSX_JF_HD __device__ __forceinline__\n"
       << JIT_JOIN_FILTER << "\n";
  char k;
  if (!jit_emit_fn(os, "eval_pred", P.ins, P.len, &C, &k)) return "";
  jit_emit_pack(os, K, &C);
  // NULL key never matches: every key column that carries a validity buffer
  os << "__device__ __forceinline__ bool jit_key_valid(const ColsArg& C, "
        "i64 r) {\n  bool ok = true;\n";
  for (int j = 0; j < K.nkeys; j++)
    if (C.validity[K.k[j].col])
      os << "  ok = ok & (C.validity[" << K.k[j].col << "][r] != 0);\n";
  os << "  return ok;\n}\n";
  const char* match = packed ? "(k[j] >> 32) == code[j]" : "k[j] == code[j]";
  os << "#define R " << R << "\n#define EMPTY_KEY 0xFFFFFFFFFFFFFFFFull\n"
     << "#define MATCH(j) (" << match << ")\n";
  if (jf_mode != DSX_JF_NONE) {
    os << R"(
extern "C" __global__ void __launch_bounds__(BLOCK) j_fprobe_mask(
    ColsArg C, i64 n, const u64* __restrict__ tkeys, i64 tmask,
    const u32* __restrict__ dup, u64* __restrict__ mask,
    i64* __restrict__ block_counts, i64* __restrict__ extra,
    const u32* __restrict__ jf, u64 jf_arg) {
  i64 lo, hi; block_range(n, 64, lo, hi);
  __shared__ u64 s_count;
  if (threadIdx.x == 0) {
    s_count = 0;
    if (blockIdx.x == 0) extra[0] = (i64)*dup;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const i64 w0 = (lo + 63) / 64, w1 = (hi + 63) / 64;  // lo == hi: no words
  i64 local = 0;
  for (i64 wb = w0 + (i64)wid * R; wb < w1; wb += (BLOCK / 64) * R) {
    bool alive[R]; u64 code[R]; u64 fw[R]; u32 f[R]; bool hit[R];
    // A: all column loads of the R words, in one branch-free block
#pragma unroll
    for (int j = 0; j < R; j++) {
      i64 r = (wb + j) * 64 + lane;
      i64 rc = r < n ? r : n - 1;  // clamped: the loads stay unconditional
      i64 pv; bool ok = eval_pred(C, rc, pv);
      bool kv = jit_key_valid(C, rc);
      code[j] = jit_pack(C, rc);
      alive[j] = (r < hi) & ok & (pv != 0) & kv;  // NULL predicate: false
    }
)";
    if (jf_mode == DSX_JF_EXACT)
      os << R"(    // B: filter words; jf_arg = code_max
#pragma unroll
    for (int j = 0; j < R; j++) {
      alive[j] = alive[j] & (code[j] <= jf_arg);
      fw[j] = alive[j] ? dsx_jf_exact_word(code[j]) : 0;
    }
    // C: one filter word per row, back to back; bit set <=> build key
#pragma unroll
    for (int j = 0; j < R; j++) f[j] = jf[fw[j]];
#pragma unroll
    for (int j = 0; j < R; j++)
      hit[j] = alive[j] & ((f[j] & dsx_jf_exact_bit(code[j])) != 0);
)";
    else
      os << R"(    // B: hashes and filter words; jf_arg = filter words - 1
    u64 h[R]; i64 s[R]; u64 k[R];
#pragma unroll
    for (int j = 0; j < R; j++) {
      h[j] = alive[j] ? dsx_jf_mix64(code[j]) : 0;
      fw[j] = alive[j] ? dsx_jf_hashed_word(h[j], jf_arg) : 0;
    }
    // C: filter words, then the first slots of the lanes that passed
#pragma unroll
    for (int j = 0; j < R; j++) f[j] = jf[fw[j]];
#pragma unroll
    for (int j = 0; j < R; j++) {
      u32 bits = dsx_jf_hashed_bits(h[j]);
      alive[j] = alive[j] & ((f[j] & bits) == bits);
      s[j] = alive[j] ? (i64)(h[j] & (u64)tmask) : 0;
    }
#pragma unroll
    for (int j = 0; j < R; j++) k[j] = tkeys[s[j]];
    // D: the rest of each chain, one word after another
#pragma unroll
    for (int j = 0; j < R; j++) {
      hit[j] = false;
      bool go = alive[j];
      while (go) {
        if (k[j] == EMPTY_KEY) break;
        if (MATCH(j)) { hit[j] = true; break; }
        s[j] = (s[j] + 1) & tmask;
        k[j] = tkeys[s[j]];
      }
    }
)";
    os << R"(#pragma unroll
    for (int j = 0; j < R; j++) {
      u64 m = __builtin_amdgcn_ballot_w64(hit[j]);
      if (lane == 0 && wb + j < w1) {
        mask[wb + j] = m;
        local += __builtin_popcountll(m);
      }
    }
  }
  if (lane == 0) atomicAdd(&s_count, (u64)local);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = (i64)s_count;
}
)";
    return os.str();
  }
  os << R"(
extern "C" __global__ void __launch_bounds__(BLOCK) j_fprobe_mask(
    ColsArg C, i64 n, const u64* __restrict__ tkeys, i64 tmask,
    const u32* __restrict__ dup, u64* __restrict__ mask,
    i64* __restrict__ block_counts, i64* __restrict__ extra) {
  i64 lo, hi; block_range(n, 64, lo, hi);
  __shared__ u64 s_count;
  if (threadIdx.x == 0) {
    s_count = 0;
    if (blockIdx.x == 0) extra[0] = (i64)*dup;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const i64 w0 = (lo + 63) / 64, w1 = (hi + 63) / 64;  // lo == hi: no words
  i64 local = 0;
  for (i64 wb = w0 + (i64)wid * R; wb < w1; wb += (BLOCK / 64) * R) {
    bool alive[R]; u64 code[R]; i64 s[R]; u64 k[R];
    // A: all column loads of the R words, in one branch-free block
#pragma unroll
    for (int j = 0; j < R; j++) {
      i64 r = (wb + j) * 64 + lane;
      i64 rc = r < n ? r : n - 1;  // clamped: the loads stay unconditional
      i64 pv; bool ok = eval_pred(C, rc, pv);
      bool kv = jit_key_valid(C, rc);
      code[j] = jit_pack(C, rc);
      alive[j] = (r < hi) & ok & (pv != 0) & kv;  // NULL predicate: false
    }
    // B: hashes (kept apart from A: the compiler branches around the 64-bit
    // multiplies of a word with no live row, and a branch in A would make
    // each word's loads wait for the previous word's)
#pragma unroll
    for (int j = 0; j < R; j++)
      s[j] = alive[j] ? (i64)(mix64(code[j]) & (u64)tmask) : 0;
    // C: first slots, back to back
#pragma unroll
    for (int j = 0; j < R; j++) k[j] = tkeys[s[j]];
    bool hit[R];
    // D: the rest of each chain, one word after another
#pragma unroll
    for (int j = 0; j < R; j++) {
      hit[j] = false;
      bool go = alive[j];
      while (go) {
        if (k[j] == EMPTY_KEY) break;
        if (MATCH(j)) { hit[j] = true; break; }
        s[j] = (s[j] + 1) & tmask;
        k[j] = tkeys[s[j]];
      }
    }
#pragma unroll
    for (int j = 0; j < R; j++) {
      u64 m = __builtin_amdgcn_ballot_w64(hit[j]);
      if (lane == 0 && wb + j < w1) {
        mask[wb + j] = m;
        local += __builtin_popcountll(m);
      }
    }
  }
  if (lane == 0) atomicAdd(&s_count, (u64)local);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = (i64)s_count;
}
)";
  return os.str();
}

// read per call, so one process can run both variants
static bool jit_fprobe_enabled() {
  const char* e = getenv("DSX_DISABLE_JIT_FPROBE");
  return !(e && *e && strcmp(e, "0") != 0);
}

// measurement knob behind the Round 4 comparison: DSX_FPROBE_R = 1..8 words
// per wave iteration; unset or out of range, the shipped value holds
static int jit_fprobe_words() {
  const char* e = getenv("DSX_FPROBE_R");
  int v = e ? atoi(e) : 0;
  return v < 1 || v > 8 ? DSX_FPROBE_JIT_WORDS : v;
}

// the generated mask kernel for this shape, or nullptr: JIT disabled, the
// generator rejects the predicate, or hipRTC failed (negative-cached)
static hipFunction_t fprobe_mask_jit_fn(DsxCtx* c, const ProgArg& P,
                                        const KeyArg& K, const ColsArg& C,
                                        int packed, int jf_mode) {
  if (!jit_enabled() || !jit_fprobe_enabled()) return nullptr;
  JitEntry* je = jit_source_entry(
      c, jit_fprobe_source(C, K, P, packed != 0, jit_fprobe_words(),
                           jf_mode));
  return je ? jit_fn(c, je, "j_fprobe_mask") : nullptr;
}

static void fprobe_mask_jit_launch(DsxCtx* c, hipFunction_t f, int grid,
                                   const ColsArg& C, int64_t n,
                                   const uint64_t* tkeys, int64_t tmask,
                                   const unsigned int* dup, uint64_t* mask,
                                   int64_t* block_counts, int64_t* extra,
                                   const uint32_t* jf, uint64_t jf_arg) {
  ColsArg Ca = C;
  // jf and jf_arg are parameters of the filtered modes' kernels only; the
  // launch reads as many entries as the kernel declares
  void* args[] = {&Ca,   &n,           &tkeys, &tmask, &dup,
                  &mask, &block_counts, &extra, &jf,    &jf_arg};
  hipModuleLaunchKernel(f, grid, 1, 1, BLOCK, 1, 1, 0, c->stream, args,
                        nullptr);
  c->fprobe_jit_launches++;
}
