// jit.inc — hipRTC query-shape specialization (included by dsxhip.hip).
//
// The generic kernels interpret expression programs per row; at HBM-roofline
// scan rates the per-row instruction budget is ~3 wave-instructions
// (measured: the interpreter costs 2-6× roofline on hist/scatter/direct).
// So the hot groupby kernels are re-generated PER QUERY SHAPE with the
// predicate, agg-input expressions, agg ops and layout constants inlined,
// compiled once with hipRTC (~0.3 s, cached by source text), and launched
// via hipModuleLaunchKernel. This is the MI355X-native analog of the
// JIT'd fused operators GPU SQL engines use — no tracing framework, just
// explicit kernels generated at plan time. Fallback: the interpreter
// kernels (DSX_DISABLE_JIT, or any hiprtc failure).

#include <hip/hiprtc.h>
#include <sstream>

struct JitEntry {
  hipModule_t mod = nullptr;
  std::unordered_map<std::string, hipFunction_t> fns;
};

// source prelude: MUST textually mirror the host-side struct layouts
static const char* JIT_PRELUDE = R"(
typedef long long i64; typedef unsigned long long u64;
typedef unsigned int u32; typedef unsigned char u8;
#define BLOCK 256
#define DSX_MAX_KEYS 4
struct ColsArg {
  const void* data[16];
  const u8* validity[16];
  int dtype[16];
  int ncols;
};
struct KeySpecJ { int col; i64 min; i64 range; int nullable; int mode; };
struct KeyArg { KeySpecJ k[DSX_MAX_KEYS]; u64 stride[DSX_MAX_KEYS]; int nkeys; };
__device__ __forceinline__ u64 mix64(u64 x) {
  x += 0x9E3779B97F4A7C15ull; x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31; return x;
}
__device__ __forceinline__ void block_range(i64 n, i64 unit, i64& lo, i64& hi) {
  i64 nu = (n + unit - 1) / unit;
  i64 per = (nu + gridDim.x - 1) / gridDim.x;
  lo = (i64)blockIdx.x * per * unit;
  i64 h = lo + per * unit;
  hi = h < n ? h : n;
  if (lo > n) lo = n;
}
__device__ __forceinline__ int gb_bucket(u64 code, int nb_mask) {
  return (int)((mix64(code ^ 0xC2B2AE3D27D4EB4Full) >> 32) & (u64)nb_mask);
}
__device__ __forceinline__ u64 f64_ordered(double d) {
  u64 b = __double_as_longlong(d);
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ u64 i64_ordered(i64 v) {
  return (u64)v ^ 0x8000000000000000ull;
}
extern "C" __device__ double __ocml_exp_f64(double);
extern "C" __device__ double __ocml_log_f64(double);
extern "C" __device__ double __ocml_pow_f64(double, double);
extern "C" __device__ double __ocml_sin_f64(double);
extern "C" __device__ double __ocml_cos_f64(double);
extern "C" __device__ double __ocml_tan_f64(double);
extern "C" __device__ double __ocml_asin_f64(double);
extern "C" __device__ double __ocml_acos_f64(double);
extern "C" __device__ double __ocml_atan_f64(double);
extern "C" __device__ double __ocml_atan2_f64(double, double);
__device__ __forceinline__ i64 jit_absl(i64 v) { return v < 0 ? -v : v; }
__device__ __forceinline__ void jit_civil(i64 days, int& y, int& m, int& d) {
  i64 z = days + 719468;
  i64 era = (z >= 0 ? z : z - 146096) / 146097;
  i64 doe = z - era * 146097;
  i64 yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  i64 yy = yoe + era * 400;
  i64 doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  i64 mp = (5 * doy + 2) / 153;
  d = (int)(doy - (153 * mp + 2) / 5 + 1);
  m = (int)(mp < 10 ? mp + 3 : mp - 9);
  y = (int)(yy + (m <= 2));
}
__device__ __forceinline__ i64 jit_year(i64 v) {
  int y, m, d; jit_civil(v, y, m, d); return y;
}
__device__ __forceinline__ i64 jit_month(i64 v) {
  int y, m, d; jit_civil(v, y, m, d); return m;
}
__device__ __forceinline__ i64 jit_day(i64 v) {
  int y, m, d; jit_civil(v, y, m, d); return d;
}
)";

// ---- expression → C source ------------------------------------------------
static const size_t JIT_EXPR_MAX_CHARS = 1 << 16;

struct JitExprGen {
  const ColsArg* cols;  // metadata only (dtype + validity presence)
  bool ok = true;
  std::vector<std::array<std::string, 2>> stk;  // [value_expr, valid_expr]
  std::vector<char> kinds;                      // 'l' or 'd'

  void push(std::string v, std::string ok_, char k) {
    stk.push_back({std::move(v), std::move(ok_)});
    kinds.push_back(k);
  }
  void pop2(std::string& a, std::string& av, char& ka, std::string& b,
            std::string& bv, char& kb) {
    b = stk.back()[0]; bv = stk.back()[1]; kb = kinds.back();
    stk.pop_back(); kinds.pop_back();
    a = stk.back()[0]; av = stk.back()[1]; ka = kinds.back();
    stk.pop_back(); kinds.pop_back();
  }

  std::string col_load(int ci, char& kind) {
    char buf[160];
    switch (cols->dtype[ci]) {
      case DSX_I64:
        kind = 'l';
        snprintf(buf, sizeof buf, "((const i64*)C.data[%d])[r]", ci);
        break;
      case DSX_F64:
        kind = 'd';
        snprintf(buf, sizeof buf, "((const double*)C.data[%d])[r]", ci);
        break;
      case DSX_I32:
        kind = 'l';
        snprintf(buf, sizeof buf, "(i64)((const int*)C.data[%d])[r]", ci);
        break;
      case DSX_F32:
        kind = 'd';
        snprintf(buf, sizeof buf, "(double)((const float*)C.data[%d])[r]", ci);
        break;
      case DSX_I8:
        kind = 'l';
        snprintf(buf, sizeof buf,
                 "(i64)((const signed char*)C.data[%d])[r]", ci);
        break;
      default:  // BOOL8
        kind = 'l';
        snprintf(buf, sizeof buf, "(i64)((const u8*)C.data[%d])[r]", ci);
    }
    return buf;
  }

  // returns false on unsupported op
  bool gen(const DsxInstr* prog, int len) {
    for (int pc = 0; pc < len && ok; pc++) {
      const DsxInstr& in = prog[pc];
      char ka, kb;
      std::string a, av, b, bv;
      char buf[64];
      switch (in.op) {
        case DSX_OP_COL: {
          char k;
          std::string v = col_load(in.arg0, k);
          std::string ok_ = cols->validity[in.arg0]
              ? ("(C.validity[" + std::to_string(in.arg0) + "][r] != 0)")
              : std::string("true");
          push(v, ok_, k);
          break;
        }
        case DSX_OP_LIT_F64: {
          double d;
          memcpy(&d, &in.imm, 8);
          snprintf(buf, sizeof buf, "%.17g", d);
          push(buf, "true", 'd');
          break;
        }
        case DSX_OP_LIT_I64:
          snprintf(buf, sizeof buf, "%lldll", (long long)in.imm);
          push(buf, "true", 'l');
          break;
        case DSX_OP_LIT_NULL:
          push("0ll", "false", 'l');
          break;
#define JBIN(OP, CEXPR, K)                                                     \
  case OP:                                                                     \
    pop2(a, av, ka, b, bv, kb);                                                \
    push("(" + a + CEXPR + b + ")",                                            \
         (av == "true" && bv == "true") ? std::string("true")                  \
                                        : "(" + av + " && " + bv + ")",        \
         K);                                                                   \
    break;
        JBIN(DSX_OP_ADD_F64, " + ", 'd')
        JBIN(DSX_OP_SUB_F64, " - ", 'd')
        JBIN(DSX_OP_MUL_F64, " * ", 'd')
        JBIN(DSX_OP_DIV_F64, " / ", 'd')
        JBIN(DSX_OP_ADD_I64, " + ", 'l')
        JBIN(DSX_OP_SUB_I64, " - ", 'l')
        JBIN(DSX_OP_MUL_I64, " * ", 'l')
        JBIN(DSX_OP_LT_F64, " < ", 'l')
        JBIN(DSX_OP_LE_F64, " <= ", 'l')
        JBIN(DSX_OP_GT_F64, " > ", 'l')
        JBIN(DSX_OP_GE_F64, " >= ", 'l')
        JBIN(DSX_OP_EQ_F64, " == ", 'l')
        JBIN(DSX_OP_NE_F64, " != ", 'l')
        JBIN(DSX_OP_LT_I64, " < ", 'l')
        JBIN(DSX_OP_LE_I64, " <= ", 'l')
        JBIN(DSX_OP_GT_I64, " > ", 'l')
        JBIN(DSX_OP_GE_I64, " >= ", 'l')
        JBIN(DSX_OP_EQ_I64, " == ", 'l')
        JBIN(DSX_OP_NE_I64, " != ", 'l')
#undef JBIN
        case DSX_OP_DIV_I64:
          pop2(a, av, ka, b, bv, kb);
          push("((" + b + ") ? (" + a + ") / (" + b + ") : 0ll)",
               "(" + av + " && " + bv + ")", 'l');
          break;
        case DSX_OP_MOD_I64:
          pop2(a, av, ka, b, bv, kb);
          push("((" + b + ") ? (" + a + ") % (" + b + ") : 0ll)",
               "(" + av + " && " + bv + ")", 'l');
          break;
        case DSX_OP_FLOORMOD_I64:
          pop2(a, av, ka, b, bv, kb);
          push("((" + b + ") ? (((" + a + ") % (" + b + ")) + (" + b +
                   ")) % (" + b + ") : 0ll)",
               "(" + av + " && " + bv + ")", 'l');
          break;
        case DSX_OP_AND:
          pop2(a, av, ka, b, bv, kb);
          if (av == "true" && bv == "true") {  // no NULLs: plain &&
            push("(i64)((" + a + ") && (" + b + "))", "true", 'l');
            break;
          }
          // SQL 3VL: F if either valid-false; else NULL if any NULL
          push("(i64)(((" + av + ") && !(" + a + ")) || ((" + bv +
                   ") && !(" + b + ")) ? 0 : 1)",
               "((((" + av + ") && !(" + a + ")) || ((" + bv + ") && !(" + b +
                   "))) || ((" + av + ") && (" + bv + ")))",
               'l');
          break;
        case DSX_OP_OR:
          pop2(a, av, ka, b, bv, kb);
          if (av == "true" && bv == "true") {  // no NULLs: plain ||
            push("(i64)((" + a + ") || (" + b + "))", "true", 'l');
            break;
          }
          push("(i64)((((" + av + ") && (" + a + ")) || ((" + bv + ") && (" +
                   b + "))) ? 1 : 0)",
               "((((" + av + ") && (" + a + ")) || ((" + bv + ") && (" + b +
                   "))) || ((" + av + ") && (" + bv + ")))",
               'l');
          break;
        case DSX_OP_NOT: {
          a = stk.back()[0]; stk.back()[0] = "(i64)(!(" + a + "))";
          kinds.back() = 'l';
          break;
        }
        case DSX_OP_IS_NULL: {
          av = stk.back()[1];
          stk.back()[0] = "(i64)(!(" + av + "))";
          stk.back()[1] = "true";
          kinds.back() = 'l';
          break;
        }
        case DSX_OP_IS_NOT_NULL: {
          av = stk.back()[1];
          stk.back()[0] = "(i64)(" + av + ")";
          stk.back()[1] = "true";
          kinds.back() = 'l';
          break;
        }
        case DSX_OP_I64_TO_F64:
          stk.back()[0] = "(double)(" + stk.back()[0] + ")";
          kinds.back() = 'd';
          break;
        case DSX_OP_F64_TO_I64:
          stk.back()[0] = "(i64)(" + stk.back()[0] + ")";
          kinds.back() = 'l';
          break;
        case DSX_OP_BITS_F64:
          stk.back()[0] = "__longlong_as_double((i64)(" + stk.back()[0] +
                          "))";
          kinds.back() = 'd';
          break;
#define JUN(OP, PRE, POST, K)                                                  \
  case OP:                                                                     \
    stk.back()[0] = std::string(PRE) + stk.back()[0] + POST;                   \
    kinds.back() = K;                                                          \
    break;
        JUN(DSX_OP_ABS_I64, "(jit_absl(", "))", 'l')
        JUN(DSX_OP_ABS_F64, "__builtin_fabs((double)(", "))", 'd')
        JUN(DSX_OP_FLOOR_F64, "__builtin_floor((double)(", "))", 'd')
        JUN(DSX_OP_CEIL_F64, "__builtin_ceil((double)(", "))", 'd')
        JUN(DSX_OP_RINT_F64, "__builtin_rint((double)(", "))", 'd')
        JUN(DSX_OP_EXP_F64, "__ocml_exp_f64((double)(", "))", 'd')
        JUN(DSX_OP_LN_F64, "__ocml_log_f64((double)(", "))", 'd')
        JUN(DSX_OP_SIN_F64, "__ocml_sin_f64((double)(", "))", 'd')
        JUN(DSX_OP_COS_F64, "__ocml_cos_f64((double)(", "))", 'd')
        JUN(DSX_OP_TAN_F64, "__ocml_tan_f64((double)(", "))", 'd')
        JUN(DSX_OP_ASIN_F64, "__ocml_asin_f64((double)(", "))", 'd')
        JUN(DSX_OP_ACOS_F64, "__ocml_acos_f64((double)(", "))", 'd')
        JUN(DSX_OP_ATAN_F64, "__ocml_atan_f64((double)(", "))", 'd')
        JUN(DSX_OP_YEAR, "jit_year((i64)(", "))", 'l')
        JUN(DSX_OP_MONTH, "jit_month((i64)(", "))", 'l')
        JUN(DSX_OP_DAY, "jit_day((i64)(", "))", 'l')
#undef JUN
        case DSX_OP_ATAN2_F64:
          pop2(a, av, ka, b, bv, kb);
          push("__ocml_atan2_f64((double)(" + a + "), (double)(" + b +
                   "))",
               (av == "true" && bv == "true") ? std::string("true")
                                              : "(" + av + " && " + bv + ")",
               'd');
          break;
        case DSX_OP_POW_F64:
          pop2(a, av, ka, b, bv, kb);
          push("__ocml_pow_f64((double)(" + a + "), (double)(" + b + "))",
               (av == "true" && bv == "true") ? std::string("true")
                                              : "(" + av + " && " + bv + ")",
               'd');
          break;
        case DSX_OP_NEG_F64:
        case DSX_OP_NEG_I64:
          stk.back()[0] = "(-(" + stk.back()[0] + "))";
          break;
        case DSX_OP_SQRT_F64:
          stk.back()[0] = "__builtin_sqrt((double)(" + stk.back()[0] + "))";
          kinds.back() = 'd';
          break;
        case DSX_OP_SELECT: {
          std::string cv = stk[stk.size() - 3][0];
          std::string cok = stk[stk.size() - 3][1];
          std::string x = stk[stk.size() - 2][0];
          std::string xok = stk[stk.size() - 2][1];
          std::string y = stk[stk.size() - 1][0];
          std::string yok = stk[stk.size() - 1][1];
          char ky = kinds[kinds.size() - 1];
          stk.pop_back(); stk.pop_back(); stk.pop_back();
          kinds.pop_back(); kinds.pop_back(); kinds.pop_back();
          std::string take = "((" + cok + ") && (" + cv + "))";
          push("(" + take + " ? (" + x + ") : (" + y + "))",
               "(" + take + " ? (" + xok + ") : (" + yok + "))", ky);
          break;
        }
        default:
          ok = false;
      }
      // the 3VL AND/OR forms repeat their operands' text, so a long chain
      // over nullable columns grows ~2.6x per level: past this size leave
      // the expression to the interpreter kernels
      if (!stk.empty() &&
          stk.back()[0].size() + stk.back()[1].size() > JIT_EXPR_MAX_CHARS)
        ok = false;
    }
    return ok && stk.size() == 1;
  }
};

// emit "__device__ bool <name>(const ColsArg& C, i64 r, <T>& out)" returning
// validity; T = double when kind 'd' else i64
static bool jit_emit_fn(std::ostringstream& os, const char* name,
                        const DsxInstr* prog, int len, const ColsArg* cols,
                        char* out_kind) {
  if (len == 0) {  // no predicate → always true
    os << "__device__ __forceinline__ bool " << name
       << "(const ColsArg& C, i64 r, i64& out) { out = 1; return true; }\n";
    *out_kind = 'l';
    return true;
  }
  JitExprGen g;
  g.cols = cols;
  if (!g.gen(prog, len)) return false;
  *out_kind = g.kinds[0];
  const char* ty = g.kinds[0] == 'd' ? "double" : "i64";
  os << "__device__ __forceinline__ bool " << name << "(const ColsArg& C, "
     << "i64 r, " << ty << "& out) { out = (" << ty << ")(" << g.stk[0][0]
     << "); return " << g.stk[0][1] << "; }\n";
  return true;
}

// pack_key over inlined key specs
static void jit_emit_pack(std::ostringstream& os, const KeyArg& K,
                          const ColsArg* cols) {
  os << "__device__ __forceinline__ u64 jit_pack(const ColsArg& C, i64 r) {\n"
     << "  u64 code = 0;\n";
  uint64_t stride = 1;
  for (int j = 0; j < K.nkeys; j++) {
    const DsxKeySpec* keys = K.k;
    int ci = keys[j].col;
    if (keys[j].mode & 6) {
      // ORDER-BY mode bits (DESC / NULLS LAST) are a static-pack_key-only
      // feature; force a loud hiprtc failure instead of silently packing
      // without the flips
      os << "#error jit_pack does not support ORDER-BY mode bits\n";
      return;
    }
    if (keys[j].mode == 1) {
      const char* lt = cols->dtype[ci] == DSX_F32 ? "float" : "double";
      os << "  { double x = (double)((const " << lt << "*)C.data[" << ci
         << "])[r];\n    bool ok = "
         << (cols->validity[ci]
                 ? ("C.validity[" + std::to_string(ci) + "][r] != 0")
                 : std::string("true"))
         << ";\n    code += (!ok || x != x) ? 0ull"
            " : (u64)__double_as_longlong(x == 0.0 ? 0.0 : x) + 1; }\n";
      continue;
    }
    const char* ld;
    char ldbuf[128];
    switch (cols->dtype[ci]) {
      case DSX_I64:
        snprintf(ldbuf, sizeof ldbuf, "((const i64*)C.data[%d])[r]", ci);
        break;
      case DSX_I32:
        snprintf(ldbuf, sizeof ldbuf, "(i64)((const int*)C.data[%d])[r]", ci);
        break;
      case DSX_I8:
        snprintf(ldbuf, sizeof ldbuf,
                 "(i64)((const signed char*)C.data[%d])[r]", ci);
        break;
      default:
        snprintf(ldbuf, sizeof ldbuf, "(i64)((const u8*)C.data[%d])[r]", ci);
    }
    ld = ldbuf;
    if (keys[j].nullable && cols->validity[ci]) {
      os << "  { bool ok = C.validity[" << ci << "][r] != 0;\n"
         << "    u64 part = ok ? (u64)((" << ld << ") - (" << keys[j].min
         << "ll)) + 1 : 0;\n    code += part * " << stride << "ull; }\n";
    } else if (keys[j].nullable) {
      // nullable FLAG without a validity buffer on THIS side: values still
      // shift +1 so codes stay comparable with the other join side (the
      // static pack_key shifts on the flag alone — radix join bug r2)
      os << "  code += ((u64)((" << ld << ") - (" << keys[j].min
         << "ll)) + 1) * " << stride << "ull;\n";
    } else {
      os << "  code += (u64)((" << ld << ") - (" << keys[j].min << "ll)) * "
         << stride << "ull;\n";
    }
    stride *= (uint64_t)keys[j].range + (keys[j].nullable ? 1 : 0);
  }
  os << "  return code;\n}\n";
}

// host-side cache lives in DsxCtx (declared there as void* to avoid header
// churn): map source → JitEntry
struct JitCacheMap {
  std::unordered_map<std::string, JitEntry> m;
};

static JitEntry* jit_lookup(DsxCtx* c, const std::string& src) {
  if (!c->jit_cache) c->jit_cache = new JitCacheMap();
  auto& m = ((JitCacheMap*)c->jit_cache)->m;
  auto it = m.find(src);
  return it == m.end() ? nullptr : &it->second;
}

static JitEntry* jit_compile(DsxCtx* c, const std::string& src) {
  auto& m = ((JitCacheMap*)c->jit_cache)->m;
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "dsx_jit.cu", 0, nullptr,
                          nullptr) != HIPRTC_SUCCESS)
    return nullptr;
  const char* opts[] = {"-O3", "--offload-arch=gfx950", "-std=c++17",
                        "-munsafe-fp-atomics"};
  hiprtcResult rc = hiprtcCompileProgram(prog, 4, opts);
  if (rc != HIPRTC_SUCCESS) {
    size_t lsz = 0;
    hiprtcGetProgramLogSize(prog, &lsz);
    std::string log(lsz, '\0');
    if (lsz) hiprtcGetProgramLog(prog, &log[0]);
    fprintf(stderr, "[dsxhip] JIT compile failed (falling back to "
                    "interpreter):\n%s\n", log.c_str());
    hiprtcDestroyProgram(&prog);
    return nullptr;
  }
  size_t csz = 0;
  hiprtcGetCodeSize(prog, &csz);
  std::string code(csz, '\0');
  hiprtcGetCode(prog, &code[0]);
  hiprtcDestroyProgram(&prog);
  JitEntry e;
  if (hipModuleLoadData(&e.mod, code.data()) != hipSuccess) return nullptr;
  auto& slot = m[src];
  slot = e;
  return &slot;
}

static hipFunction_t jit_fn(DsxCtx* c, JitEntry* e, const char* name) {
  auto it = e->fns.find(name);
  if (it != e->fns.end()) return it->second;
  hipFunction_t f;
  if (hipModuleGetFunction(&f, e->mod, name) != hipSuccess) return nullptr;
  e->fns[name] = f;
  return f;
}
