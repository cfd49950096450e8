// Prints the GEMM dispatcher's plan (ops/csrc/gemm_plan.h) for every case read on stdin, one
// "case <TAB> plan" line each.  Host code only: tests/test_gemm_plan_cpu.py builds it with the
// host C++ compiler and compares its output with tests/golden/gemm_plan_cases.txt.
//
// A case is a product signature as ops/gemm.py keys gemm_tuned.json,
//   MxNxK:<A><B layout, k or m>:<f32 or bf16 (h) output>:<act><act_bwd>:<flags>
// (flags: b bias, x aux_out, r residual, c colsum, a accumulate), then key=value tokens:
//   impl ws          GemmArgs::impl, workspace MiB
//   deriv            GemmArgs::aux_deriv
//   lda ldb ldc ldr ldi ldo    leading dimensions (default: the stored columns rounded up to 8)
//   ac bc            stored columns of A / B (default: K for a k-major operand, else M / N)
//   coff             byte offset of C from a 256-B aligned address
//   gimpl splits xcd reserve actlds reslds nt    GemmSettings: impl, force_splits, xcd_split,
//                    cu_reserve, act_lds, res_lds, nt_store
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "gemm_plan.h"

using dpc::GemmArgs;
using dpc::GemmSettings;

static bool parse_case(const std::string& line, GemmArgs& a, GemmSettings& st) {
  long long v[32];
  static const char* keys[] = {"deriv", "impl", "ws", "lda", "ldb", "ldc", "ldr", "ldi", "ldo", "ac", "bc", "coff",
                               "gimpl", "splits", "xcd", "reserve", "actlds", "reslds", "nt"};
  enum { DERIV, IMPL, WS, LDA, LDB, LDC, LDR, LDI, LDO, AC, BC, COFF, GIMPL, SPLITS, XCD, RESERVE, ACTLDS, RESLDS, NT,
         NKEYS };
  for (int i = 0; i < NKEYS; ++i) v[i] = -1;
  int M, N, K, act, actb;
  char la, lb, out, flags[16] = "";
  if (sscanf(line.c_str(), "%dx%dx%d:%c%c:%c:%1d%1d:%15[a-z]", &M, &N, &K, &la, &lb, &out, &act, &actb, flags) < 8) return false;
  size_t pos = line.find(' ');
  while (pos != std::string::npos && pos < line.size()) {
    size_t end = line.find(' ', ++pos);
    if (end == std::string::npos) end = line.size();
    const std::string tok = line.substr(pos, end - pos);
    pos = end;
    if (tok.empty()) continue;
    const size_t eq = tok.find('=');
    if (eq == std::string::npos) return false;
    int k = 0;
    while (k < NKEYS && tok.compare(0, eq, keys[k]) != 0) ++k;
    if (k == NKEYS) return false;
    v[k] = atoll(tok.c_str() + eq + 1);
  }
  auto has = [&](char c) { return strchr(flags, c) != nullptr; };
  auto get = [&](int k, long long d) { return v[k] >= 0 ? v[k] : d; };
  auto r8 = [](long long x) { return (x + 7) / 8 * 8; };
  auto fake = [](int slot, long long off = 0) { return (void*)(uintptr_t)(0x100000000ull * (unsigned)slot + (unsigned long long)off); };
  a = GemmArgs{};
  st = GemmSettings{};
  a.M = M, a.N = N, a.K = K;
  a.a_kmaj = la == 'k', a.b_kmaj = lb == 'k';
  a.a_r = a.a_kmaj ? a.M : a.K, a.a_c = (int)get(AC, a.a_kmaj ? a.K : a.M);
  a.b_r = a.b_kmaj ? a.N : a.K, a.b_c = (int)get(BC, a.b_kmaj ? a.K : a.N);
  a.lda = get(LDA, r8(a.a_c)), a.ldb = get(LDB, r8(a.b_c)), a.ldc = get(LDC, a.N);
  a.out_f32 = out == 'f', a.accumulate = has('a');
  a.act = act, a.act_bwd = actb, a.aux_deriv = (int)get(DERIV, 0);
  a.alpha = 1.f;
  a.A = fake(1), a.B = fake(2), a.C = fake(3, get(COFF, 0));
  if (has('b')) a.bias = (const float*)fake(4);
  if (has('r')) a.residual = (const float*)fake(5), a.ldr = get(LDR, a.N);
  if (a.act_bwd) a.aux_in = fake(6), a.ld_aux_in = get(LDI, a.N);
  if (has('x')) a.aux_out = fake(7), a.ld_aux_out = get(LDO, a.N);
  if (has('c')) a.colsum = (float*)fake(8);
  if (get(WS, 0) > 0) a.ws = fake(9), a.ws_bytes = v[WS] << 20;
  a.impl = (int)get(IMPL, 0);
  st.impl = v[GIMPL] >= 0 ? (int)v[GIMPL] : -1;
  st.force_splits = (int)get(SPLITS, 0), st.xcd_split = (int)get(XCD, 0), st.cu_reserve = (int)get(RESERVE, 0);
  st.act_lds = v[ACTLDS] >= 0 ? (int)v[ACTLDS] : -1, st.res_lds = v[RESLDS] >= 0 ? (int)v[RESLDS] : -1;
  st.nt_store = (int)get(NT, 77);
  st.cus = 256;
  return true;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--impls")) {  // the implementation table's ids
    for (const dpc::GemmImpl& r : dpc::GEMM_IMPLS) std::cout << r.id << "\t" << r.name << "\n";
    return 0;
  }
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    GemmArgs a;
    GemmSettings st;
    if (!parse_case(line, a, st)) {
      std::cerr << "bad case: " << line << "\n";
      return 2;
    }
    char buf[512];
    dpc::gemm_plan_text(dpc::gemm_plan(a, st), buf, (int)sizeof buf);
    std::cout << line << "\t" << buf << "\n";
  }
  return 0;
}
