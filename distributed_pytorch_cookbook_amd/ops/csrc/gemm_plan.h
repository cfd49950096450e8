// Which kernel a bf16 product gets: a pure host function from (GemmArgs, GemmSettings) to a
// GemmPlan.  No HIP header, no global state, nothing launched -- this file compiles with a plain
// host C++17 compiler, and tests/test_gemm_plan_cpu.py pins its answers without a GPU.  gemm.hip
// (gemm_run) turns a plan into launches.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>

namespace dpc {

struct GemmArgs {
  const void* A;
  const void* B;
  void* C;
  const float* bias;      // [N] f32, optional
  const float* residual;  // [M][ldr] f32, optional (may alias C)
  const void* aux_in;     // [M][ld_aux_in] bf16, optional: multiply by act'(aux_in)
  void* aux_out;          // [M][ld_aux_out] bf16, optional: store pre-activation
  const float* alpha_ptr; // device scalar multiplier, optional
  float* colsum;          // [N] f32, optional: colsum[n] += sum_m v (v after act_bwd, before act)
  long long lda, ldb, ldc, ldr, ld_aux_in, ld_aux_out;
  int M, N, K;
  float alpha;
  int act;         // activation applied after bias (Act)
  int act_bwd;     // multiply by act'(aux_in) (Act)
  int out_f32;     // C is f32 (else bf16)
  int accumulate;  // C += result (f32 output only)
  int a_kmaj, b_kmaj;
  // stored extents of the operands ([rows][cols] as laid out in memory); reads beyond them
  // return zeros.  k-major: rows = M or N, cols = K;  mn-major: rows = K, cols = M or N.
  int a_r, a_c, b_r, b_c;
  // set by the dispatcher (callers pass 0): > 1 = XCD-aligned split-K into this many k-ranges
  int ksplit;
  // caller's implementation choice (0 = the dispatcher's shape policy), e.g. from the
  // measured per-shape table of ops/gemm.py (autotuned on MI355X); a forced global impl
  // (dpc_gemm_set_impl, sweeps / tests) takes precedence
  int impl;
  // gemm_f32.hip only: aux_in / aux_out are f32 (else bf16)
  int aux_f32;
  // split-K workspace (optional, f32, ws_bytes long): the v7 kernel stores each k-range's
  // partial tile there with plain stores and a reduction pass sums them into C, instead of
  // f32 atomics into C (plan7 below)
  void* ws;
  long long ws_bytes;
  // set by the dispatcher (callers pass 0): epilogue stores with the non-temporal bit -- bit 0 the
  // bf16 C / aux_out stores, bit 1 the f32 C stores (DPC_GEMM_NT, default 3).  The short-K
  // forward products spent 20-35 % of their time in the tile-end store burst; with nt stores
  // v9 runs the GPT-2 QKV / up / LM-head forward 947 / 964 / 1031 -> 1151 / 1150 / 1163 TF/s
  // and 8192^3 1327 -> 1448 (bench/g7lab epi set, profiles/r4_gemm/lab_epi_nt.log)
  int nt_store;
  // forward epilogues with aux_out and act == ACT_GELU: aux_out = bf16(act'(v)) instead of the
  // pre-activation bf16(v), for an input gradient with act_bwd = ACT_MUL (models/fused.py: the
  // FFN up-projection)
  int aux_deriv;
};

struct G7Plan {
  int tiles_m, tiles_n;
  int tile_n;  // tile width: 256 (v7) or 128 (v8)
  int units;   // tiles x splits (split-major: unit = split * tiles + tile)
  int grid;    // workgroups launched
  int nk;      // k-slices per unit (even)
  int nk_all;  // k-slices of the whole product (slices of a unit past it read zeros)
  int splits;
  int store_cnt;  // vector-memory ops the epilogue issues per wave-lane (0: unknown -> no credit)
  int debug;      // bench/g7lab.hip only (the planner leaves 0): 1 = no epilogue (main-loop ablations, ABL)
};

// (common.h's Act values and gemm7_kern.h's slice depth; gemm.hip static_asserts they agree)
constexpr int GP_ACT_GELU = 2, GP_ACT_MUL = 3, GP_G7_KB = 32;

// ---- everything the decision reads besides the arguments.  gemm.hip keeps the one process-wide
// instance: the environment is read into it once, the dpc_*_set_* entry points write to it.
struct GemmSettings {
  int impl = -1;         // dpc_gemm_set_impl: >= 0 forces this implementation for every product
  int force_splits = 0;  // dpc_gemm_set_splits: > 0 forces the split-K count of plain f32 products
  // XCD-aligned split-K mapping of v2 / v3 (tile_slot): measured ~6 % slower than the default
  // mapping on the GPT-2 weight gradients, so off unless requested (sweeps)
  int xcd_split = 0;
  // DPC_GEMM_POLICY="fs=10,dl=4": per-class implementation override for sweeps.  fs / fl =
  // forward (both k-major) with K <= / > 1024, ds / dl = dgrad (B mn-major) with K <= / > 2304,
  // w = weight gradient (both mn-major).
  int policy[5] = {0, 0, 0, 0, 0};
  // GemmArgs::nt_store for every product (DPC_GEMM_NT: bit 0 bf16 outputs, bit 1 f32 outputs
  // non-temporal; bits 2-3 the cache scope of the v7 / v9 epilogue stores: 0 none, 1 sc0, 2 sc1,
  // 3 sc0 sc1).  Default 15 = nt + sc0 sc1: the epilogue's stores retire sooner, and the next
  // tile's counted DMA waits -- which CDNA4's one in-order vmcnt makes wait for them too -- stall
  // less.  Same box against nt alone (round 5, profiles/r5_epi/store_policy.log): up-projection
  // fused 402 -> 384 us, down-projection fused 367 -> 349, plain up 283 -> 274, plain input
  // gradient 300 -> 290; DDP 960.8K -> 971.6K (two runs each).  Bits 4-6: a separate scope for
  // the f32 outputs (gemm.h:g_f32_pol) -- default 77 = the above for bf16 outputs, PLAIN stores for
  // the f32 ones (the residual stream and the split-K slabs, which the next LayerNorm / the slab
  // reduction read back at once from the Infinity Cache): DDP +0.45 % same box, three interleaved
  // rounds (984.1 / 981.2 / 981.7K -> 989.7 / 984.5 / 985.5K, profiles/r5_epi/f32_store_scope.log).
  int nt_store = 77;
  // the LDS-staged act' / residual epilogues (EPI 8, 10 / EPI 9): setter value (dpc_gemm7_set_*,
  // -1 = unset), else DPC_G7_ACTLDS / DPC_G7_RESLDS (default on)
  int act_lds = -1, act_lds_env = 1;
  int res_lds = -1, res_lds_env = 1;
  // Resident-CU budget.  v7 / v8 / v9 are persistent: their grid is sized to fill every CU (one
  // / two 160 KiB workgroups each), so a kernel already resident on a CU -- an RCCL collective on
  // the comm stream -- would hold back that CU's GEMM workgroup until the collective ends, and
  // that workgroup's whole share of the tiles would then run as a second round (the product's
  // time roughly doubled).  While the engines have a collective in flight they reserve R CUs
  // (parallel/transport.py; DPC_CU_RESERVE): the grid shrinks to CUs - R workgroups, the XCD
  // remap (g7_local) stays bijective for any grid, and the tiles redistribute over the workgroups
  // that are resident.
  int cus = 256, cu_reserve = 0;
};

// ---- the implementation table: one row per id (GemmArgs::impl, dpc_gemm_set_impl, the values of
// ops/gemm_tuned.json, ops/gemm.py:_CANDIDATES).  Ids missing here (5-9, 11-15, 18: v3 / v4 / v5 /
// v6 variants that neither the table nor the policy chose) were removed; asking for one is an
// error (rc 1).
//   v1: register-staged 128x128 -- the fallback when v2's requirements fail, never a candidate
//   v2: LDS-DMA 128x128, 8 waves          v3: 256x128, 8 waves
//   v7: persistent 256x256, one 4-wave workgroup per CU, one wave per SIMD (each wave a 128x128
//       tile of 8 x 8 v_mfma_f32_16x16x32_bf16 accumulators), the k-slices of all its tiles one
//       stream through a 5-slot LDS ring filled by LDS-DMA and never drained at a tile boundary;
//       the epilogue works straight from registers (gemm7_kern.h).  Plain f32 products split K.
//       dma = where in the MFMA groups the DMA pieces issue (gemm7_kern.h SCHED): the column is
//       what the id ASKS for; gemm7_sched / gemm7_sched_plain below say what it gets -- pairs
//       under one M0 write (3) or quads (4) where the operands allow it, the split interleave (6)
//       whenever an operand is mn-major, v9 for plain nt products.
//   v8: v7 with 256x128 tiles, two workgroups per CU (epilogue beside the other's MFMAs)
//   v7d: v7 whose GELU / GELU' epilogues are deferred into the next tile's main loop
//   v9: 64-deep stages, whole-line DMA pieces of the k-major operands (gemm9_kern.h)
enum GemmFamily { GF_V1, GF_V2, GF_V3, GF_V7, GF_V8, GF_V7D, GF_V9 };
struct GemmImpl {
  int id;
  const char* name;
  int family;
  int kb, stages;      // k depth of a stage, ring slots
  int tile_m, tile_n;
  int wgs;             // v2 / v3: workgroups resident per CU (LDS-bound), for the split-K cost model
  int dma;             // v7 family: the DMA placement asked for
  bool persistent;     // grid capped at the resident workgroups, units streamed; else one unit each
};
constexpr GemmImpl GEMM_IMPLS[] = {
    {1, "v1", GF_V1, 64, 1, 128, 128, 2, 0, false},
    {2, "v2-64x2", GF_V2, 64, 2, 128, 128, 2, 0, false},
    {3, "v2-64x3", GF_V2, 64, 3, 128, 128, 1, 0, false},
    {4, "v2-32x3", GF_V2, 32, 3, 128, 128, 3, 0, false},
    {10, "v3-256x128", GF_V3, 32, 3, 256, 128, 1, 0, false},
    {16, "v7-dma0", GF_V7, 32, 5, 256, 256, 1, 0, true},
    {17, "v7-unit", GF_V7, 32, 5, 256, 256, 1, 2, false},
    {19, "v7-dma1", GF_V7, 32, 5, 256, 256, 1, 1, true},
    {20, "v7", GF_V7, 32, 5, 256, 256, 1, 2, true},
    {21, "v8", GF_V8, 32, 5, 256, 128, 2, 2, true},
    {22, "v7-pair", GF_V7, 32, 5, 256, 256, 1, 3, true},
    {23, "v7-quad", GF_V7, 32, 5, 256, 256, 1, 4, true},
    {24, "v7d", GF_V7D, 32, 5, 256, 256, 1, 5, true},
    {25, "v7-split", GF_V7, 32, 5, 256, 256, 1, 6, true},
    {26, "v9", GF_V9, 64, 2, 256, 256, 1, 7, true},
};
inline const GemmImpl* gemm_impl_row(int id) {
  for (const GemmImpl& r : GEMM_IMPLS)
    if (r.id == id) return &r;
  return nullptr;
}

// ---- the plan
// A kernel identity: the template family and its template arguments in declaration order (bools
// as 0 / 1) -- for the persistent families exactly what a line of gemm_parts.txt spells out.
enum GemmKernelFamily { GK_NONE, GK_V1, GK_V2, GK_V3, GK_V7, GK_V7D, GK_V9 };
struct GemmKernelId {
  int family;
  int t[8];
};
constexpr unsigned long long gemm_kernel_key(const GemmKernelId& k) {
  unsigned long long key = (unsigned long long)k.family;
  for (int i = 0; i < 6; ++i) key = (key << 8) | (unsigned long long)(k.t[i] & 255);
  return key;
}

enum GemmStep { GS_NONE, GS_CLEAR, GS_KERNEL, GS_SPLITK_REDUCE, GS_COLSUM_REDUCE };
struct GemmPlan {
  int rc = 0;  // 0: run the steps; -1: not taken (bad arguments); 1: a removed implementation
  int nsteps = 0;
  int steps[3] = {GS_NONE, GS_NONE, GS_NONE};
  // the GS_KERNEL step
  GemmKernelId kernel = {GK_NONE, {0, 0, 0, 0, 0, 0, 0, 0}};
  unsigned grid = 0, block = 0;
  unsigned long long a_bytes = 0, b_bytes = 0;  // bytes a tile load may touch (buffer descriptors)
  G7Plan g7 = {};                               // persistent families only
  // dispatcher-owned argument edits
  int ksplit = 0, nt_store = 0;
  bool drop_ws = false;  // ws nulled: the column-sum partials do not fit, the epilogue uses atomics
  // the reduction step's grid
  unsigned red_x = 0, red_y = 0;
  int last_kernel = 0;  // dpc_gemm_last_kernel(): 900 + EPI v9, 700 + EPI v7 (+ 50: v8, v7d), 0 v1-v3
};

namespace plan_detail {

inline bool al(const void* p, int b) { return ((uintptr_t)p % (uintptr_t)b) == 0; }

// bytes a tile load may legitimately touch: [rows][ld], 16-B chunks up to roundup8(cols)
inline long long operand_bytes(long long rows, long long cols, long long ld) {
  if (rows <= 0 || cols <= 0) return 0;
  return ((rows - 1) * ld + ((cols + 7) / 8) * 8) * 2;
}

inline int policy_impl(const GemmArgs& a, const GemmSettings& st) {
  if (a.a_kmaj && a.b_kmaj) return st.policy[a.K <= 1024 ? 0 : 1];
  if (a.a_kmaj) return st.policy[a.K <= 2304 ? 2 : 3];
  if (!a.b_kmaj) return st.policy[4];
  return 0;
}

inline bool plain_epilogue(const GemmArgs& a) {
  return !a.bias && !a.residual && !a.aux_in && !a.aux_out && !a.colsum && !a.act && !a.act_bwd;
}

// An mn-major operand holds every logical row of the product as a column.  The descriptor-bounded
// loads (v2 / v3 and the persistent families) end an operand at its last byte, not at the end of a
// stored row: the columns past a_c (b_c) of a k-row are whatever follows them in memory, which
// only the register-staged kernel's predicates read as zeros.
inline bool mn_cols_ok(const GemmArgs& a) { return (a.a_kmaj || a.a_c >= a.M) && (a.b_kmaj || a.b_c >= a.N); }

// v2 / v3 requirements: a k-major operand must hold exactly K (% 64) columns (its k-tail is not
// zeroed by the descriptor), an mn-major one every logical column (mn_cols_ok), N % 4 == 0 and
// 16-B aligned f32 epilogue operands (vector epilogue), every operand inside a 31-bit byte range.
inline bool gemm2_ok(const GemmArgs& a) {
  const bool kmaj_ok = (!a.a_kmaj || (a.a_c == a.K && a.K % 64 == 0)) && (!a.b_kmaj || (a.b_c == a.K && a.K % 64 == 0)) &&
                       mn_cols_ok(a);
  return kmaj_ok && a.N % 4 == 0 && operand_bytes(a.a_r, a.a_c, a.lda) > 0 && operand_bytes(a.b_r, a.b_c, a.ldb) > 0 &&
         a.K > 0 && a.ldc % 4 == 0 && a.ldr % 4 == 0 && a.ld_aux_in % 4 == 0 && a.ld_aux_out % 4 == 0 &&
         al(a.C, a.out_f32 ? 16 : 8) && al(a.bias, 16) && al(a.residual, 16) && al(a.aux_in, 8) && al(a.aux_out, 8) &&
         al(a.colsum, 4);
}

// Whether the persistent families take this product: k-major operands hold exactly K columns
// with K % 32 == 0 (a slice never straddles a row end; mn-major operands end at row K, so their
// last slice reads zeros past it, and hold every logical column: mn_cols_ok), N % 8 == 0, 16-B
// aligned C / bias / residual, 8-B aligned aux.
inline bool gemm7_ok(const GemmArgs& a) {
  const bool kmaj_ok = (!a.a_kmaj || (a.a_c == a.K && a.K % 32 == 0)) && (!a.b_kmaj || (a.b_c == a.K && a.K % 32 == 0)) &&
                       (a.a_kmaj || a.a_r == a.K) && (a.b_kmaj || a.b_r == a.K) && mn_cols_ok(a);
  return kmaj_ok && a.K > 0 && operand_bytes(a.a_r, a.a_c, a.lda) > 0 && operand_bytes(a.b_r, a.b_c, a.ldb) > 0 &&
         a.N % 8 == 0 && a.ldc % 8 == 0 && a.ldr % 4 == 0 && a.ld_aux_in % 4 == 0 && a.ld_aux_out % 4 == 0 &&
         al(a.C, 16) && al(a.bias, 16) && al(a.residual, 16) && al(a.aux_in, 8) && al(a.aux_out, 8) && al(a.colsum, 4);
}

// SCHED 3 / 4 / 6 pre-bias the voffset of the k-th piece of a group by -k KiB: it must hold that
// many bytes of rows before it (k-major: 16 rows per piece, mn-major: 4 k-rows per piece)
inline bool bias_ok(const GemmArgs& a, long long bytes = 1024) {
  auto ok = [bytes](bool kmaj, long long ld) { return kmaj ? ld * 2 * 16 >= bytes : ld * 2 * 4 >= bytes; };
  return ok(a.a_kmaj, a.lda) && ok(a.b_kmaj, a.ldb);
}

// The DMA schedule of every v7 / v8 kernel but the plain v7 one.  Two DMA pieces at the head of
// every even MFMA group, issued under one M0 write (SCHED 3) where the operands allow it, else
// one M0 write per piece (SCHED 2): +3 to +7 % on every GPT-2 product and on 8192^3 (1252 ->
// 1330 TF/s nt; profiles/r3_gemm/ab22_*).  v7 products with an mn-major operand (input and
// weight gradients) take the split interleave (SCHED 6: one M0 / DMA instruction per MFMA gap):
// +4..8 % on nn and tn (8192^3 nn 1331 -> 1409, tn 1335 -> 1437 TF/s), within 1 % on nt
// (profiles/r3_gemm/lab_sched6.log).
inline int gemm7_sched(const GemmArgs& a, int wn) {
  if (!bias_ok(a)) return 2;
  return wn == 128 && (!a.a_kmaj || !a.b_kmaj) ? 6 : 3;
}

// The plain v7 kernel (EPI 0) is built for every placement an id can ask for.  The grouped-M0
// forms replace the per-piece ones: dma 0 / 2 (one or two pieces per group) -> pairs (3), dma 1
// (four pieces at groups 0 and 4) -> quads (4); every placement gives way to the split
// interleave when an operand is mn-major (it beat each of them there).
inline int gemm7_sched_plain(const GemmArgs& a, int dma) {
  if ((dma == 6 || !a.a_kmaj || !a.b_kmaj) && bias_ok(a)) return 6;
  if ((dma == 4 || dma == 1) && bias_ok(a, 3072)) return 4;
  if (dma == 1) return 1;
  if (bias_ok(a)) return 3;
  return dma == 2 ? 2 : 0;
}

inline void add_step(GemmPlan& p, int step) { p.steps[p.nsteps++] = step; }

inline void set_kernel7(GemmPlan& p, const GemmArgs& a, int epi, int sched, int wn) {
  p.kernel = {GK_V7, {epi, sched, a.a_kmaj != 0, a.b_kmaj != 0, wn, 0, 0, 0}};
  p.last_kernel = 700 + epi + (wn == 64 ? 50 : 0);
}

// v9 runs 64-deep stages: the slices of v7's plan recounted (the split count stays)
inline void set_kernel9(GemmPlan& p, const GemmArgs& a, int epi, int er) {
  p.kernel = {GK_V9, {epi, a.a_kmaj != 0, a.b_kmaj != 0, 0, er, 0, 0, 0}};
  p.last_kernel = 900 + epi;
  p.g7.nk_all = (a.K + 63) / 64;
  p.g7.nk = (p.g7.nk_all + p.g7.splits - 1) / p.g7.splits;
}

inline void add_splitk_reduce(GemmPlan& p, const GemmArgs& a) {
  const long long nq = (long long)a.M * (a.N / 4);
  p.red_x = (unsigned)std::min<long long>((nq + 255) / 256, 4096);
  p.red_y = 1;
  add_step(p, GS_SPLITK_REDUCE);
}

// The persistent families (v7 / v8 / v7d / v9).  False: the product does not meet their
// requirements and the caller falls back to v2 / v1.
inline bool plan7(const GemmArgs& a, const GemmSettings& st, const GemmImpl& row, GemmPlan& p) {
  if (!gemm7_ok(a)) return false;
  const bool v8 = row.family == GF_V8;
  const int dma = row.dma;
  G7Plan& pl = p.g7;
  pl = G7Plan{};
  pl.tile_n = row.tile_n;
  pl.tiles_m = (a.M + 255) / 256;
  pl.tiles_n = (a.N + pl.tile_n - 1) / pl.tile_n;
  const int tiles = pl.tiles_m * pl.tiles_n;
  pl.nk_all = (a.K + GP_G7_KB - 1) / GP_G7_KB;
  const bool plain = !a.bias && !a.act_bwd && !a.aux_out && !a.act && !a.residual && !a.colsum;
  const bool splittable = plain && a.out_f32;
  // splits: forced (> 0), else automatic for plain f32 products only: the tiles are too few to
  // fill the chip, e.g. weight gradients -- K = tokens, M x N = a weight
  int s = st.force_splits > 0 ? st.force_splits : 1;
  auto slab_fits = [&](int c) {
    return a.ws && (long long)c * a.M * a.N * 4 <= a.ws_bytes && a.ldc % 4 == 0 && al(a.ws, 16);
  };
  const int cus = std::max(8, st.cus - st.cu_reserve);  // CUs the grid may occupy
  if (st.force_splits <= 0 && splittable) {
    // fill the chip (few tiles) or even out the last round (wave quantisation): time ~ rounds
    // * (slices per unit + the split epilogue) [+ the slab reduction].  Units are in k-slices
    // (~0.7 us at the measured MFMA rate).  The split epilogue: 256 KiB of f32 adds per CU at
    // the chip's memory-side atomic rate, ~40 slices, or the same bytes as plain slab stores,
    // ~12, plus a reduction pass over (c + 1) M x N f32 at ~5 TB/s.
    double best = 1e30;
    for (int c = 1; c <= 32; ++c) {
      const int per = 2 * ((pl.nk_all + 2 * c - 1) / (2 * c));
      if (c > 1 && per < 16) break;
      // (v8: two 256 x 128 units per CU at once, each half a v7 unit's MFMA work)
      const int rounds = v8 ? (tiles * c + 2 * cus - 1) / (2 * cus) : (tiles * c + cus - 1) / cus;
      double cost = (double)rounds * per;
      if (c > 1 && slab_fits(c)) {
        const double red_us = (double)(c + 1 + a.accumulate) * a.M * a.N * 4 / 5e6;
        cost += rounds * 12.0 + red_us / 0.7;
      } else if (c > 1) {
        if (v8) continue;  // v8 splits through workspace slabs only (no atomic epilogue)
        cost += rounds * 40.0;
      }
      if (cost < best - 1e-9) { best = cost; s = c; }
    }
  }
  if (s > 1 && (!splittable || (v8 && !slab_fits(s)))) return false;
  // slab split (workspace for every k-range's partial tile) when the caller passed one that is
  // large enough; otherwise f32 atomics into C
  const bool slab = s > 1 && slab_fits(s);
  // the input-gradient epilogue (act', column sums) carries no forward operation
  if ((a.act_bwd || a.colsum) && (a.bias || a.act || a.aux_out || a.residual || a.accumulate)) return false;
  pl.splits = s;
  pl.nk = 2 * ((pl.nk_all + 2 * s - 1) / (2 * s));  // even: a unit starts on register set 0
  pl.units = tiles * s;
  const int slots = v8 ? 2 * cus : cus;  // workgroups resident at once
  pl.grid = (row.persistent && pl.units > slots) ? slots : pl.units;
  // vector-memory ops an epilogue issues per lane, for the store credit: only epilogues that
  // read nothing per element and issue every store of a full tile (no column-sum atomics)
  const bool no_loads = !a.residual && !a.act_bwd && !a.accumulate && !a.colsum;
  pl.store_cnt = (no_loads && (s == 1 || slab) && !v8) ? ((a.out_f32 || slab ? 64 : 32) + (a.aux_out ? 32 : 0)) : 0;
  pl.debug = 0;
  p.grid = (unsigned)pl.grid;
  p.block = 256;
  p.steps[0] = p.steps[1] = p.steps[2] = GS_NONE;
  p.nsteps = 0;
  p.drop_ws = false;

  // v7d (id 24): the GELU / GELU' fused epilogues of full-depth products (nk >= 18: at least 16
  // slices to spread a tile's deferred chunks over), the forward forms with both operands
  // k-major, the input-gradient form with A k-major, B n-major; paired-M0 DMA
  if (row.family == GF_V7D && s == 1 && pl.nk >= 18 && bias_ok(a)) {
    const bool fwd = a.act == GP_ACT_GELU && a.aux_out && !a.aux_deriv && !a.accumulate && !a.act_bwd && !a.colsum &&
                     a.ld_aux_out % 8 == 0 && al(a.aux_out, 16) && a.a_kmaj && a.b_kmaj;
    const bool up = fwd && !a.residual && !a.out_f32;
    // (residual may alias C: a chunk is read, then written, by one lane)
    const bool down = fwd && a.residual && a.out_f32 && a.ldr % 4 == 0 && al(a.residual, 16) && pl.nk >= 34;
    const bool bwd = a.act_bwd == GP_ACT_GELU && a.aux_in && !a.out_f32 && !a.accumulate && !a.bias && !a.act &&
                     !a.aux_out && !a.residual && a.ld_aux_in % 8 == 0 && al(a.aux_in, 16) && a.a_kmaj && !a.b_kmaj;
    const int epi = up ? 5 : down ? 7 : bwd ? 6 : 0;
    if (epi) {
      p.kernel = {GK_V7D, {epi, 3, a.a_kmaj != 0, a.b_kmaj != 0, 0, 0, 0, 0}};
      p.last_kernel = 750 + epi;
      add_step(p, GS_KERNEL);
      return true;
    }
  }
  // v9, always with the early-release schedule (gemm9_kern.h ER = 4: +2..5 % on the GPT-2 nt
  // products, profiles/r4_er/; forward epilogue +2 %, profiles/r4_g9/)
  if (!v8 && a.K % 64 == 0 && s == 1 && !a.accumulate && a.a_kmaj && a.lda >= 64) {
    // plain nt products -- every GPT-2 forward projection -- whatever v7 placement was asked
    // for (but the forced split interleave and v7d): +0.7..+8.7 % over v7 (8192^3 1383 -> 1429,
    // out-projection 1045 -> 1136 TF/s; profiles/r3_gemm/lab_v9.log)
    const bool nt = plain && a.b_kmaj && a.ldb >= 64 && dma != 6 && dma != 5;
    // plain input gradients (B mn-major) only when asked for (id 26): against v7's split
    // interleave +4-5 % on the out-projection input gradients (K = N = D), -1..-3 % on the
    // others (profiles/r4_g9/ab_*.log), so the table gives it the square ones
    const bool km = plain && !a.b_kmaj && a.ldb >= 128 && dma == 7;
    // forward epilogues that read nothing per element (bias / activation / aux_out, no residual:
    // the FFN up-projection) when asked for (id 26): the 2 x 32 bf16 stores of a tile stay in
    // flight into the next tile's stages
    const bool fwd = !plain && !a.residual && !a.act_bwd && !a.colsum && a.b_kmaj && a.K >= 192 && a.ldb >= 64 &&
                     (!a.aux_out || (a.ld_aux_out % 8 == 0 && al(a.aux_out, 16))) && dma == 7;
    if (nt || km || fwd) {
      set_kernel9(p, a, fwd ? 1 : 0, 4);
      add_step(p, GS_KERNEL);
      return true;
    }
  }
  // weight gradients (both operands mn-major, split K through workspace slabs) on v9 only when
  // asked for (id 26): measured SLOWER than v7's split interleave (GPT-2 small QKV / up weight
  // gradients 0.205 -> 0.216 / 0.269 -> 0.285 ms; profiles/r3_gemm/v9_wgrad_negative.txt) -- the
  // mn-major pieces were whole lines already, and the two-buffer ring leaves the HBM-streamed
  // operands less latency slack
  if (slab && !v8 && !a.a_kmaj && !a.b_kmaj && a.lda >= 128 && a.ldb >= 128 && dma == 7) {
    set_kernel9(p, a, 4, 0);
    add_step(p, GS_KERNEL);
    add_splitk_reduce(p, a);
    return true;
  }
  const int wn = v8 ? 64 : 128;
  if (slab) {
    set_kernel7(p, a, 4, gemm7_sched(a, wn), wn);
    add_step(p, GS_KERNEL);
    add_splitk_reduce(p, a);
  } else if (s > 1) {
    if (!a.accumulate) add_step(p, GS_CLEAR);
    set_kernel7(p, a, 2, gemm7_sched(a, 128), 128);
    add_step(p, GS_KERNEL);
  } else if (v8) {
    set_kernel7(p, a, plain && !a.accumulate ? 0 : (!a.act_bwd && !a.colsum ? 1 : 3), gemm7_sched(a, 64), 64);
    add_step(p, GS_KERNEL);
  } else if (plain && !a.accumulate) {
    set_kernel7(p, a, 0, gemm7_sched_plain(a, dma), 128);
    add_step(p, GS_KERNEL);
  } else if (!a.act_bwd && !a.colsum) {
    // forward epilogue with an f32 residual into an f32 output: the residual staged through LDS
    // (g7_epilogue_res_lds, EPI 9)
    const bool res_lds = (st.res_lds >= 0 ? st.res_lds : st.res_lds_env) && a.residual && a.out_f32 && !a.aux_deriv &&
                         !a.accumulate && a.ldr % 4 == 0 && al(a.residual, 16) && a.ldr <= (1 << 20);
    set_kernel7(p, a, res_lds ? 9 : 1, gemm7_sched(a, 128), 128);
    add_step(p, GS_KERNEL);
  } else {
    // input-gradient epilogue with an act' operand: the operand staged through LDS by DMA
    // (g7_epilogue_act_lds, EPI 8; EPI 10 = ACT_MUL, compiled for the default store policy only
    // -- another policy takes EPI 3)
    const bool act_lds = (st.act_lds >= 0 ? st.act_lds : st.act_lds_env) && a.act_bwd && a.aux_in && !a.out_f32 &&
                         a.ld_aux_in % 8 == 0 && (a.act_bwd != GP_ACT_MUL || ((st.nt_store >> 2) & 3) == 3) &&
                         al(a.aux_in, 16) && a.ld_aux_in <= (1 << 20);
    if (act_lds) {
      // column sums through the workspace ([2 tiles_m][N] partials + g7_colsum_reduce) when the
      // caller passed one large enough, else f32 atomics from the epilogue
      const long long rows = 2ll * pl.tiles_m;
      const bool cs_ws = a.colsum && a.ws && rows * a.N * 4 <= a.ws_bytes && al(a.ws, 16) && a.N % 4 == 0 &&
                         al(a.colsum, 16);
      p.drop_ws = a.ws && !cs_ws;
      set_kernel7(p, a, a.act_bwd == GP_ACT_MUL ? 10 : 8, gemm7_sched(a, 128), 128);
      add_step(p, GS_KERNEL);
      if (cs_ws) {
        p.red_x = (unsigned)((a.N / 4 + 255) / 256);
        p.red_y = (unsigned)((rows + 15) / 16);
        add_step(p, GS_COLSUM_REDUCE);
      }
    } else {
      set_kernel7(p, a, 3, gemm7_sched(a, 128), 128);
      add_step(p, GS_KERNEL);
    }
  }
  return true;
}

// v1 - v3: one workgroup per 128x128 / 256x128 tile (and k-range)
inline void plan123(const GemmArgs& a, const GemmSettings& st, const GemmImpl& row, GemmPlan& p) {
  p.g7 = G7Plan{};
  p.last_kernel = 0;
  p.nsteps = 0;
  p.drop_ws = false;
  const int ak = a.a_kmaj != 0, bk = a.b_kmaj != 0;
  if (row.family == GF_V1) {
    p.kernel = {GK_V1, {ak, bk, 0, 0, 0, 0, 0, 0}};
    p.grid = (unsigned)(((a.M + 127) / 128) * ((a.N + 127) / 128));
    p.block = 256;
    add_step(p, GS_KERNEL);
    return;
  }
  const int t = ((a.M + row.tile_m - 1) / row.tile_m) * ((a.N + row.tile_n - 1) / row.tile_n);
  const int nk = (a.K + 63) / 64;
  int splits = 1;
  // plain f32 products (weight gradients: small M x N, K = tokens) are split along K
  if (a.out_f32 && plain_epilogue(a)) {
    // Split-K count from a cost model fitted to the GPT-2 weight-gradient sweep on MI355X
    // (bench/wgrad_splits.py, profiles/r1_wgrad_splits.txt): time ~ rounds(s) / s + beta * s,
    // rounds = ceil(tiles * s / resident workgroups) (wave quantisation of the grid) and
    // beta * s the split-K partial-sum atomics relative to the K-proportional MFMA work.
    const int slots = 256 * row.wgs;
    const double beta = 0.0056 * 32768.0 / (double)a.K;
    double best = 1e30;
    for (int s = 1; s <= 16 && (s == 1 || nk / s >= 8); ++s) {
      const long long rounds = ((long long)t * s + slots - 1) / slots;
      const double cost = (double)rounds / s + beta * s;
      if (cost < best - 1e-9) { best = cost; splits = s; }
    }
    if (st.force_splits > 0) splits = st.force_splits;
  }
  if (splits > 1 && !a.accumulate) add_step(p, GS_CLEAR);
  p.grid = (unsigned)(t * splits);  // 1-D: tile_slot() maps block -> (split, tile)
  p.ksplit = splits > 1 ? (st.xcd_split ? -splits : splits) : 0;
  if (row.family == GF_V2) {
    p.kernel = {GK_V2, {row.kb, row.stages, ak, bk, 0, 0, 0, 0}};
    p.block = 256;
  } else {
    p.kernel = {GK_V3, {row.tile_m, row.tile_n, 4, 2, row.kb, row.stages, ak, bk}};
    p.block = 512;
  }
  add_step(p, GS_KERNEL);
}

}  // namespace plan_detail

inline GemmPlan gemm_plan(const GemmArgs& a, const GemmSettings& st) {
  using namespace plan_detail;
  GemmPlan p;
  if (a.M <= 0 || a.N <= 0) return p;
  // aux_deriv: GELU' as the second output (v9 / v7 / v2 / v3 epilogues; v7d and the LDS-staged
  // residual epilogue skip it)
  if (a.aux_deriv && (!a.aux_out || a.act != GP_ACT_GELU)) { p.rc = -1; return p; }
  p.a_bytes = (unsigned long long)operand_bytes(a.a_r, a.a_c, a.lda);
  p.b_bytes = (unsigned long long)operand_bytes(a.b_r, a.b_c, a.ldb);
  p.nt_store = st.nt_store;
  const bool v2_ok = gemm2_ok(a);
  const bool plain = plain_epilogue(a);
  const int pol = policy_impl(a, st);
  // a forced global id, else the caller's (the measured per-shape table), else the shape policy
  int impl = st.impl;
  if (impl < 0 && a.impl > 0) impl = a.impl;
  if (impl < 0 && pol <= 0 && gemm7_ok(a)) {
    // products without a fused epilogue -- the QKV / out / LM-head forward, every input
    // gradient without act', the weight gradients (split K) -- run the persistent 4-wave
    // kernel (v7); GPT-2 small B=64 shapes on MI355X: 940-1,220 TF/s vs 640-940 for the
    // 8-wave / 128-wide kernels (bench/gemm_ab.py, profiles/r2_gemm/)
    if (plain) impl = 20;
    // forward epilogues that read nothing per element (bias / activation / aux_out: the FFN
    // products, whose table entries all name v9) take v9's load-free epilogue when no table
    // entry covers the shape -- e.g. the down projection as a bias-only product (its residual add
    // moved into the next LayerNorm), which the older policy sent to the 128 x 128 kernel at
    // 366 us against ~280
    else if (a.a_kmaj && a.b_kmaj && !a.residual && !a.accumulate && !a.aux_in && !a.colsum && !a.act_bwd &&
             a.K % 64 == 0 && a.K >= 192)
      impl = 26;
  }
  if (impl < 0) {
    // Default per operand layout and depth, from the GPT-2 shape sweep on MI355X
    // (bench/kernels.py, profiles/kernels_r1_*.json): forward products with a short K
    // (<= 1024) are epilogue/prologue heavy and run best as 256x128 tiles two workgroups
    // per CU (10); deep or mn-major products keep the 128x128 2-stage kernel (2), except
    // dgrad at K <= 2304 and mid-size wgrad, where the 3-stage 32-deep ring wins.
    impl = 1;
    if (v2_ok) {
      impl = 2;
      if (a.a_kmaj && a.b_kmaj && a.K <= 1024) impl = 10;
      else if (a.a_kmaj && !a.b_kmaj && a.K <= 1024) impl = 10;  // dgrad + act' / colsum epilogue
      else if (a.a_kmaj && !a.b_kmaj && a.K <= 2304) impl = 4;
      else if (!a.a_kmaj && !a.b_kmaj && a.M > 2304 && a.M <= 4096) impl = 4;
      if (pol > 0) impl = pol;
    }
  }
  // a weight gradient the policy decides: the split-K persistent kernel (chosen above when its
  // requirements hold -- its planner splits K to fill the chip however few tiles there are), else
  // the 2-stage 64-k kernel.  (An off-table 1024 x 1024 x 16368 out-projection weight gradient
  // once fell to the 2-stage kernel at 506 TF/s, profiles/r4_pp/.)
  if (st.impl < 0 && a.impl <= 0 && v2_ok && plain && a.out_f32 && !a.a_kmaj && !a.b_kmaj && pol <= 0 && impl != 20)
    impl = 2;
  if (impl < 2) impl = 1;  // (a forced 0 runs the fallback, as 1 does)
  const GemmImpl* row = gemm_impl_row(impl);
  if (row && row->family >= GF_V7) {
    if (plan7(a, st, *row, p)) return p;
    row = gemm_impl_row(2);  // requirements not met: the 128x128 kernels
  }
  if (!row) { p.rc = 1; return p; }  // a removed implementation
  if (!v2_ok) row = gemm_impl_row(1);
  plan123(a, st, *row, p);
  return p;
}

// One line of text: "<step>; <step> | last=<dpc_gemm_last_kernel code>" ("rc=<n>" for the steps when not 0)
inline int gemm_plan_text(const GemmPlan& p, char* buf, int cap) {
  int n = 0;
  auto put = [&](const char* fmt, auto... v) {
    if (n < cap) n += snprintf(buf + n, (size_t)(cap - n), fmt, v...);
  };
  auto puts = [&](const char* s) { put("%s", s); };
  auto tf = [](int v) { return v ? "true" : "false"; };
  if (p.rc) put("rc=%d", p.rc);
  for (int i = 0; i < p.nsteps; ++i) {
    if (i) puts("; ");
    const GemmKernelId& k = p.kernel;
    const G7Plan& g = p.g7;
    switch (p.steps[i]) {
      case GS_CLEAR: puts("clear"); break;
      case GS_SPLITK_REDUCE: put("splitk_reduce grid=%u", p.red_x); break;
      case GS_COLSUM_REDUCE: put("colsum_reduce grid=%ux%u", p.red_x, p.red_y); break;
      case GS_KERNEL:
        if (k.family == GK_V1) put("gemm_kernel<%s, %s>", tf(k.t[0]), tf(k.t[1]));
        else if (k.family == GK_V2) put("gemm2_kernel<%d, %d, %s, %s>", k.t[0], k.t[1], tf(k.t[2]), tf(k.t[3]));
        else if (k.family == GK_V3)
          put("gemm3_kernel<%d, %d, %d, %d, %d, %d, %s, %s>", k.t[0], k.t[1], k.t[2], k.t[3], k.t[4], k.t[5], tf(k.t[6]), tf(k.t[7]));
        else if (k.family == GK_V7) put("gemm7_kernel<%d, %d, %s, %s, %d, %d>", k.t[0], k.t[1], tf(k.t[2]), tf(k.t[3]), k.t[4], k.t[5]);
        else if (k.family == GK_V7D) put("gemm7d_kernel<%d, %d, %s, %s>", k.t[0], k.t[1], tf(k.t[2]), tf(k.t[3]));
        else put("gemm9_kernel<%d, %s, %s, %d, %d>", k.t[0], tf(k.t[1]), tf(k.t[2]), k.t[3], k.t[4]);
        // the persistent families' grid is G7Plan::grid; what has its default value is left out
        if (k.family >= GK_V7)
          put(" g7=%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", g.tiles_m, g.tiles_n, g.tile_n, g.units, g.grid, g.nk, g.nk_all, g.splits,
              g.store_cnt, g.debug);
        else put(" grid=%u", p.grid);
        if (p.block != 256) put(" block=%u", p.block);
        if (p.ksplit) put(" ksplit=%d", p.ksplit);
        if (p.nt_store != 77) put(" nt=%d", p.nt_store);
        if (p.drop_ws) puts(" wsdrop");
        break;
      default: break;
    }
  }
  put(" | last=%d", p.last_kernel);
  return n < cap ? n : cap - 1;
}

}  // namespace dpc
