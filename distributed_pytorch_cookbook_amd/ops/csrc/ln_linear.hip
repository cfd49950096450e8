// LayerNorm fused into the few-row Linear that consumes it -- one launch where the one-token decode
// step had two (LN1 + QKV, LN2 + up-projection, final norm + LM head):
//   y[m, n] = act(LN(x[m, :]) . w[n, :] (* scale[n]) + bias[n]) (+ residual[m, n]),  1 <= M <= 32,
//   LN(x)[k] = bf16((x[k] - mean) * rstd * gamma[k] + beta[k]),  rstd = 1 / sqrt(var + eps),
// x the f32 residual stream, gamma / beta f32, w bf16 [Nw][ldw] or raw e4m3 bytes with one f32 scale
// per output row (wq_gemm.hip's QWeight).  The epilogue contract is that of dpc_gemm_skinny and
// dpc_gemm_wq8: f32 bias, activation codes, f32 residual, bf16 or f32 y, columns Nw <= n < N
// written as 0, no float atomics and a fixed summation order (two calls, same bits).
//
// ln_linear_kernel<RB, CB, NW, FP8>, grid ceil(N / (16 CB)), NW waves, dynamic LDS.
//   * The split of the few-row kernels: a workgroup owns a strip of 16 CB output columns and all M
//     rows (RB = ceil(M / 16) row blocks), its NW waves split K step by step, the partials are
//     summed through LDS in wave order, accumulator a by wave a % NW, then one epilogue.
//   * Before anything else a wave requests the weights of its first step: they are in flight
//     while the rows are normalised.
//   * Statistics: wave v takes rows v, v + NW, ...  A row lives in registers (8 float4 per lane,
//     K <= 2048; chunks past that are read again in every pass): the sum, then the sum of squared
//     differences from the mean -- two passes, each reduced by the __shfl_xor butterfly.  The
//     order of every sum is ln_fwd_kernel's (layernorm.hip), so for K <= 2048 the normalised row
//     is the one that kernel writes.
//   * The row is normalised, scaled, shifted, rounded to bf16 once and stored in LDS as
//     [M][K + pad] (global x is read once per workgroup).  pad is 8 or 16 elements, whichever makes
//     the row stride an ODD number of 16-byte units: the main loop's read is 16 lanes, 16
//     consecutive rows, one k -- 16 different 16-byte slots of the 256 bytes the banks cover.
//     Row blocks past M read row M - 1 (clamped, not masked: they feed rows that are never stored).
//   * Main loop: the weights go from global memory straight into MFMA registers (A operand of
//     v_mfma_f32_16x16x32_bf16), the next step's loads issued before the current step's MFMAs; the
//     B operand is a 16-byte LDS read.  bf16 weights: a step is 64 k (lane (r, q) holds k0 + 16 q ..
//     + 15 of its weight rows, two MFMAs per accumulator).  e4m3: 128 k (32 bytes per lane, widened
//     by fp8_to_bf16x4, four MFMAs); the scale meets the summed accumulator ahead of the bias.
//     The one step that K cuts short runs with its chunks at or past K zeroed in both operands.
//
// LDS: M (K + pad) 2 bytes of image + NW CB RB 1 KiB of partials, at most 160 KiB: 32 rows up to
// K = 2288, 16 rows up to K = 4848.  The host refuses anything else (hipErrorInvalidValue).
//
// Plans (columns, waves): (16, 8) and (32, 4), from ops/gemm.py:skinny_plan unless forced.
//
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950, no scratch in any instantiation),
// VGPRs of ln_linear_kernel<RB, CB, NW, FP8>:
//   bf16  CB 1, NW 8:  RB 1: 114   RB 2: 114      CB 2, NW 4:  RB 1: 124   RB 2: 124
//   e4m3  CB 1, NW 8:  RB 1: 117   RB 2: 117      CB 2, NW 4:  RB 1: 127   RB 2: 127
// (the row held across the two sums decides them, not the accumulators; gamma and beta are read
// in the last pass, from L2: held across the sums they cost 64 more and a workgroup per CU).
#include "common.h"
#include "fp8.h"

namespace dpc {

struct LnLinearArgs {
  const float* x;         // [M][ldx] f32
  const float* gamma;     // [K] f32
  const float* beta;      // [K] f32
  const void* w;          // [Nw][ldw] bf16 or e4m3 bytes, k contiguous
  const float* scale;     // [Nw] f32 with e4m3 weights, else null
  const float* bias;      // [Nw] f32 or null
  const float* residual;  // [M][ldr] f32 or null
  void* y;                // [M][ldy] bf16 or f32
  long long ldx, ldw, ldr, ldy;
  int M, N, Nw, K;
  float eps;
  int act, y_f32;
  int nb, nw;             // the plan: (16, 8) or (32, 4)
};

constexpr int LNL_NV = 8;                  // float4 per lane of a row held in registers
constexpr int LNL_LDS_BYTES = 160 * 1024;  // a gfx950 workgroup's LDS

// the image's row stride in elements: an odd number of 16-byte units
__host__ __device__ inline int lnl_ld(int K) { return K + ((K / 8) % 2 == 0 ? 8 : 16); }

// one step's weights of a lane: per column block two 16-byte chunks (16 k bf16, 32 k e4m3)
template <int CB>
struct LnlW {
  uint4 w[CB][2];
};

// ES: bytes per weight element.  TAIL: chunks at or past K are read from k = 0 instead and zeroed
template <int CB, int ES, bool TAIL>
__device__ __forceinline__ void lnl_load_w(LnlW<CB>& f, const unsigned char* const* wrow, int k, int K) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int kh = k + h * (16 / ES);
    const bool ok = !TAIL || kh < K;
    const int kk = ok ? kh : 0;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      f.w[c][h] = *reinterpret_cast<const uint4*>(wrow[c] + (long long)kk * ES);
      if (TAIL && !ok) f.w[c][h] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// the NX 16-byte chunks (8 k each) of the image under a lane's weights
template <int RB, int NX, bool TAIL>
__device__ __forceinline__ void lnl_load_x(uint4 (&x)[RB][NX], const bf16_t* const* xrow, int k, int K) {
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    const bool ok = !TAIL || k + 8 * j < K;
    const int kk = ok ? k + 8 * j : 0;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      x[r][j] = *reinterpret_cast<const uint4*>(xrow[r] + kk);
      if (TAIL && !ok) x[r][j] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// 8 e4m3 (two dwords) -> one bf16x8 operand
__device__ __forceinline__ bf16x8 lnl_widen8(unsigned lo, unsigned hi) {
  const uint2 a = fp8_to_bf16x4(lo), b = fp8_to_bf16x4(hi);
  return __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, b.x, b.y));
}

template <int RB, int CB, bool FP8>
__device__ __forceinline__ void lnl_mma(floatx4 (&acc)[CB][RB], const LnlW<CB>& f, const uint4 (&x)[RB][FP8 ? 4 : 2]) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      if constexpr (FP8) {
        const bf16x8 a0 = lnl_widen8(f.w[c][h].x, f.w[c][h].y), a1 = lnl_widen8(f.w[c][h].z, f.w[c][h].w);
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          acc[c][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, __builtin_bit_cast(bf16x8, x[r][2 * h]), acc[c][r], 0, 0, 0);
          acc[c][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, __builtin_bit_cast(bf16x8, x[r][2 * h + 1]), acc[c][r], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int r = 0; r < RB; ++r)
          acc[c][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, f.w[c][h]),
                                                              __builtin_bit_cast(bf16x8, x[r][h]), acc[c][r], 0, 0, 0);
      }
    }
}

// rows wv, wv + NW, ... of x, normalised into the image (one wave per row)
template <int NW>
__device__ __forceinline__ void lnl_normalise(const LnLinearArgs& p, bf16_t* img, int ldl, int lane, int wv) {
  const int nv4 = p.K >> 2;
  if (wv >= p.M) return;
  const float4* g4 = reinterpret_cast<const float4*>(p.gamma);
  const float4* b4 = reinterpret_cast<const float4*>(p.beta);
  for (int m = wv; m < p.M; m += NW) {
    const float4* xr = reinterpret_cast<const float4*>(p.x + (long long)m * p.ldx);
    uint2* yr = reinterpret_cast<uint2*>(img + m * ldl);
    float4 v[LNL_NV];
#pragma unroll
    for (int i = 0; i < LNL_NV; ++i) v[i] = xr[min(lane + i * 64, nv4 - 1)];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LNL_NV; ++i) {
      if (lane + i * 64 >= nv4) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      s += v[i].x + v[i].y + v[i].z + v[i].w;
    }
    for (int c = lane + LNL_NV * 64; c < nv4; c += 64) {
      const float4 t = xr[c];
      s += t.x + t.y + t.z + t.w;
    }
    const float mu = wave_sum(s) / p.K;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < LNL_NV; ++i) {
      if (lane + i * 64 < nv4) {
        const float a = v[i].x - mu, b = v[i].y - mu, cc = v[i].z - mu, d = v[i].w - mu;
        ss += a * a + b * b + cc * cc + d * d;
      }
    }
    for (int c = lane + LNL_NV * 64; c < nv4; c += 64) {
      const float4 t = xr[c];
      const float a = t.x - mu, b = t.y - mu, cc = t.z - mu, d = t.w - mu;
      ss += a * a + b * b + cc * cc + d * d;
    }
    const float rs = rsqrtf(wave_sum(ss) / p.K + p.eps);
#pragma unroll
    for (int i = 0; i < LNL_NV; ++i) {
      const int c = lane + i * 64;
      if (c < nv4) {
        const float4 g = g4[c], b = b4[c];
        yr[c] = make_uint2(pack2bf((v[i].x - mu) * rs * g.x + b.x, (v[i].y - mu) * rs * g.y + b.y),
                           pack2bf((v[i].z - mu) * rs * g.z + b.z, (v[i].w - mu) * rs * g.w + b.w));
      }
    }
    for (int c = lane + LNL_NV * 64; c < nv4; c += 64) {
      const float4 t = xr[c], g = g4[c], b = b4[c];
      yr[c] = make_uint2(pack2bf((t.x - mu) * rs * g.x + b.x, (t.y - mu) * rs * g.y + b.y),
                         pack2bf((t.z - mu) * rs * g.z + b.z, (t.w - mu) * rs * g.w + b.w));
    }
  }
}

template <int RB, int CB, int NW, bool FP8>
__global__ __launch_bounds__(64 * NW) void ln_linear_kernel(LnLinearArgs p) {
  constexpr int ACC = CB * RB;
  constexpr int STEP = FP8 ? 128 : 64;  // k per wave step: 4 lane groups x 32 or 16
  constexpr int ES = FP8 ? 1 : 2, NX = STEP / 32;
  extern __shared__ uint4 lnl_smem[];
  const int ldl = lnl_ld(p.K);
  bf16_t* img = reinterpret_cast<bf16_t*>(lnl_smem);                       // [M][ldl]
  floatx4(*red)[ACC][64] = reinterpret_cast<floatx4(*)[ACC][64]>(img + p.M * ldl);  // [NW][ACC][64]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * (16 * CB);

  const unsigned char* wrow[CB];
  const bf16_t* xrow[RB];
#pragma unroll
  for (int c = 0; c < CB; ++c)
    wrow[c] = static_cast<const unsigned char*>(p.w) + (long long)min(n0 + c * 16 + r16, p.Nw - 1) * p.ldw * ES;
#pragma unroll
  for (int r = 0; r < RB; ++r) xrow[r] = img + min(r * 16 + r16, p.M - 1) * ldl;

  floatx4 acc[CB][RB];
#pragma unroll
  for (int c = 0; c < CB; ++c)
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[c][r] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int K = p.K, kl = q * (STEP / 4);
  int k0 = wv * STEP;
  LnlW<CB> wc;
  uint4 xs[RB][NX];
  // the first step's weights travel while the rows are normalised
  if (k0 + STEP <= K) lnl_load_w<CB, ES, false>(wc, wrow, k0 + kl, K);
  __builtin_amdgcn_sched_barrier(0);
  lnl_normalise<NW>(p, img, ldl, lane, wv);
  __syncthreads();

  // whole steps with a whole one after them, two per trip: the weight registers alternate (a copy
  // at the end of every step would wait for the next weights before the next x reads issue)
  while (k0 + NW * STEP + STEP <= K) {
    LnlW<CB> wn;
    lnl_load_x<RB, NX, false>(xs, xrow, k0 + kl, K);
    lnl_load_w<CB, ES, false>(wn, wrow, k0 + NW * STEP + kl, K);
    // the next step's weights issue before the MFMAs (left alone, the scheduler sinks each load
    // to its use)
    __builtin_amdgcn_sched_barrier(0);
    lnl_mma<RB, CB, FP8>(acc, wc, xs);
    k0 += NW * STEP;
    if (k0 + NW * STEP + STEP > K) {
      wc = wn;
      break;
    }
    lnl_load_x<RB, NX, false>(xs, xrow, k0 + kl, K);
    lnl_load_w<CB, ES, false>(wc, wrow, k0 + NW * STEP + kl, K);
    __builtin_amdgcn_sched_barrier(0);
    lnl_mma<RB, CB, FP8>(acc, wn, xs);
    k0 += NW * STEP;
  }
  if (k0 + STEP <= K) {  // the last whole step: its weights are here or on their way
    lnl_load_x<RB, NX, false>(xs, xrow, k0 + kl, K);
    __builtin_amdgcn_sched_barrier(0);
    lnl_mma<RB, CB, FP8>(acc, wc, xs);
    k0 += NW * STEP;
  }
  if (k0 < K) {  // the step K cuts short (one wave of the workgroup at most)
    lnl_load_x<RB, NX, true>(xs, xrow, k0 + kl, K);
    lnl_load_w<CB, ES, true>(wc, wrow, k0 + kl, K);
    __builtin_amdgcn_sched_barrier(0);
    lnl_mma<RB, CB, FP8>(acc, wc, xs);
  }

#pragma unroll
  for (int c = 0; c < CB; ++c)
#pragma unroll
    for (int r = 0; r < RB; ++r) red[wv][c * RB + r][lane] = acc[c][r];
  __syncthreads();

  // C/D map of 16x16x32 with the weights as A: weight row (column n of y) = 4 q + i, x row = r16
  const bool vec = (p.ldy % 4 == 0) && ((uintptr_t)p.y % 16 == 0);
  for (int a = wv; a < ACC; a += NW) {
    const int c = a / RB, r = a % RB;
    floatx4 s = red[0][a][lane];
#pragma unroll
    for (int v = 1; v < NW; ++v) s += red[v][a][lane];
    const int m = r * 16 + r16, n = n0 + c * 16 + 4 * q;
    if (m >= p.M || n >= p.N) continue;
    // (the scale, bias and residual loads issue together: columns past Nw read column Nw - 1)
    float sc[4] = {1.f, 1.f, 1.f, 1.f}, b[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
    if constexpr (FP8) {
#pragma unroll
      for (int i = 0; i < 4; ++i) sc[i] = p.scale[min(n + i, p.Nw - 1)];
    }
    if (p.bias) {
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = p.bias[min(n + i, p.Nw - 1)];
    }
    if (p.residual) {
#pragma unroll
      for (int i = 0; i < 4; ++i) rs[i] = p.residual[(long long)m * p.ldr + min(n + i, p.Nw - 1)];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float z = FP8 ? s[i] * sc[i] + b[i] : s[i] + b[i];
      v[i] = n + i < p.Nw ? act_fwd(z, p.act) + rs[i] : 0.f;
    }
    const long long o = (long long)m * p.ldy + n;
    if (vec && n + 3 < p.N) {
      if (p.y_f32) *reinterpret_cast<float4*>(static_cast<float*>(p.y) + o) = make_float4(v[0], v[1], v[2], v[3]);
      else *reinterpret_cast<uint2*>(static_cast<bf16_t*>(p.y) + o) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (n + i >= p.N) break;
        if (p.y_f32) static_cast<float*>(p.y)[o + i] = v[i];
        else static_cast<bf16_t*>(p.y)[o + i] = f2bf(v[i]);
      }
    }
  }
}

// image + partials of one workgroup
static long long lnl_lds_bytes(int M, int K, int nb, int nw) {
  const int acc = (nb / 16) * ((M + 15) / 16);
  return (long long)M * lnl_ld(K) * 2 + (long long)nw * acc * 64 * 16;
}

template <int RB, int CB, int NW, bool FP8>
static int lnl_launch_rb(const LnLinearArgs& a, hipStream_t stream) {
  const unsigned lds = (unsigned)lnl_lds_bytes(a.M, a.K, 16 * CB, NW);
  auto kern = ln_linear_kernel<RB, CB, NW, FP8>;
  if (lds > 64 * 1024) {  // above the default limit of a launch
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LNL_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid((unsigned)((a.N + 16 * CB - 1) / (16 * CB))), block(64 * NW);
  hipLaunchKernelGGL(kern, grid, block, lds, stream, a);
  return (int)hipGetLastError();
}

template <int CB, int NW>
static int lnl_launch(const LnLinearArgs& a, hipStream_t stream) {
  const bool two = a.M > 16;
  if (a.scale) return two ? lnl_launch_rb<2, CB, NW, true>(a, stream) : lnl_launch_rb<1, CB, NW, true>(a, stream);
  return two ? lnl_launch_rb<2, CB, NW, false>(a, stream) : lnl_launch_rb<1, CB, NW, false>(a, stream);
}

}  // namespace dpc

using namespace dpc;

// Requirements: 1 <= M <= 32, K % 8 == 0 (bf16 weights: scale null) or K % 16 == 0 (e4m3: scale
// set), x / gamma / beta / w 16-B aligned with 16-B aligned rows (ldx % 4 == 0, ldw % 8 == 0 bf16,
// % 16 == 0 e4m3), 1 <= Nw <= N <= ldy, Nw <= ldr with a residual, (nb, nw) one of (16, 8),
// (32, 4), and the image and the partials within a workgroup's LDS.
DPC_API int dpc_ln_linear(const LnLinearArgs* a, hipStream_t stream) {
  if (a->M <= 0 || a->N <= 0) return 0;
  const bool fp8 = a->scale != nullptr;
  if (a->M > 32 || a->K <= 0 || a->K % (fp8 ? 16 : 8) || a->ldx % 4 || a->ldw % (fp8 ? 16 : 8) || a->ldx < a->K ||
      a->ldw < a->K || a->Nw < 1 || a->Nw > a->N || a->N > a->ldy || (a->residual && a->ldr < a->Nw) || !a->gamma ||
      !a->beta || ((uintptr_t)a->x % 16) || ((uintptr_t)a->w % 16) || ((uintptr_t)a->gamma % 16) ||
      ((uintptr_t)a->beta % 16))
    return (int)hipErrorInvalidValue;
  const bool p16 = a->nb == 16 && a->nw == 8, p32 = a->nb == 32 && a->nw == 4;
  if (!(p16 || p32) || lnl_lds_bytes(a->M, a->K, a->nb, a->nw) > LNL_LDS_BYTES) return (int)hipErrorInvalidValue;
  return p16 ? lnl_launch<1, 8>(*a, stream) : lnl_launch<2, 4>(*a, stream);
}
