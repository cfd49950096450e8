// Weight-only FP8 (e4m3) Linear for 1..64 rows -- the weight stream of a decode step at half the bytes:
//   y[m, n] = act(scale[n] * (x[m, :] . q[n, :]) + bias[n]) (+ residual[m, n]),  1 <= M <= 64,
// x bf16, q raw e4m3 bytes [Nw][ldw] (k contiguous), scale f32 [Nw] (one per output row, the
// quantiser below).  Every e4m3 value is a bf16 value, so a weight byte is widened in registers
// (fp8.h: fp8_to_bf16x4, exact) and fed to the bf16 MFMA: the product is exact bf16 x bf16 into f32,
// the scale meets the summed accumulator once, ahead of the bias.  The only error beyond the bf16
// kernels' is the quantisation of the weights themselves.  Otherwise the contract of
// dpc_gemm_skinny (skinny_gemm.hip): f32 bias, activation codes, f32 residual, bf16 or f32 y,
// columns Nw <= n < N written as 0, no float atomics and no second launch (two calls, same bits).
//
// wq_kernel<RB, CB, NW>, grid ceil(N / (16 CB)), NW waves.
//   * A workgroup owns a strip of 16 CB output columns and all M rows (RB = ceil(M / 16) row
//     blocks, RB x CB floatx4 accumulators per lane): every weight byte is read once chip-wide.
//     The weights are the A operand of v_mfma_f32_16x16x32_bf16 and x the B operand, so a lane's
//     four results are four consecutive columns of one row: one 8-byte or 16-byte store.
//   * One step of a wave is 128 k: a whole 128-byte line of each of its weight rows.  Lane
//     (r, q) = (lane & 15, lane >> 4) loads the 32 contiguous bytes k0 + 32 q .. of its weight row
//     (two 16-byte loads), widens them into four bf16x8 operands and issues four MFMAs per
//     (column block, row block) against the four 16-byte x chunks at the same k (64 contiguous
//     bytes of an x row; a dot product does not care how k is dealt over lanes and MFMAs).
//   * The weight loads of the wave's next step issue before the converts and MFMAs of the current
//     one (2 CB 16-byte registers per step, two steps held); the x chunks of the current step are
//     requested first, so the wait ahead of the first MFMA leaves the next weights in flight.
//     A scheduling barrier keeps the compiler from pairing each load with its use.
//   * The NW waves split K step by step (wave v takes steps v, v + NW, ...); a wave with no step
//     adds zeros.  The one step that K cuts short runs with its 16-byte chunks at or past K read
//     from k = 0 and zeroed in both operands (K % 16 == 0: a chunk is wholly in or out).
//   * Partials are summed through LDS in wave order, accumulator a by wave a % NW, then the
//     epilogue runs once.  Rows past M and weight rows past Nw are clamped, not masked.
//
// Plans (columns, waves): (16, 8) and (32, 4), from ops/gemm.py:skinny_plan unless forced.
//
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950, no scratch in any instantiation),
// VGPRs of wq_kernel<RB, CB, NW>:
//   CB 1, NW 8:  RB 1: 66   RB 2: 90    RB 3: 108   RB 4: 134
//   CB 2, NW 4:  RB 1: 86   RB 2: 100   RB 3: 120   RB 4: 140
// wq_quant_kernel: 29.
//
// dpc_wq_quantize: q[n, k] = fp8_rne(clamp(float(w[n, k]) * inv[n], -448, 448)), 16 bytes per
// thread (fp8.h: fp8_quant16); ops/gemm.py:weight_quantize_ref is its torch twin, bit for bit.
#include "common.h"
#include "fp8.h"

namespace dpc {

struct WqArgs {
  const void* x;          // [M][ldx] bf16
  const void* q;          // [Nw][ldw] e4m3 bytes, k contiguous
  const float* scale;     // [Nw] f32
  const float* bias;      // [Nw] f32 or null
  const float* residual;  // [M][ldr] f32 or null
  void* y;                // [M][ldy] bf16 or f32
  long long ldx, ldw, ldr, ldy;
  int M, N, Nw, K;
  int act, y_f32;
  int nb, nw;             // the plan: (16, 8) or (32, 4)
};

struct WqQuantArgs {
  const void* w;     // [N][ldw] bf16
  const float* inv;  // [N] f32: 1 / scale
  void* q;           // [N][ldq] e4m3 bytes
  long long ldw, ldq;
  int N, K;
};

constexpr int WQ_STEP = 128;  // k per wave step: 4 lane groups x 32

// one step's weight bytes of a lane: per column block two 16-byte chunks (32 k)
template <int CB>
struct WqW {
  uint4 w[CB][2];
};

// TAIL: chunks at or past K are read from k = 0 instead and zeroed
template <int CB, bool TAIL>
__device__ __forceinline__ void wq_load_w(WqW<CB>& f, const fp8_t* const* wrow, int k, int K) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const bool ok = !TAIL || k + 16 * h < K;
    const int kk = ok ? k + 16 * h : 0;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      f.w[c][h] = *reinterpret_cast<const uint4*>(wrow[c] + kk);
      if (TAIL && !ok) f.w[c][h] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// the four 16-byte x chunks (8 k each) under a lane's 32 weight bytes
template <int RB, bool TAIL>
__device__ __forceinline__ void wq_load_x(uint4 (&x)[RB][4], const bf16_t* const* xrow, int k, int K) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
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
__device__ __forceinline__ bf16x8 wq_widen8(unsigned lo, unsigned hi) {
  const uint2 a = fp8_to_bf16x4(lo), b = fp8_to_bf16x4(hi);
  return __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, b.x, b.y));
}

template <int RB, int CB>
__device__ __forceinline__ void wq_mma(floatx4 (&acc)[CB][RB], const WqW<CB>& f, const uint4 (&x)[RB][4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const bf16x8 a0 = wq_widen8(f.w[c][h].x, f.w[c][h].y), a1 = wq_widen8(f.w[c][h].z, f.w[c][h].w);
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        acc[c][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, __builtin_bit_cast(bf16x8, x[r][2 * h]), acc[c][r], 0, 0, 0);
        acc[c][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, __builtin_bit_cast(bf16x8, x[r][2 * h + 1]), acc[c][r], 0, 0, 0);
      }
    }
}

template <int RB, int CB, int NW>
__global__ __launch_bounds__(64 * NW) void wq_kernel(WqArgs p) {
  constexpr int ACC = CB * RB;
  __shared__ floatx4 red[NW][ACC][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * (16 * CB);
  const bf16_t* X = static_cast<const bf16_t*>(p.x);
  const fp8_t* W = static_cast<const fp8_t*>(p.q);

  const fp8_t* wrow[CB];
  const bf16_t* xrow[RB];
#pragma unroll
  for (int c = 0; c < CB; ++c) wrow[c] = W + (long long)min(n0 + c * 16 + r16, p.Nw - 1) * p.ldw;
#pragma unroll
  for (int r = 0; r < RB; ++r) xrow[r] = X + (long long)min(r * 16 + r16, p.M - 1) * p.ldx;

  floatx4 acc[CB][RB];
#pragma unroll
  for (int c = 0; c < CB; ++c)
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[c][r] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int K = p.K, kl = q * 32;
  int k0 = wv * WQ_STEP;
  WqW<CB> wc;
  uint4 xs[RB][4];
  if (k0 + WQ_STEP <= K) wq_load_w<CB, false>(wc, wrow, k0 + kl, K);
  // whole steps with a whole one after them, two per trip: the weight registers alternate (a copy
  // at the end of every step would wait for the next weights before the next x loads issue)
  while (k0 + NW * WQ_STEP + WQ_STEP <= K) {
    WqW<CB> wn;
    wq_load_x<RB, false>(xs, xrow, k0 + kl, K);
    wq_load_w<CB, false>(wn, wrow, k0 + NW * WQ_STEP + kl, K);
    // x first, then the next step's weights: the MFMAs wait for x alone (left alone, the
    // scheduler sinks each load to its use)
    __builtin_amdgcn_sched_barrier(0);
    wq_mma<RB, CB>(acc, wc, xs);
    k0 += NW * WQ_STEP;
    if (k0 + NW * WQ_STEP + WQ_STEP > K) {
      wc = wn;
      break;
    }
    wq_load_x<RB, false>(xs, xrow, k0 + kl, K);
    wq_load_w<CB, false>(wc, wrow, k0 + NW * WQ_STEP + kl, K);
    __builtin_amdgcn_sched_barrier(0);
    wq_mma<RB, CB>(acc, wn, xs);
    k0 += NW * WQ_STEP;
  }
  if (k0 + WQ_STEP <= K) {  // the last whole step: its weights are here or on their way
    wq_load_x<RB, false>(xs, xrow, k0 + kl, K);
    __builtin_amdgcn_sched_barrier(0);
    wq_mma<RB, CB>(acc, wc, xs);
    k0 += NW * WQ_STEP;
  }
  if (k0 < K) {  // the step K cuts short (one wave of the workgroup at most)
    wq_load_x<RB, true>(xs, xrow, k0 + kl, K);
    wq_load_w<CB, true>(wc, wrow, k0 + kl, K);
    __builtin_amdgcn_sched_barrier(0);
    wq_mma<RB, CB>(acc, wc, xs);
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
    float sc[4], b[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sc[i] = p.scale[min(n + i, p.Nw - 1)];
    if (p.bias) {
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = p.bias[min(n + i, p.Nw - 1)];
    }
    if (p.residual) {
#pragma unroll
      for (int i = 0; i < 4; ++i) rs[i] = p.residual[(long long)m * p.ldr + min(n + i, p.Nw - 1)];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = n + i < p.Nw ? act_fwd(s[i] * sc[i] + b[i], p.act) + rs[i] : 0.f;
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

template <int CB, int NW>
static void wq_launch(const WqArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + 16 * CB - 1) / (16 * CB))), block(64 * NW);
  switch ((a.M + 15) / 16) {
    case 1: hipLaunchKernelGGL((wq_kernel<1, CB, NW>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((wq_kernel<2, CB, NW>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((wq_kernel<3, CB, NW>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((wq_kernel<4, CB, NW>), grid, block, 0, stream, a); break;
  }
}

// one thread per 16 k of one row: two 16-byte loads, one 16-byte store
__global__ __launch_bounds__(256) void wq_quant_kernel(WqQuantArgs p) {
  const long long chunks = p.K / 16;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= chunks * p.N) return;
  const long long n = t / chunks, k = (t % chunks) * 16;
  const bf16_t* src = static_cast<const bf16_t*>(p.w) + n * p.ldw + k;
  const uint4 lo = *reinterpret_cast<const uint4*>(src), hi = *reinterpret_cast<const uint4*>(src + 8);
  *reinterpret_cast<uint4*>(static_cast<fp8_t*>(p.q) + n * p.ldq + k) = fp8_quant16(lo, hi, p.inv[n]);
}

}  // namespace dpc

using namespace dpc;

// Requirements: 1 <= M <= 64, K % 16 == 0, weight rows 16-B aligned (ldw % 16 == 0), x rows 16-B
// aligned (ldx % 8 == 0), 1 <= Nw <= N <= ldy, Nw <= ldr with a residual, (nb, nw) one of
// (16, 8), (32, 4).
DPC_API int dpc_gemm_wq8(const WqArgs* a, hipStream_t stream) {
  if (a->M <= 0 || a->N <= 0) return 0;
  if (a->M > 64 || a->K <= 0 || a->K % 16 || a->ldx % 8 || a->ldw % 16 || a->ldx < a->K || a->ldw < a->K || a->Nw < 1 ||
      a->Nw > a->N || a->N > a->ldy || (a->residual && a->ldr < a->Nw) || !a->scale || ((uintptr_t)a->x % 16) ||
      ((uintptr_t)a->q % 16))
    return (int)hipErrorInvalidValue;
  if (a->nb == 16 && a->nw == 8) wq_launch<1, 8>(*a, stream);
  else if (a->nb == 32 && a->nw == 4) wq_launch<2, 4>(*a, stream);
  else return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

// Requirements: K % 16 == 0, w rows 16-B aligned (ldw % 8 == 0), q rows 16-B aligned (ldq % 16 == 0).
DPC_API int dpc_wq_quantize(const WqQuantArgs* a, hipStream_t stream) {
  if (a->N <= 0 || a->K <= 0) return 0;
  if (a->K % 16 || a->ldw % 8 || a->ldq % 16 || a->ldw < a->K || a->ldq < a->K || !a->inv || ((uintptr_t)a->w % 16) ||
      ((uintptr_t)a->q % 16))
    return (int)hipErrorInvalidValue;
  const long long threads = (long long)a->N * (a->K / 16);
  hipLaunchKernelGGL(wq_quant_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, *a);
  return (int)hipGetLastError();
}
