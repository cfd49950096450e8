// Few-row Linear for 17..64 rows (batched decode, blocks of draft tokens, chunked-prefill tails):
//   y[m, n] = act(x[m, :] . w[n, :] + bias[n]) (+ residual[m, n]),  1 <= M <= 64,
// the contract of dpc_gemv (decode.hip) with more rows.  The product is still a stream of the
// weight matrix, but between 17 and 64 rows every weight byte meets enough x rows for the matrix
// cores: the vector ALUs would be instruction-bound, and the 256 x 256 tile kernels give it
// N / 256 workgroups.
//
// skinny_kernel<RB, CB, NW>, grid ceil(N / (16 CB)), NW waves.
//   * A workgroup owns a strip of NB = 16 CB output columns and all M rows, so every weight byte
//     is read once chip-wide.  The rows run as RB = ceil(M / 16) row blocks: RB x CB accumulators
//     (floatx4) per lane.
//   * Operands go from global memory straight into MFMA registers (v_mfma_f32_16x16x32_bf16): both
//     are k-contiguous, and a lane's operand is 8 consecutive k of one row -- one 16-byte load, no
//     LDS staging.  The weights are the A operand and x the B operand, so a lane's four results are
//     four CONSECUTIVE columns n of one row m: one 8-byte (bf16) or 16-byte (f32) store.
//   * Whole-line reads: lane (r, q) = (lane & 15, lane >> 4) takes the 32 contiguous bytes
//     k0 + 16 q .. k0 + 16 q + 15 of its row per step and feeds two MFMAs with them (x is read with
//     the same k permutation; a dot product does not care about the order of k).  One step of a
//     wave is 64 k: a whole 128-byte line of each weight row.
//   * The NW waves split K, step by step (wave v takes steps v, v + NW, ...), two steps in flight.
//     A wave that gets no step contributes zeros.  The one step that K cuts short runs with its
//     16-byte chunks past K zeroed in both operands.
//   * After the loop every wave stores its accumulators to LDS; accumulator a is summed by wave
//     a % NW over the waves in index order and goes through the epilogue (bias, activation, f32
//     residual, zero padding for Nw <= n < N, bf16 or f32 store) once.  No float atomics, no
//     second launch: two calls give the same bits.
//   * Rows past M and weight rows past Nw are clamped to the last valid row, not masked: a surplus
//     x row only feeds output rows that are never stored, a surplus weight row only columns that
//     are written as 0.
//
// NB and NW come from the host planner (ops/gemm.py:skinny_plan): NB trades the x re-reads (every
// workgroup reads all of x from L2) against the workgroup count.  Two plans are built: 16 columns
// with 8 waves and 32 columns with 4 (a 64-column strip was slower than both on every measured
// shape, docs/GENERATION.md).
#include "common.h"

namespace dpc {

struct SkinnyArgs {
  const void* x;          // [M][ldx] bf16
  const void* w;          // [Nw][ldw] bf16, k contiguous (nn.Linear layout)
  const float* bias;      // [Nw] f32 or null
  const float* residual;  // [M][ldr] f32 or null
  void* y;                // [M][ldy] bf16 or f32
  long long ldx, ldw, ldr, ldy;
  int M, N, Nw, K;
  int act, y_f32;
  int nb, nw;             // the plan: columns per workgroup, waves per workgroup: (16, 8) or (32, 4)
};

constexpr int SK_STEP = 64;  // k per wave step: 4 lane groups x 16

// one step's operands of a lane: [block][half] 16-byte chunks
template <int RB, int CB>
struct SkFrag {
  uint4 w[CB][2], x[RB][2];
};

// TAIL: chunks at or past K are read from k = 0 instead and zeroed (in both operands: the other
// one may hold an inf)
template <int RB, int CB, bool TAIL>
__device__ __forceinline__ void sk_load(SkFrag<RB, CB>& f, const bf16_t* const* wrow, const bf16_t* const* xrow,
                                        int k, int K) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const bool ok = !TAIL || k + 8 * h < K;
    const int kk = ok ? k + 8 * h : 0;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      f.w[c][h] = *reinterpret_cast<const uint4*>(wrow[c] + kk);
      if (TAIL && !ok) f.w[c][h] = make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      f.x[r][h] = *reinterpret_cast<const uint4*>(xrow[r] + kk);
      if (TAIL && !ok) f.x[r][h] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

template <int RB, int CB>
__device__ __forceinline__ void sk_mma(floatx4 (&acc)[CB][RB], const SkFrag<RB, CB>& f) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
      for (int r = 0; r < RB; ++r)
        acc[c][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, f.w[c][h]),
                                                            __builtin_bit_cast(bf16x8, f.x[r][h]), acc[c][r], 0, 0, 0);
}

template <int RB, int CB, int NW>
__global__ __launch_bounds__(64 * NW) void skinny_kernel(SkinnyArgs p) {
  constexpr int ACC = CB * RB;
  __shared__ floatx4 red[NW][ACC][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * (16 * CB);
  const bf16_t* X = static_cast<const bf16_t*>(p.x);
  const bf16_t* W = static_cast<const bf16_t*>(p.w);

  const bf16_t* wrow[CB];
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

  const int K = p.K, kl = q * 16;
  int k0 = wv * SK_STEP;
  for (; k0 + NW * SK_STEP + SK_STEP <= K; k0 += 2 * NW * SK_STEP) {  // two whole steps in flight
    SkFrag<RB, CB> f0, f1;
    sk_load<RB, CB, false>(f0, wrow, xrow, k0 + kl, K);
    sk_load<RB, CB, false>(f1, wrow, xrow, k0 + NW * SK_STEP + kl, K);
    // every load of both steps issues before the first MFMA waits (left alone, the scheduler
    // keeps the register count down by pairing each load with its MFMA and a full wait)
    __builtin_amdgcn_sched_barrier(0);
    sk_mma<RB, CB>(acc, f0);
    sk_mma<RB, CB>(acc, f1);
  }
  if (k0 + SK_STEP <= K) {  // a last whole step
    SkFrag<RB, CB> f;
    sk_load<RB, CB, false>(f, wrow, xrow, k0 + kl, K);
    __builtin_amdgcn_sched_barrier(0);
    sk_mma<RB, CB>(acc, f);
    k0 += NW * SK_STEP;
  }
  if (k0 < K) {  // the step K cuts short (one wave of the workgroup at most)
    SkFrag<RB, CB> f;
    sk_load<RB, CB, true>(f, wrow, xrow, k0 + kl, K);
    __builtin_amdgcn_sched_barrier(0);
    sk_mma<RB, CB>(acc, f);
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
    // (the four bias and residual loads issue together: columns past Nw read column Nw - 1)
    float b[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
    if (p.bias) {
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = p.bias[min(n + i, p.Nw - 1)];
    }
    if (p.residual) {
#pragma unroll
      for (int i = 0; i < 4; ++i) rs[i] = p.residual[(long long)m * p.ldr + min(n + i, p.Nw - 1)];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = n + i < p.Nw ? act_fwd(s[i] + b[i], p.act) + rs[i] : 0.f;
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
static void sk_launch(const SkinnyArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + 16 * CB - 1) / (16 * CB))), block(64 * NW);
  switch ((a.M + 15) / 16) {
    case 1: hipLaunchKernelGGL((skinny_kernel<1, CB, NW>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((skinny_kernel<2, CB, NW>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((skinny_kernel<3, CB, NW>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((skinny_kernel<4, CB, NW>), grid, block, 0, stream, a); break;
  }
}

}  // namespace dpc

using namespace dpc;

// Requirements: 1 <= M <= 64, K % 8 == 0, x / w rows 16-B aligned (ld % 8 == 0), 1 <= Nw <= N <= ldy,
// Nw <= ldr with a residual, (nb, nw) one of (16, 8), (32, 4).
DPC_API int dpc_gemm_skinny(const SkinnyArgs* a, hipStream_t stream) {
  if (a->M <= 0 || a->N <= 0) return 0;
  if (a->M > 64 || a->K <= 0 || a->K % 8 || a->ldx % 8 || a->ldw % 8 || a->Nw < 1 || a->Nw > a->N || a->N > a->ldy ||
      (a->residual && a->ldr < a->Nw) || ((uintptr_t)a->x % 16) || ((uintptr_t)a->w % 16))
    return (int)hipErrorInvalidValue;
  if (a->nb == 16 && a->nw == 8) sk_launch<1, 8>(*a, stream);
  else if (a->nb == 32 && a->nw == 4) sk_launch<2, 4>(*a, stream);
  else return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}
