// Weight-only MXFP4 Linear for 1..64 rows -- the weight stream of a decode step at half a byte per
// element:
//   y[m, n] = act(x[m, :] . w4[n, :] + bias[n]) (+ residual[m, n]),  1 <= M <= 64,
// x bf16, w4 the MXFP4 weight (mxfp4.h): q [Nw][ldw] bytes of two e2m1 each, k contiguous, element
// 2j in the low nibble of byte j, and scale [Nw][K / 32] e8m0 bytes, one per block of 32 k.  One
// v_cvt_scalef32_pk_bf16_fp4 turns a byte and its block's scale into two bf16 with the scale
// applied, exactly (every e2m1 value times a power of two is a bf16 value), so the operand of the
// bf16 MFMA is the dequantised weight itself: no scale meets the accumulator, the epilogue is the
// skinny kernel's, and the only error beyond the bf16 kernels' is the rounding of the weights.
// Otherwise the contract of dpc_gemm_wq8 (wq_gemm.hip): f32 bias, activation codes, f32 residual,
// bf16 or f32 y, columns Nw <= n < N written as 0, no float atomics and no second launch (two
// calls, same bits).
//
// wq4_kernel<RB, CB, NW>, grid ceil(N / (16 CB)), NW waves.
//   * The work split of wq_kernel: a workgroup owns a strip of 16 CB output columns and all M rows
//     (RB = ceil(M / 16) row blocks, RB x CB floatx4 accumulators per lane); the weights are the A
//     operand of v_mfma_f32_16x16x32_bf16 and x the B operand, so a lane's four results are four
//     consecutive columns of one row.
//   * One step of a wave is 256 k: a whole 128-byte line of each of its weight rows, the same bytes
//     per step as wq_kernel in half the trips (the per-layer products are bound by latency more
//     than by bytes: a 128 k step would keep half the bytes in flight for the same number of
//     round trips).  Lane (r, q) = (lane & 15, lane >> 4) loads the 32 contiguous bytes of k0 +
//     64 q .. of its weight row as two 16-byte loads -- each exactly one MX block, hence one scale
//     for the whole load -- widens each dword (8 k) with four converts into one bf16x8 operand and
//     issues four MFMAs per load and (column block, row block) against the four 16-byte x chunks at
//     the same k (128 contiguous bytes of an x row per step; a dot product does not care how k is
//     dealt over lanes and MFMAs).
//   * The two scales of a lane's step are adjacent bytes of its scale row: one 2-byte load where
//     the scale rows keep that alignment (K / 32 even, all the model shapes), else two 1-byte
//     loads.  They are requested with the weights, a step ahead, and become floats by a shift
//     (byte << 23) at the converts.
//   * The weight and scale loads of the wave's next step issue before the converts and MFMAs of
//     the current one (two register sets alternate); the x chunks of the current step are requested
//     first, so the wait ahead of the first MFMA leaves the next weights in flight.  A scheduling
//     barrier keeps the compiler from pairing each load with its use.
//   * The NW waves split K step by step (wave v takes steps v, v + NW, ...); a wave with no step
//     adds zeros.  The one step that K cuts short runs with its blocks at or past K read from
//     k = 0 and zeroed in both operands (K % 32 == 0: a block is wholly in or out; a zero nibble
//     is 0 under any scale).
//   * Partials are summed through LDS in wave order, accumulator a by wave a % NW, then the
//     epilogue runs once.  Rows past M and weight rows past Nw are clamped, not masked.
//
// Plans (columns, waves): (16, 8) and (32, 4), from ops/gemm.py:skinny_plan unless forced.
//
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950, no scratch in any instantiation),
// VGPRs of wq4_kernel<RB, CB, NW>:
//   CB 1, NW 8:  RB 1: 84    RB 2: 122   RB 3: 160   RB 4: 198
//   CB 2, NW 4:  RB 1: 110   RB 2: 137   RB 3: 173   RB 4: 209
// wq4_quant_kernel: 52.
//
// dpc_wq4_quantize: one thread per block of 32 k -- amax over the bf16 payloads, the exponent from
// its bits, sixteen bytes of codes by compares, one scale byte (mxfp4.h);
// ops/gemm.py:mx_quantize_ref is its torch twin, bit for bit.
#include "common.h"
#include "mxfp4.h"

namespace dpc {

struct Wq4Args {
  const void* x;               // [M][ldx] bf16
  const unsigned char* q;      // [Nw][ldw] bytes of two e2m1, k contiguous
  const unsigned char* scale;  // [Nw][K / 32] e8m0, contiguous
  const float* bias;           // [Nw] f32 or null
  const float* residual;       // [M][ldr] f32 or null
  void* y;                     // [M][ldy] bf16 or f32
  long long ldx, ldw, ldr, ldy;  // ldw in bytes
  int M, N, Nw, K;
  int act, y_f32;
  int nb, nw;                  // the plan: (16, 8) or (32, 4)
};

struct Wq4QuantArgs {
  const void* w;         // [N][ldw] bf16
  unsigned char* q;      // [N][ldq] bytes
  unsigned char* scale;  // [N][K / 32]
  long long ldw, ldq;
  int N, K;
};

constexpr int WQ4_STEP = 256;  // k per wave step: 4 lane groups x 2 blocks of 32

// one step's weights of a lane: per column block two 16-byte loads (a block of 32 k each) and the
// two blocks' scale bytes (block h in byte h)
template <int CB>
struct Wq4W {
  uint4 w[CB][2];
  unsigned s[CB];
};

// k: the lane's first k of the step.  TAIL: blocks at or past K are read from k = 0 instead and
// zeroed.  PAIR: the scale rows are 2-byte aligned (uniform over the launch)
template <int CB, bool TAIL>
__device__ __forceinline__ void wq4_load_w(Wq4W<CB>& f, const unsigned char* const* wrow, const unsigned char* const* srow,
                                           int k, int K, bool pair) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const bool ok = !TAIL || k + MX_BLOCK * h < K;
    const int kk = ok ? k + MX_BLOCK * h : 0;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      f.w[c][h] = *reinterpret_cast<const uint4*>(wrow[c] + kk / 2);
      if (TAIL && !ok) f.w[c][h] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  if (!TAIL && pair) {
#pragma unroll
    for (int c = 0; c < CB; ++c) f.s[c] = *reinterpret_cast<const unsigned short*>(srow[c] + k / MX_BLOCK);
  } else {
    const int k1 = !TAIL || k + MX_BLOCK < K ? k + MX_BLOCK : 0;
    const int kz = !TAIL || k < K ? k : 0;
#pragma unroll
    for (int c = 0; c < CB; ++c)
      f.s[c] = (unsigned)srow[c][kz / MX_BLOCK] | ((unsigned)srow[c][k1 / MX_BLOCK] << 8);
  }
}

// the eight 16-byte x chunks (8 k each) under a lane's 64 weights
template <int RB, bool TAIL>
__device__ __forceinline__ void wq4_load_x(uint4 (&x)[RB][8], const bf16_t* const* xrow, int k, int K) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool ok = !TAIL || k + 8 * j < K;
    const int kk = ok ? k + 8 * j : 0;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      x[r][j] = *reinterpret_cast<const uint4*>(xrow[r] + kk);
      if (TAIL && !ok) x[r][j] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

template <int RB, int CB>
__device__ __forceinline__ void wq4_mma(floatx4 (&acc)[CB][RB], const Wq4W<CB>& f, const uint4 (&x)[RB][8]) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const float s = mx_scale((f.s[c] >> (8 * h)) & 0xffu);
      const bf16x8 a[4] = {mx_widen8(f.w[c][h].x, s), mx_widen8(f.w[c][h].y, s), mx_widen8(f.w[c][h].z, s),
                           mx_widen8(f.w[c][h].w, s)};
#pragma unroll
      for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[c][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], __builtin_bit_cast(bf16x8, x[r][4 * h + j]), acc[c][r], 0, 0, 0);
    }
}

template <int RB, int CB, int NW>
__global__ __launch_bounds__(64 * NW) void wq4_kernel(Wq4Args p) {
  constexpr int ACC = CB * RB;
  __shared__ floatx4 red[NW][ACC][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * (16 * CB);
  const bf16_t* X = static_cast<const bf16_t*>(p.x);
  const int K = p.K, kl = q * 64;
  const bool pair = ((K / MX_BLOCK) % 2 == 0) && ((uintptr_t)p.scale % 2 == 0);

  const unsigned char* wrow[CB];
  const unsigned char* srow[CB];
  const bf16_t* xrow[RB];
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    const long long n = min(n0 + c * 16 + r16, p.Nw - 1);
    wrow[c] = p.q + n * p.ldw;
    srow[c] = p.scale + n * (K / MX_BLOCK);
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) xrow[r] = X + (long long)min(r * 16 + r16, p.M - 1) * p.ldx;

  floatx4 acc[CB][RB];
#pragma unroll
  for (int c = 0; c < CB; ++c)
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[c][r] = floatx4{0.f, 0.f, 0.f, 0.f};

  int k0 = wv * WQ4_STEP;
  Wq4W<CB> wc;
  uint4 xs[RB][8];
  if (k0 + WQ4_STEP <= K) wq4_load_w<CB, false>(wc, wrow, srow, k0 + kl, K, pair);
  // whole steps with a whole one after them, two per trip: the weight registers alternate (a copy
  // at the end of every step would wait for the next weights before the next x loads issue)
  while (k0 + NW * WQ4_STEP + WQ4_STEP <= K) {
    Wq4W<CB> wn;
    wq4_load_x<RB, false>(xs, xrow, k0 + kl, K);
    wq4_load_w<CB, false>(wn, wrow, srow, k0 + NW * WQ4_STEP + kl, K, pair);
    // x first, then the next step's weights and scales: the MFMAs wait for x alone (left alone,
    // the scheduler sinks each load to its use)
    __builtin_amdgcn_sched_barrier(0);
    wq4_mma<RB, CB>(acc, wc, xs);
    k0 += NW * WQ4_STEP;
    if (k0 + NW * WQ4_STEP + WQ4_STEP > K) {
      wc = wn;
      break;
    }
    wq4_load_x<RB, false>(xs, xrow, k0 + kl, K);
    wq4_load_w<CB, false>(wc, wrow, srow, k0 + NW * WQ4_STEP + kl, K, pair);
    __builtin_amdgcn_sched_barrier(0);
    wq4_mma<RB, CB>(acc, wn, xs);
    k0 += NW * WQ4_STEP;
  }
  if (k0 + WQ4_STEP <= K) {  // the last whole step: its weights are here or on their way
    wq4_load_x<RB, false>(xs, xrow, k0 + kl, K);
    __builtin_amdgcn_sched_barrier(0);
    wq4_mma<RB, CB>(acc, wc, xs);
    k0 += NW * WQ4_STEP;
  }
  if (k0 < K) {  // the step K cuts short (one wave of the workgroup at most)
    wq4_load_x<RB, true>(xs, xrow, k0 + kl, K);
    wq4_load_w<CB, true>(wc, wrow, srow, k0 + kl, K, pair);
    __builtin_amdgcn_sched_barrier(0);
    wq4_mma<RB, CB>(acc, wc, xs);
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
    // (the bias and residual loads issue together: columns past Nw read column Nw - 1)
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
static void wq4_launch(const Wq4Args& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + 16 * CB - 1) / (16 * CB))), block(64 * NW);
  switch ((a.M + 15) / 16) {
    case 1: hipLaunchKernelGGL((wq4_kernel<1, CB, NW>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((wq4_kernel<2, CB, NW>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((wq4_kernel<3, CB, NW>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((wq4_kernel<4, CB, NW>), grid, block, 0, stream, a); break;
  }
}

// e2m1 code (sign in bit 3) of the f32 with these bits, times inv = 2^-e
__device__ __forceinline__ unsigned wq4_code(unsigned bits, float inv) {
  return mx_code(__uint_as_float(bits & 0x7fffffffu) * inv) | ((bits >> 31) << 3);
}

// one thread per block of 32 k of one row: four 16-byte loads, one 16-byte store, one scale byte
__global__ __launch_bounds__(256) void wq4_quant_kernel(Wq4QuantArgs p) {
  const long long blocks = p.K / MX_BLOCK;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= blocks * p.N) return;
  const long long n = t / blocks, b = t % blocks;
  const uint4* src = reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(p.w) + n * p.ldw + b * MX_BLOCK);
  unsigned d[16];  // two bf16 each
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint4 v = src[i];
    d[4 * i] = v.x, d[4 * i + 1] = v.y, d[4 * i + 2] = v.z, d[4 * i + 3] = v.w;
  }
  unsigned amax = 0u;  // |bf16| payloads order as integers
#pragma unroll
  for (int i = 0; i < 16; ++i) amax = max(amax, max(d[i] & 0x7fffu, (d[i] >> 16) & 0x7fffu));
  const int e = mx_exponent(amax << 16);
  const float inv = __uint_as_float((unsigned)(127 - e) << 23);
  unsigned o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[i] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned w = d[4 * i + j];
      o[i] |= (wq4_code(w << 16, inv) | (wq4_code(w & 0xffff0000u, inv) << 4)) << (8 * j);
    }
  }
  *reinterpret_cast<uint4*>(p.q + n * p.ldq + b * (MX_BLOCK / 2)) = make_uint4(o[0], o[1], o[2], o[3]);
  p.scale[n * blocks + b] = (unsigned char)(e + 127);
}

}  // namespace dpc

using namespace dpc;

// Requirements: 1 <= M <= 64, K % 32 == 0, weight rows 16-B aligned (ldw % 16 == 0, ldw >= K / 2
// bytes), x rows 16-B aligned (ldx % 8 == 0), scale [Nw][K / 32] contiguous, 1 <= Nw <= N <= ldy,
// Nw <= ldr with a residual, (nb, nw) one of (16, 8), (32, 4).
DPC_API int dpc_gemm_wq4(const Wq4Args* a, hipStream_t stream) {
  if (a->M <= 0 || a->N <= 0) return 0;
  if (a->M > 64 || a->K <= 0 || a->K % MX_BLOCK || a->ldx % 8 || a->ldw % 16 || a->ldx < a->K || a->ldw < a->K / 2 ||
      a->Nw < 1 || a->Nw > a->N || a->N > a->ldy || (a->residual && a->ldr < a->Nw) || !a->scale || !a->q || !a->x ||
      !a->y || ((uintptr_t)a->x % 16) || ((uintptr_t)a->q % 16))
    return (int)hipErrorInvalidValue;
  if (a->nb == 16 && a->nw == 8) wq4_launch<1, 8>(*a, stream);
  else if (a->nb == 32 && a->nw == 4) wq4_launch<2, 4>(*a, stream);
  else return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

// Requirements: K % 32 == 0, w rows 16-B aligned (ldw % 8 == 0), q rows 16-B aligned (ldq % 16 == 0,
// ldq >= K / 2 bytes), scale [N][K / 32] contiguous.
DPC_API int dpc_wq4_quantize(const Wq4QuantArgs* a, hipStream_t stream) {
  if (a->N <= 0 || a->K <= 0) return 0;
  if (a->K % MX_BLOCK || a->ldw % 8 || a->ldq % 16 || a->ldw < a->K || a->ldq < a->K / 2 || !a->w || !a->q || !a->scale ||
      ((uintptr_t)a->w % 16) || ((uintptr_t)a->q % 16))
    return (int)hipErrorInvalidValue;
  const long long threads = (long long)a->N * (a->K / MX_BLOCK);
  hipLaunchKernelGGL(wq4_quant_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, *a);
  return (int)hipGetLastError();
}
