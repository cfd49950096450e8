// Append attention: a block of n new tokens per sequence against a KV cache that already holds
// tokens -- Sq != Sk, the causal diagonal offset by a length that lives on the device.  Chunked
// prefill, continuing a cache with a block, scoring a handful of draft tokens.
//
// New token i of sequence s sits at position p = start + i, start = len[s] (len[0] without
// per_seq), read on the device: no launch shape depends on it, so the call can be captured in a
// HIP graph.  p < Smax: its key / value go to cache row p and its output is
// softmax(scale q_i . K[0..p]) V[0..p] (bottom-right aligned causal mask).  p >= Smax (or a
// negative start): nothing is written and the output row is zero, the decode kernels' rule for a
// full sequence.  len is not advanced.
//
// Three launches on one stream:
//   append_kv_kernel      the block's K / V rows out of qkv into the cache, one 16-B chunk per
//                         thread, guarded by p < Smax.  The attention launch then reads every key
//                         from the cache alone.
//   append_attn_kernel    grid (query tiles, nsplit, N*H), 4 waves.  A workgroup owns AQB = 128
//                         query rows of one (sequence, head), a wave a slab of 32 whose Q fragments
//                         stay in registers for the whole sweep.  K and V arrive in AKT = 64-key
//                         tiles through LDS: plain 16-B global loads of tile t+1 are issued into
//                         registers before the work on tile t and stored to the other of two LDS
//                         buffers after it (synchronous staging, one barrier per tile; no LDS-DMA
//                         ring).  The LDS image is attention.hip's (128-B physical rows, 16-B chunk
//                         swizzle), so the row reads and the transposing V reads are conflict free.
//                         S^T = K Q^T with v_mfma_f32_32x32x16_bf16: the query sits on the lane, the
//                         row max and row sum are lane-local (+ one xor-32 shuffle), and the score
//                         accumulators, packed to bf16, are the B operand of O^T += V^T P^T.  Online
//                         softmax in f32, log2 units, the running max moved only when a tile max
//                         exceeds it by 2^8 (attention.hip's lazy rescale).  Key tiles wholly under
//                         the wave's diagonal run unmasked, tiles that cross it compare the key
//                         offset with the lane's limit, tiles wholly above it are skipped.
//                         Split sp of nsplit takes a contiguous run of the workgroup's live key
//                         tiles (ceil(live / nsplit) each; live follows the device length, the grid
//                         does not).  nsplit == 1 normalises and stores bf16 o; otherwise the lane
//                         writes f32 (o[hd], m, l) of its query row to the workspace
//                         [N*n*H][nsplit][hd + 4].
//   append_attn_combine_kernel   (nsplit > 1) one thread per (row, head dim): the partials in index
//                         order, an empty split has l = 0.  No float atomics anywhere: the same
//                         inputs give the same bits on every run.
//
// The 1-byte e4m3 cache (fp8.h; dpc_append_attn_fp8) differs in the first launch and in the
// staging alone:
//   kv_store_fp8_kernel   in place of append_kv_kernel: a thread takes 16 output bytes -- two 16-B
//                         bf16 loads, x inv_scale, clamp, eight converts, one 16-B store.
//   append_attn_kernel<HD, fp8_t>   fetch loads 8 bytes (8 elements) where the bf16 path loads 16,
//                         with the same thread-to-chunk assignment, and stage widens them to 8
//                         bf16 (exact: the upper halves of the converted f32) into the same 16-B
//                         LDS chunk.  The LDS image, the MFMA loop, masking, splits and combine
//                         are shared; k_scale multiplies c, v_scale multiplies o once on its way
//                         out (normalised output or partial).  The block's own keys are read back
//                         from the cache like every other key: quantised first, then attended to.
//                         (16-B loads with another assignment were not tried: unmeasured.)
#include "fp8.h"

#include <type_traits>

namespace dpc {

struct AppendAttnArgs {
  const void* qkv;       // [N*n][ldqkv] bf16: q | k | v blocks of H*hd each, token-major
  void* kc;              // [N][Smax][E] bf16 key cache
  void* vc;              // [N][Smax][E] bf16 value cache
  void* o;               // [N*n][ldo] bf16
  const long long* len;  // device: cached tokens before the block ([1], or [N] with per_seq)
  long long ldqkv, ldo;
  int N, n, H, hd, Smax;
  float scale;
  int per_seq;
  float* ws;             // [N*n*H][nsplit][hd + 4] f32: o[hd], m, l, -, -  (nsplit > 1)
  int nsplit;
};

constexpr int AKT = 64;    // keys per staged tile
constexpr int AQB = 128;   // query rows per workgroup (4 waves x 32)
constexpr int ANT = 256;
constexpr int APPEND_MAX_SPLITS = 64;
constexpr float ALOG2E = 1.4426950408889634f;

typedef short4_t __attribute__((address_space(3))) * ap_lds4_t;

// ---- the LDS image and operand fragments of attention.hip (see its header for the layout)
__device__ __forceinline__ int ap_swz(int prow) {
  const int a = (prow >> 1) & 7;
  return a ^ ((a & 1) << 2);
}
// element offset of (row, 16-B chunk) in the LDS image of a [64][HD] tile
template <int HD>
__device__ __forceinline__ int ap_toff(int row, int chunk) {
  const int e = row * HD + chunk * 8;
  const int prow = e >> 6, pch = (e >> 3) & 7;
  return (prow << 6) + ((pch ^ ap_swz(prow)) << 3);
}
// row fragment (A or B operand of 32x32x16): lane holds X[row0 + (lane & 31)][16 st + 8 h .. +7]
template <int HD>
__device__ __forceinline__ bf16x8 ap_row_frag(const bf16_t* lds, int row0, int st, int lane) {
  return *reinterpret_cast<const bf16x8*>(lds + ap_toff<HD>(row0 + (lane & 31), 2 * st + (lane >> 5)));
}
// transposed fragment: lane gets X[rows r0 + 16 s + 8 (j >> 2) + 4 h + (j & 3)][col c0 + (lane & 31)],
// the permuted k order of an accumulator-as-operand k-step s
template <int HD>
__device__ __forceinline__ bf16x8 ap_tr_frag(const bf16_t* lds, int r0, int s, int c0, int lane) {
  const int h = lane >> 5, g2 = (lane >> 4) & 1, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
  const int row = r0 + 16 * s + 4 * h + q;
  const int col = c0 + 16 * g2 + 4 * p;
  const bf16_t* a0 = lds + ap_toff<HD>(row, col >> 3) + (col & 7);
  const bf16_t* a1 = lds + ap_toff<HD>(row + 8, col >> 3) + (col & 7);
  short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ap_lds4_t)a0);
  short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ap_lds4_t)a1);
  typedef short short8_t __attribute__((ext_vector_type(8)));
  short8_t s8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, s8);
}
// accumulator registers 8s..8s+7 -> bf16 operand fragment of k-step s
__device__ __forceinline__ bf16x8 ap_acc_frag(const floatx16& x, int s) {
  uint4 u;
  u.x = pack2bf(x[8 * s + 0], x[8 * s + 1]);
  u.y = pack2bf(x[8 * s + 2], x[8 * s + 3]);
  u.z = pack2bf(x[8 * s + 4], x[8 * s + 5]);
  u.w = pack2bf(x[8 * s + 6], x[8 * s + 7]);
  return __builtin_bit_cast(bf16x8, u);
}
// accumulator register r of a lane holds row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int ap_acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ float ap_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

#define AP_MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// start of sequence s, or -1 for a sequence that takes nothing (negative or past the capacity)
__device__ __forceinline__ int ap_start(const AppendAttnArgs& p, int s) {
  const long long v = p.per_seq ? p.len[s] : *p.len;
  return v >= 0 && v < p.Smax ? (int)v : -1;
}

// ------------------------------------------------------------------ append
// thread g: 16-B chunk g % (2 E / 8) of token g / (2 E / 8)'s k | v columns
__global__ __launch_bounds__(ANT) void append_kv_kernel(AppendAttnArgs p) {
  const int E = p.H * p.hd, cpt = E >> 2;  // chunks per token: k and v
  const long long g = (long long)blockIdx.x * ANT + threadIdx.x;
  const long long tok = g / cpt;
  if (tok >= (long long)p.N * p.n) return;
  const int c = (int)(g - tok * cpt);
  const int s = (int)(tok / p.n), i = (int)(tok - (long long)s * p.n);
  const int start = ap_start(p, s);
  if (start < 0 || i >= p.Smax - start) return;  // position start + i past the capacity: not written
  const bool isk = c < (E >> 3);
  const int cc = isk ? c : c - (E >> 3);
  const bf16_t* src = static_cast<const bf16_t*>(p.qkv) + tok * p.ldqkv + (isk ? E : 2 * E);
  bf16_t* dst = static_cast<bf16_t*>(isk ? p.kc : p.vc) + ((long long)s * p.Smax + start + i) * E;
  reinterpret_cast<uint4*>(dst)[cc] = reinterpret_cast<const uint4*>(src)[cc];
}

struct AppendAttnFp8Args {  // AppendAttnArgs (kc / vc e4m3) + the cache's scales
  const void* qkv;
  void* kc;
  void* vc;
  void* o;
  const long long* len;
  long long ldqkv, ldo;
  int N, n, H, hd, Smax;
  float scale;
  int per_seq;
  float* ws;
  int nsplit;
  float k_scale, k_inv, v_scale, v_inv;
};

static AppendAttnArgs ap_plain(const AppendAttnFp8Args& f) {
  AppendAttnArgs a;
  a.qkv = f.qkv, a.kc = f.kc, a.vc = f.vc, a.o = f.o, a.len = f.len;
  a.ldqkv = f.ldqkv, a.ldo = f.ldo;
  a.N = f.N, a.n = f.n, a.H = f.H, a.hd = f.hd, a.Smax = f.Smax;
  a.scale = f.scale, a.per_seq = f.per_seq, a.ws = f.ws, a.nsplit = f.nsplit;
  return a;
}

// thread g: 16-element chunk g % (2 E / 16) of token g / (2 E / 16)'s k | v columns, quantised
__global__ __launch_bounds__(ANT) void kv_store_fp8_kernel(AppendAttnArgs p, float k_inv, float v_inv) {
  const int E = p.H * p.hd, cpt = E >> 3;  // chunks per token: k and v
  const long long g = (long long)blockIdx.x * ANT + threadIdx.x;
  const long long tok = g / cpt;
  if (tok >= (long long)p.N * p.n) return;
  const int c = (int)(g - tok * cpt);
  const int s = (int)(tok / p.n), i = (int)(tok - (long long)s * p.n);
  const int start = ap_start(p, s);
  if (start < 0 || i >= p.Smax - start) return;  // position start + i past the capacity: not written
  const bool isk = c < (E >> 4);
  const int cc = isk ? c : c - (E >> 4);
  const uint4* src = reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(p.qkv) + tok * p.ldqkv + (isk ? E : 2 * E)) + 2 * cc;
  fp8_t* dst = static_cast<fp8_t*>(isk ? p.kc : p.vc) + ((long long)s * p.Smax + start + i) * E;
  reinterpret_cast<uint4*>(dst)[cc] = fp8_quant16(src[0], src[1], isk ? k_inv : v_inv);
}

// ------------------------------------------------------------------ attention
// CT: the cache element, bf16_t or fp8_t; ks / vs: the e4m3 cache's scales (unused for bf16)
template <int HD, typename CT = bf16_t>
__global__ __launch_bounds__(ANT) void append_attn_kernel(AppendAttnArgs p, float ks, float vs) {
  constexpr bool FP8 = std::is_same<CT, fp8_t>::value;
  typedef typename std::conditional<FP8, uint2, uint4>::type ld_t;  // a chunk of 8 cache elements
  constexpr int TILE = AKT * HD;    // elements of one tile
  constexpr int NST = HD / 16;      // k-steps of a product over the head
  constexpr int NDT = HD / 32;      // 32-column blocks of the O accumulator
  constexpr int CPR = HD / 8;       // 16-B chunks per key row
  constexpr int NLD = HD / 32;      // chunks of K (and of V) per thread per tile
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * 2 * TILE];  // [buffer][K|V]

  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qb = blockIdx.x, sp = blockIdx.y;
  const int s = blockIdx.z / p.H, h = blockIdx.z % p.H;
  const int n = p.n, Smax = p.Smax, E = p.H * HD;
  const int start = ap_start(p, s);

  // the workgroup's queries qb AQB .. qe - 1 see keys 0 .. kend - 1
  const int qe = min(n, qb * AQB + AQB);
  const int kend = start < 0 ? 0 : min(Smax, start + qe);
  const int live = (kend + AKT - 1) / AKT;
  const int per = (live + p.nsplit - 1) / p.nsplit;
  const int t0 = sp * per, t1 = min(live, t0 + per);  // this split's tiles (workgroup-uniform)

  // the wave's 32 queries; lane's query qi at position pos (pos = -1: takes nothing)
  const int q0 = qb * AQB + wid * 32;
  const int qi = q0 + (lane & 31);
  const bool qvalid = start >= 0 && qi < n && qi < Smax - start;
  const int pos = qvalid ? start + qi : -1;
  const bool wave_on = start >= 0 && q0 < n && q0 < Smax - start;                   // some lane is valid
  const bool wave_full = start >= 0 && q0 + 31 < n && q0 + 31 < Smax - start;       // every lane is
  const int last_w = wave_on ? (start + min(min(q0 + 31, n - 1), Smax - 1 - start)) / AKT : -1;

  const long long tok = (long long)s * n + qi;
  bf16x8 qf[NST];
  {
    const bf16_t* Q = static_cast<const bf16_t*>(p.qkv) + tok * p.ldqkv + h * HD;
#pragma unroll
    for (int st = 0; st < NST; ++st)
      qf[st] = qvalid ? *reinterpret_cast<const bf16x8*>(Q + 16 * st + 8 * hh) : bf16x8{};
  }
  const float c = FP8 ? p.scale * ALOG2E * ks : p.scale * ALOG2E;  // (e4m3: K dequantised here)

  const CT* K = static_cast<const CT*>(p.kc) + (long long)s * Smax * E + h * HD;
  const CT* V = static_cast<const CT*>(p.vc) + (long long)s * Smax * E + h * HD;
  // thread's chunk i of a tile: key row (tid + ANT i) / CPR, chunk (tid + ANT i) % CPR
  ld_t kr[NLD], vr[NLD];
  auto fetch = [&](int t) {  // rows at or past kend land as zeros (never read past the live keys)
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int g = tid + ANT * i, row = g / CPR, ch = g % CPR;
      const int j = t * AKT + row;
      kr[i] = ld_t{};
      vr[i] = ld_t{};
      if (j < kend) {
        kr[i] = reinterpret_cast<const ld_t*>(K + (long long)j * E)[ch];
        vr[i] = reinterpret_cast<const ld_t*>(V + (long long)j * E)[ch];
      }
    }
  };
  auto stage = [&](int t) {
    bf16_t* buf = smem + ((t - t0) & 1) * 2 * TILE;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int g = tid + ANT * i, off = ap_toff<HD>(g / CPR, g % CPR);
      if constexpr (FP8) {  // 8 e4m3 -> 8 bf16, exact
        const uint2 k0 = fp8_to_bf16x4(kr[i].x), k1 = fp8_to_bf16x4(kr[i].y);
        const uint2 v0 = fp8_to_bf16x4(vr[i].x), v1 = fp8_to_bf16x4(vr[i].y);
        *reinterpret_cast<uint4*>(buf + off) = make_uint4(k0.x, k0.y, k1.x, k1.y);
        *reinterpret_cast<uint4*>(buf + TILE + off) = make_uint4(v0.x, v0.y, v1.x, v1.y);
      } else {
        *reinterpret_cast<uint4*>(buf + off) = kr[i];
        *reinterpret_cast<uint4*>(buf + TILE + off) = vr[i];
      }
    }
  };

  float m = -INFINITY, l = 0.f;
  floatx16 o[NDT];
#pragma unroll
  for (int d = 0; d < NDT; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;

  if (t0 < t1) {
    fetch(t0);
    stage(t0);
  }
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    if (t + 1 < t1) fetch(t + 1);  // in flight under this tile's work
    if (t <= last_w) {             // wave-uniform: tiles wholly above the wave's diagonal are skipped
      const bf16_t* lk = smem + ((t - t0) & 1) * 2 * TILE;
      const bf16_t* lv = lk + TILE;
      const int kt0 = t * AKT;
      // S^T = K Q^T: keys on the accumulator rows, the query on the lane; raw (unscaled) scores
      floatx16 sc[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[kb][r] = 0.f;
#pragma unroll
        for (int st = 0; st < NST; ++st)
          sc[kb] = AP_MFMA32(ap_row_frag<HD>(lk, kb * 32, st, lane), qf[st], sc[kb]);
      }
      // the tile crosses the diagonal of the wave's first query, or some lane takes nothing
      if (kt0 + AKT - 1 > start + q0 || !wave_full) {
        const int lim = pos - kt0;  // key offsets above it are masked; pos = -1 masks every key
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (kb * 32 + ap_acc_row(r, lane) > lim) sc[kb][r] = -INFINITY;
      }
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[kb][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * c;  // scaled log2 units (c > 0)
      // lazy rescale: the running max moves only when the tile max exceeds it by > 2^8, so
      // p <= 256 (exact enough in f32 / bf16) and most tiles skip the O rescale
      if (__ballot(mx > m + 8.f)) {
        const float mn = fmaxf(m, mx);
        const float alpha = (mn == -INFINITY) ? 1.f : ap_exp2(m - mn);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int d = 0; d < NDT; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
      }
      const float nmu = (m == -INFINITY) ? 0.f : -m;
      float ls = 0.f;
      bf16x8 pb[2][2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = ap_exp2(fmaf(sc[kb][r], c, nmu));
          sc[kb][r] = e;
          ls += e;
        }
        pb[kb][0] = ap_acc_frag(sc[kb], 0);
        pb[kb][1] = ap_acc_frag(sc[kb], 1);
      }
      l += ls;
      // O^T += V^T P^T: V^T through transposing LDS reads, P^T straight from the score registers
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss)
#pragma unroll
          for (int d = 0; d < NDT; ++d)
            o[d] = AP_MFMA32(ap_tr_frag<HD>(lv, kb * 32, ss, d * 32, lane), pb[kb][ss], o[d]);
    }
    if (t + 1 < t1) stage(t + 1);  // the other buffer: every wave left it at the last barrier
    __syncthreads();
  }

  l += __shfl_xor(l, 32, 64);  // the two lane halves summed different key rows
  if (qi >= n) return;
  // lane (query lane & 31, half hh) holds head dims 32 d + 8 g + 4 hh .. + 3 in o[d][4 g .. 4 g + 3]
  if (p.nsplit == 1) {
    const float inv = l > 0.f ? (FP8 ? vs : 1.f) / l : 0.f;  // (e4m3: V dequantised here)
    bf16_t* O = static_cast<bf16_t*>(p.o) + tok * p.ldo + h * HD;
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint2 w;
        w.x = pack2bf(o[d][4 * g + 0] * inv, o[d][4 * g + 1] * inv);
        w.y = pack2bf(o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv);
        *reinterpret_cast<uint2*>(O + 32 * d + 8 * g + 4 * hh) = w;
      }
    return;
  }
  float* wsp = p.ws + ((tok * p.H + h) * p.nsplit + sp) * (HD + 4);
  if constexpr (FP8) {
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[d][r] *= vs;
  }
#pragma unroll
  for (int d = 0; d < NDT; ++d)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(wsp + 32 * d + 8 * g + 4 * hh) =
          make_float4(o[d][4 * g + 0], o[d][4 * g + 1], o[d][4 * g + 2], o[d][4 * g + 3]);
  if (hh == 0) *reinterpret_cast<float2*>(wsp + HD) = make_float2(m, l);
}

// o = sum_s 2^(m_s - M) o_s / sum_s 2^(m_s - M) l_s, M = max m_s; 0 when every split was empty.
// Row = (token, head); 256 / hd rows per workgroup, one thread per head dim.
__global__ __launch_bounds__(ANT) void append_attn_combine_kernel(AppendAttnArgs p) {
  const int hd = p.hd, t = threadIdx.x % hd;
  const long long row = (long long)blockIdx.x * (ANT / hd) + threadIdx.x / hd;
  if (row >= (long long)p.N * p.n * p.H) return;
  const long long tok = row / p.H;
  const int h = (int)(row - tok * p.H);
  const float* wsp = p.ws + row * p.nsplit * (hd + 4);
  float M = -INFINITY;
#pragma unroll 8
  for (int s = 0; s < p.nsplit; ++s) M = fmaxf(M, wsp[s * (hd + 4) + hd]);
  float num = 0.f, den = 0.f;
  if (M > -INFINITY) {
#pragma unroll 8
    for (int s = 0; s < p.nsplit; ++s) {
      const float* ps = wsp + s * (hd + 4);
      const float wgt = ap_exp2(ps[hd] - M);
      num = fmaf(wgt, ps[t], num);
      den = fmaf(wgt, ps[hd + 1], den);
    }
  }
  static_cast<bf16_t*>(p.o)[tok * p.ldo + h * hd + t] = f2bf(den > 0.f ? num / den : 0.f);
}

template <int HD, typename CT = bf16_t>
static void append_attn_launch(const AppendAttnArgs* a, hipStream_t stream, float ks = 1.f, float vs = 1.f) {
  const dim3 grid((unsigned)((a->n + AQB - 1) / AQB), (unsigned)a->nsplit, (unsigned)(a->N * a->H));
  hipLaunchKernelGGL((append_attn_kernel<HD, CT>), grid, dim3(ANT), 0, stream, *a, ks, vs);
}

static bool ap_bad(const AppendAttnArgs* a) {
  return (a->hd != 32 && a->hd != 64 && a->hd != 128) || a->ldqkv % 8 || a->ldo % 8 || a->H <= 0 || a->Smax <= 0 ||
         !(a->scale > 0.f) || a->Smax > (1 << 30) || a->n > (1 << 22) || (long long)a->N * a->H > 65535 || a->nsplit < 1 ||
         a->nsplit > APPEND_MAX_SPLITS || (a->nsplit > 1 && !a->ws) || ((uintptr_t)a->qkv % 16) ||
         ((uintptr_t)a->kc % 16) || ((uintptr_t)a->vc % 16) || ((uintptr_t)a->o % 16) || ((uintptr_t)a->ws % 16);
}

static int ap_combine(const AppendAttnArgs* a, hipStream_t stream) {
  const long long rows = (long long)a->N * a->n * a->H;
  const int rpb = ANT / a->hd;
  hipLaunchKernelGGL(append_attn_combine_kernel, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(ANT), 0, stream, *a);
  return (int)hipGetLastError();
}

static int kv_store_fp8(const AppendAttnArgs* a, float k_inv, float v_inv, hipStream_t stream) {
  const long long chunks = (long long)a->N * a->n * (a->H * a->hd / 8);
  hipLaunchKernelGGL(kv_store_fp8_kernel, dim3((unsigned)((chunks + ANT - 1) / ANT)), dim3(ANT), 0, stream, *a, k_inv, v_inv);
  return (int)hipGetLastError();
}

}  // namespace dpc

using namespace dpc;

// queries per workgroup and keys per tile (the same at every head size): the diagonal's tile
// offsets and the planner's units
DPC_API void dpc_append_attn_tiles(int hd, int* qb, int* kt) {
  (void)hd;
  *qb = AQB;
  *kt = AKT;
}

// Requirements: hd 32, 64 or 128; scale > 0 (the tile maximum is taken on raw scores and scaled
// afterwards); 1 <= nsplit <= 64; Smax <= 2^30; N*H <= 65535; qkv / o / cache
// rows 16-B aligned; ws (nsplit > 1) holds N*n*H*nsplit*(hd + 4) floats.
DPC_API int dpc_append_attn(const AppendAttnArgs* a, hipStream_t stream) {
  if (a->N <= 0 || a->n <= 0) return 0;
  if (ap_bad(a)) return (int)hipErrorInvalidValue;
  const long long chunks = (long long)a->N * a->n * (a->H * a->hd / 4);
  hipLaunchKernelGGL(append_kv_kernel, dim3((unsigned)((chunks + ANT - 1) / ANT)), dim3(ANT), 0, stream, *a);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  switch (a->hd) {
    case 32: append_attn_launch<32>(a, stream); break;
    case 64: append_attn_launch<64>(a, stream); break;
    default: append_attn_launch<128>(a, stream); break;
  }
  rc = (int)hipGetLastError();
  if (rc || a->nsplit == 1) return rc;
  return ap_combine(a, stream);
}

// The quantising store alone: n rows per sequence of qkv's k and v columns into the e4m3 cache at
// rows len[s] + i (those below Smax).  Reads qkv, kc, vc, len, ldqkv, N, n, H, hd, Smax, per_seq and
// the inverse scales; hd 32, 64 or 128.
DPC_API int dpc_kv_store_fp8(const AppendAttnFp8Args* f, hipStream_t stream) {
  if (f->N <= 0 || f->n <= 0) return 0;
  if ((f->hd != 32 && f->hd != 64 && f->hd != 128) || f->ldqkv % 8 || f->H <= 0 || f->Smax <= 0 || f->Smax > (1 << 30) ||
      f->n > (1 << 22) || !(f->k_inv > 0.f) || !(f->v_inv > 0.f) || ((uintptr_t)f->qkv % 16) ||
      ((uintptr_t)f->kc % 16) || ((uintptr_t)f->vc % 16))
    return (int)hipErrorInvalidValue;
  const AppendAttnArgs a = ap_plain(*f);
  return kv_store_fp8(&a, f->k_inv, f->v_inv, stream);
}

// dpc_append_attn over an e4m3 cache: the same requirements, and positive scales.
DPC_API int dpc_append_attn_fp8(const AppendAttnFp8Args* f, hipStream_t stream) {
  if (f->N <= 0 || f->n <= 0) return 0;
  const AppendAttnArgs a = ap_plain(*f);
  if (ap_bad(&a) || !(f->k_scale > 0.f) || !(f->v_scale > 0.f) || !(f->k_inv > 0.f) || !(f->v_inv > 0.f))
    return (int)hipErrorInvalidValue;
  int rc = kv_store_fp8(&a, f->k_inv, f->v_inv, stream);
  if (rc) return rc;
  switch (a.hd) {
    case 32: append_attn_launch<32, fp8_t>(&a, stream, f->k_scale, f->v_scale); break;
    case 64: append_attn_launch<64, fp8_t>(&a, stream, f->k_scale, f->v_scale); break;
    default: append_attn_launch<128, fp8_t>(&a, stream, f->k_scale, f->v_scale); break;
  }
  rc = (int)hipGetLastError();
  if (rc || a.nsplit == 1) return rc;
  return ap_combine(&a, stream);
}
