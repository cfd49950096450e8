// Split-KV ("flash-decoding") single-query attention for KV-cache decoding: any cache length,
// and enough workgroups to fill the part at small batch.
//
// decode_attn_split_kernel<P>, grid (N*H, nsplit), 4 waves.  nsplit is fixed on the host and the
// length is read on the device, so the launch has no length-dependent shape and can be captured
// in a HIP graph.  Split s owns the keys [s chunk, min(L, (s + 1) chunk)), chunk = ceil(L / nsplit)
// rounded up to the workgroup's keys per pass (DS_NW * 64 / P); a split past L owns nothing.
//
// A key row (hd bf16) is read by P adjacent lanes, 16 B each, P the next power of two at or above
// hd / 8 (lanes c >= hd / 8 idle), so a wave covers 64 / P keys per pass with whole-row loads and
// the workgroup DS_NW times that.  DS_U passes are unrolled: the K chunk and the V chunk of all of
// them are issued before the first score is formed (V does not depend on it), 2 DS_U independent
// 16-B loads in flight per lane.  The score is an 8-element partial dot per lane and a log2 P-step
// butterfly over the group; every lane group is its own online-softmax stream in registers
// (running m and l, a[8] for the 8 head dims the lane owns; base-2 exponentials, log2(e) folded
// into q; one rescale per DS_U keys).  No LDS score buffer, so no bound on the cache length.  At
// the end of the range the streams merge across the lane groups of a wave with shuffles and across
// the waves through DS_NW * P * 10 floats of LDS.  nsplit == 1 normalises and stores bf16 o;
// otherwise f32 (m, l, a[hd]) go to the workspace [N*H][nsplit][hd + 2] and
// decode_attn_combine_kernel (one thread per head dim, the partials in index order, no atomics:
// the same inputs give the same bits on every run) writes o.
//
// The new token's key / value are read from qkv, never from the cache, by the split that owns
// position len; that workgroup alone appends the row, and no workgroup reads cache row len, so
// the append races with no read.  A full cache (len >= Smax or len < 0) appends nothing and gives
// a zero row with any nsplit: L = 0, every range is empty, every partial is (-inf, 0, 0).
//
// One query row per (sequence, head) and a K/V stream private to each: there is no tile for MFMA
// to reuse, the work is a read of the cache on the vector ALUs.
//
// decode_attn_split_fp8_kernel<HD> (hd 32, 64, 128): the same split / merge / combine over a 1-byte
// e4m3 cache (fp8.h).  A lane's 16-B chunk is 16 head dims, so a key row takes P = HD / 16 lanes
// (2, 4, 8), a wave covers 64 / P keys per pass -- twice the bf16 kernel's -- and a lane keeps
// q[16] and a[16]; the butterfly is log2 P steps.  DS_U = 4 passes stay unrolled: 8 independent
// 16-B loads per lane in flight (K and V of 4 passes), the same count and twice the keys of the
// bf16 kernel; more would hold > 32 VGPRs of raw chunks beside q and a (110 VGPRs as built).  A
// loop pipelined over two register sets (the next block's loads issued before this block's
// converts) was measured and not kept: faster at one split, slower at the planner's counts.
// Each dword goes through v_cvt_pk_f32_fp8 (low and high half) straight into the v_fma_f32 of
// the dot / the accumulator.  k_scale rides on q (scale log2(e) k_scale), v_scale on the accumulator as it
// leaves (o, or a split's partial), so the workspace and decode_attn_combine_kernel are the bf16
// kernel's.  Quantise first, then attend: the workgroup that owns pos forms the new row's e4m3
// chunks in registers, appends them with 16-B stores, and every lane that meets key pos takes
// those registers, never the cache row -- the token weighs the same now and in every later step.
#include "fp8.h"

namespace dpc {

struct DecodeSplitArgs {     // DecodeAttnArgs (decode.hip) + ws, nsplit
  const void* qkv;           // [N][ldqkv] bf16: q | k | v blocks of H*hd each
  void* kc;                  // [N][Smax][E] bf16 key cache
  void* vc;                  // [N][Smax][E] bf16 value cache
  void* o;                   // [N][ldo] bf16
  const long long* len;      // device: cached tokens before this one ([1], or [N] with per_seq)
  long long ldqkv, ldo;
  int N, H, hd, Smax;
  float scale;
  int per_seq;
  float* ws;                 // [N*H][nsplit][hd + 2] f32: m, l, a[hd]  (nsplit > 1)
  int nsplit;
};

constexpr int DS_NW = 4;           // waves per workgroup
constexpr int DS_NT = 64 * DS_NW;
constexpr int DS_U = 4;            // passes in flight
constexpr int DS_MAX_SPLITS = 64;

__device__ __forceinline__ float ds_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// stream (m2, l2, a2) into (m, l, a); two empty streams (m = -inf) stay empty
template <int NE = 8>
__device__ __forceinline__ void ds_merge(float& m, float& l, float* a, float m2, float l2, const float* a2) {
  const float mn = fmaxf(m, m2);
  const float mm = mn == -INFINITY ? 0.f : mn;
  const float c1 = ds_exp2(m - mm), c2 = ds_exp2(m2 - mm);
  l = l * c1 + l2 * c2;
#pragma unroll
  for (int e = 0; e < NE; ++e) a[e] = a[e] * c1 + a2[e] * c2;
  m = mn;
}

template <int P>
__global__ __launch_bounds__(DS_NT) void decode_attn_split_kernel(DecodeSplitArgs p) {
  constexpr int G = 64 / P;        // keys per wave per pass
  constexpr int KPP = DS_NW * G;   // keys per workgroup per pass
  __shared__ float red[DS_NW][P][10];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane % P, g = lane / P;
  const int n = blockIdx.x / p.H, h = blockIdx.x % p.H, s = blockIdx.y;
  const int hd = p.hd, E = p.H * hd, nc = hd >> 3;
  const long long pos = p.per_seq ? p.len[n] : *p.len;
  const bool live = pos >= 0 && pos < p.Smax;  // else a full cache: append nothing, attend to nothing
  const int L = live ? (int)pos + 1 : 0;
  const int chunk = ((L + p.nsplit - 1) / p.nsplit + KPP - 1) / KPP * KPP;
  const int start = s * chunk, end = min(L, start + chunk);

  const bf16_t* qrow = static_cast<const bf16_t*>(p.qkv) + n * p.ldqkv + h * hd;
  const bf16_t* knew = qrow + E;
  const bf16_t* vnew = qrow + 2 * E;
  bf16_t* kc = static_cast<bf16_t*>(p.kc) + (long long)n * p.Smax * E + h * hd;
  bf16_t* vc = static_cast<bf16_t*>(p.vc) + (long long)n * p.Smax * E + h * hd;
  // the owner of pos appends the new row (every load of key pos below comes from qkv)
  if (live && pos >= start && pos < end && tid < 2 * nc) {
    const bool isk = tid < nc;
    const int cc = isk ? tid : tid - nc;
    reinterpret_cast<uint4*>((isk ? kc : vc) + pos * E)[cc] = reinterpret_cast<const uint4*>(isk ? knew : vnew)[cc];
  }

  const bool act = c < nc;
  float q[8];
  {
    uint4 qv = make_uint4(0u, 0u, 0u, 0u);
    if (act) qv = reinterpret_cast<const uint4*>(qrow)[c];
    unpack8(qv, q);
    const float sl = p.scale * 1.4426950408889634f;  // scores in log2 units
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] *= sl;
  }
  float m = -INFINITY, l = 0.f;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  for (int b0 = start; b0 < end; b0 += DS_U * KPP) {
    const int b = b0 + w * G + g;  // this lane group's key of pass 0
    uint4 kv[DS_U], vv[DS_U];
#pragma unroll
    for (int u = 0; u < DS_U; ++u) {
      const int j = b + u * KPP;
      kv[u] = make_uint4(0u, 0u, 0u, 0u);
      vv[u] = make_uint4(0u, 0u, 0u, 0u);
      if (act && j < end) {
        kv[u] = reinterpret_cast<const uint4*>(j == pos ? knew : kc + (long long)j * E)[c];
        vv[u] = reinterpret_cast<const uint4*>(j == pos ? vnew : vc + (long long)j * E)[c];
      }
    }
    float sc[DS_U];
    float mb = m;
#pragma unroll
    for (int u = 0; u < DS_U; ++u) {
      float f[8];
      unpack8(kv[u], f);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d = fmaf(f[e], q[e], d);
#pragma unroll
      for (int o = P / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
      sc[u] = b + u * KPP < end ? d : -INFINITY;
      mb = fmaxf(mb, sc[u]);
    }
    const float mm = mb == -INFINITY ? 0.f : mb;
    const float alpha = ds_exp2(m - mm);
    l *= alpha;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] *= alpha;
#pragma unroll
    for (int u = 0; u < DS_U; ++u) {
      const float pj = ds_exp2(sc[u] - mm);
      float f[8];
      unpack8(vv[u], f);
      l += pj;
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = fmaf(pj, f[e], a[e]);
    }
    m = mb;
  }

  // the lane groups of the wave, then the waves
#pragma unroll
  for (int o = P; o < 64; o <<= 1) {
    const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
    float a2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a2[e] = __shfl_xor(a[e], o, 64);
    ds_merge(m, l, a, m2, l2, a2);
  }
  if (g == 0) {
    red[w][c][0] = m;
    red[w][c][1] = l;
#pragma unroll
    for (int e = 0; e < 8; ++e) red[w][c][2 + e] = a[e];
  }
  __syncthreads();
  if (tid >= P) return;  // wave 0, g == 0, c == tid
#pragma unroll
  for (int ww = 1; ww < DS_NW; ++ww) ds_merge(m, l, a, red[ww][c][0], red[ww][c][1], &red[ww][c][2]);
  if (p.nsplit == 1) {
    if (!act) return;
    const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] *= inv;
    reinterpret_cast<uint4*>(static_cast<bf16_t*>(p.o) + n * p.ldo + h * hd)[c] = pack8(a);
    return;
  }
  float* wsp = p.ws + ((long long)blockIdx.x * p.nsplit + s) * (hd + 2);
  if (c == 0) {
    wsp[0] = m;
    wsp[1] = l;
  }
  if (act) {
#pragma unroll
    for (int e = 0; e < 8; ++e) wsp[2 + c * 8 + e] = a[e];
  }
}

struct DecodeSplitFp8Args {  // DecodeSplitArgs (kc / vc e4m3) + the cache's scales
  const void* qkv;
  void* kc;
  void* vc;
  void* o;
  const long long* len;
  long long ldqkv, ldo;
  int N, H, hd, Smax;
  float scale;
  int per_seq;
  float* ws;
  int nsplit;
  float k_scale, k_inv, v_scale, v_inv;
};

template <int HD>
__global__ __launch_bounds__(DS_NT) void decode_attn_split_fp8_kernel(DecodeSplitFp8Args p) {
  constexpr int P = HD / 16;       // lanes per key row
  constexpr int G = 64 / P;        // keys per wave per pass
  constexpr int KPP = DS_NW * G;   // keys per workgroup per pass
  __shared__ float red[DS_NW][P][18];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane % P, g = lane / P;
  const int n = blockIdx.x / p.H, h = blockIdx.x % p.H, s = blockIdx.y;
  const int E = p.H * HD;
  const long long pos = p.per_seq ? p.len[n] : *p.len;
  const bool live = pos >= 0 && pos < p.Smax;  // else a full cache: append nothing, attend to nothing
  const int L = live ? (int)pos + 1 : 0;
  const int chunk = ((L + p.nsplit - 1) / p.nsplit + KPP - 1) / KPP * KPP;
  const int start = s * chunk, end = min(L, start + chunk);

  const bf16_t* qrow = static_cast<const bf16_t*>(p.qkv) + n * p.ldqkv + h * HD;
  fp8_t* kc = static_cast<fp8_t*>(p.kc) + (long long)n * p.Smax * E + h * HD;
  fp8_t* vc = static_cast<fp8_t*>(p.vc) + (long long)n * p.Smax * E + h * HD;
  // the owner of pos: chunk c of the new row as stored, formed in registers; lanes 0 .. 2 P - 1
  // append it (every use of key pos below takes kn / vn, never the cache row)
  uint4 kn = make_uint4(0u, 0u, 0u, 0u), vn = kn;
  if (live && pos >= start && pos < end) {  // workgroup-uniform
    const uint4* ks = reinterpret_cast<const uint4*>(qrow + E) + 2 * c;
    const uint4* vs = reinterpret_cast<const uint4*>(qrow + 2 * E) + 2 * c;
    kn = fp8_quant16(ks[0], ks[1], p.k_inv);
    vn = fp8_quant16(vs[0], vs[1], p.v_inv);
    if (tid < P) reinterpret_cast<uint4*>(kc + pos * E)[c] = kn;
    else if (tid < 2 * P) reinterpret_cast<uint4*>(vc + pos * E)[c] = vn;
  }

  float q[16];
  {
    const uint4* qs = reinterpret_cast<const uint4*>(qrow) + 2 * c;
    unpack8(qs[0], q);
    unpack8(qs[1], q + 8);
    const float sl = p.scale * 1.4426950408889634f * p.k_scale;  // scores in log2 units, K dequantised
#pragma unroll
    for (int e = 0; e < 16; ++e) q[e] *= sl;
  }
  float m = -INFINITY, l = 0.f;
  float a[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) a[e] = 0.f;

  for (int b0 = start; b0 < end; b0 += DS_U * KPP) {
    const int b = b0 + w * G + g;  // this lane group's key of pass 0
    uint4 kv[DS_U], vv[DS_U];
#pragma unroll
    for (int u = 0; u < DS_U; ++u) {
      const int j = b + u * KPP;
      kv[u] = make_uint4(0u, 0u, 0u, 0u);
      vv[u] = make_uint4(0u, 0u, 0u, 0u);
      if (j == pos) {
        kv[u] = kn;
        vv[u] = vn;
      } else if (j < end) {
        kv[u] = reinterpret_cast<const uint4*>(kc + (long long)j * E)[c];
        vv[u] = reinterpret_cast<const uint4*>(vc + (long long)j * E)[c];
      }
    }
    float sc[DS_U];
    float mb = m;
#pragma unroll
    for (int u = 0; u < DS_U; ++u) {
      float f[16];
      fp8_unpack16(kv[u], f);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) d = fmaf(f[e], q[e], d);
#pragma unroll
      for (int o = P / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
      sc[u] = b + u * KPP < end ? d : -INFINITY;
      mb = fmaxf(mb, sc[u]);
    }
    const float mm = mb == -INFINITY ? 0.f : mb;
    const float alpha = ds_exp2(m - mm);
    l *= alpha;
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] *= alpha;
#pragma unroll
    for (int u = 0; u < DS_U; ++u) {
      const float pj = ds_exp2(sc[u] - mm);
      float f[16];
      fp8_unpack16(vv[u], f);
      l += pj;
#pragma unroll
      for (int e = 0; e < 16; ++e) a[e] = fmaf(pj, f[e], a[e]);
    }
    m = mb;
  }

  // the lane groups of the wave, then the waves
#pragma unroll
  for (int o = P; o < 64; o <<= 1) {
    const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
    float a2[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) a2[e] = __shfl_xor(a[e], o, 64);
    ds_merge<16>(m, l, a, m2, l2, a2);
  }
  if (g == 0) {
    red[w][c][0] = m;
    red[w][c][1] = l;
#pragma unroll
    for (int e = 0; e < 16; ++e) red[w][c][2 + e] = a[e];
  }
  __syncthreads();
  if (tid >= P) return;  // wave 0, g == 0, c == tid
#pragma unroll
  for (int ww = 1; ww < DS_NW; ++ww) ds_merge<16>(m, l, a, red[ww][c][0], red[ww][c][1], &red[ww][c][2]);
  if (p.nsplit == 1) {
    const float inv = l > 0.f ? p.v_scale / l : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] *= inv;
    uint4* od = reinterpret_cast<uint4*>(static_cast<bf16_t*>(p.o) + n * p.ldo + h * HD) + 2 * c;
    od[0] = pack8(a);
    od[1] = pack8(a + 8);
    return;
  }
  float* wsp = p.ws + ((long long)blockIdx.x * p.nsplit + s) * (HD + 2);
  if (c == 0) {
    wsp[0] = m;
    wsp[1] = l;
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) wsp[2 + c * 16 + e] = a[e] * p.v_scale;
}

// o = sum_s 2^(m_s - M) a_s / sum_s 2^(m_s - M) l_s, M = max m_s; 0 when every split was empty
__global__ __launch_bounds__(256) void decode_attn_combine_kernel(DecodeSplitArgs p) {
  const int t = threadIdx.x, hd = p.hd;
  if (t >= hd) return;
  const int n = blockIdx.x / p.H, h = blockIdx.x % p.H;
  const float* wsp = p.ws + (long long)blockIdx.x * p.nsplit * (hd + 2);
  // (unrolled: the partials come from memory, and a rolled loop waits for each load in turn)
  float M = -INFINITY;
#pragma unroll 8
  for (int s = 0; s < p.nsplit; ++s) M = fmaxf(M, wsp[s * (hd + 2)]);
  float num = 0.f, den = 0.f;
  if (M > -INFINITY) {
#pragma unroll 8
    for (int s = 0; s < p.nsplit; ++s) {
      const float* ps = wsp + s * (hd + 2);
      const float wgt = ds_exp2(ps[0] - M);
      num = fmaf(wgt, ps[2 + t], num);
      den = fmaf(wgt, ps[1], den);
    }
  }
  static_cast<bf16_t*>(p.o)[n * p.ldo + h * hd + t] = f2bf(den > 0.f ? num / den : 0.f);
}

static int ds_lanes(int hd) {  // P: the next power of two at or above hd / 8
  int P = 1;
  while (P * 8 < hd) P *= 2;
  return P;
}

}  // namespace dpc

using namespace dpc;

// keys one workgroup covers per pass at head size hd (split boundaries are multiples of it)
DPC_API int dpc_decode_split_keys_per_pass(int hd) { return DS_NW * 64 / ds_lanes(hd); }

// Requirements: hd % 8 == 0, hd <= 256, 1 <= nsplit <= 64, Smax <= 2^30, qkv / o / cache rows
// 16-B aligned; ws (nsplit > 1) holds N*H*nsplit*(hd + 2) floats.
DPC_API int dpc_decode_attn_split(const DecodeSplitArgs* a, hipStream_t stream) {
  if (a->N <= 0) return 0;
  if (a->hd <= 0 || a->hd % 8 || a->hd > 256 || a->ldqkv % 8 || a->ldo % 8 || a->H <= 0 || a->Smax <= 0 ||
      a->Smax > (1 << 30) || a->nsplit < 1 || a->nsplit > DS_MAX_SPLITS || (a->nsplit > 1 && !a->ws) ||
      ((uintptr_t)a->qkv % 16) || ((uintptr_t)a->kc % 16) || ((uintptr_t)a->vc % 16) || ((uintptr_t)a->o % 16))
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)(a->N * a->H), (unsigned)a->nsplit);
  switch (ds_lanes(a->hd)) {
    case 1: hipLaunchKernelGGL(decode_attn_split_kernel<1>, grid, dim3(DS_NT), 0, stream, *a); break;
    case 2: hipLaunchKernelGGL(decode_attn_split_kernel<2>, grid, dim3(DS_NT), 0, stream, *a); break;
    case 4: hipLaunchKernelGGL(decode_attn_split_kernel<4>, grid, dim3(DS_NT), 0, stream, *a); break;
    case 8: hipLaunchKernelGGL(decode_attn_split_kernel<8>, grid, dim3(DS_NT), 0, stream, *a); break;
    case 16: hipLaunchKernelGGL(decode_attn_split_kernel<16>, grid, dim3(DS_NT), 0, stream, *a); break;
    default: hipLaunchKernelGGL(decode_attn_split_kernel<32>, grid, dim3(DS_NT), 0, stream, *a); break;
  }
  int rc = (int)hipGetLastError();
  if (rc || a->nsplit == 1) return rc;
  hipLaunchKernelGGL(decode_attn_combine_kernel, dim3((unsigned)(a->N * a->H)), dim3((unsigned)((a->hd + 63) / 64 * 64)),
                     0, stream, *a);
  return (int)hipGetLastError();
}

// keys one workgroup of the fp8 kernel covers per pass (hd 32, 64, 128)
DPC_API int dpc_decode_fp8_keys_per_pass(int hd) { return DS_NW * 64 / (hd / 16); }

// The e4m3 cache.  Requirements: hd 32, 64 or 128, 1 <= nsplit <= 64, Smax <= 2^30, positive
// scales, qkv / o / cache rows 16-B aligned; ws (nsplit > 1) holds N*H*nsplit*(hd + 2) floats.
DPC_API int dpc_decode_attn_split_fp8(const DecodeSplitFp8Args* a, hipStream_t stream) {
  if (a->N <= 0) return 0;
  if ((a->hd != 32 && a->hd != 64 && a->hd != 128) || a->ldqkv % 8 || a->ldo % 8 || a->H <= 0 || a->Smax <= 0 ||
      a->Smax > (1 << 30) || a->nsplit < 1 || a->nsplit > DS_MAX_SPLITS || (a->nsplit > 1 && !a->ws) ||
      !(a->k_scale > 0.f) || !(a->v_scale > 0.f) || !(a->k_inv > 0.f) || !(a->v_inv > 0.f) ||
      ((uintptr_t)a->qkv % 16) || ((uintptr_t)a->kc % 16) || ((uintptr_t)a->vc % 16) || ((uintptr_t)a->o % 16))
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)(a->N * a->H), (unsigned)a->nsplit);
  switch (a->hd) {
    case 32: hipLaunchKernelGGL(decode_attn_split_fp8_kernel<32>, grid, dim3(DS_NT), 0, stream, *a); break;
    case 64: hipLaunchKernelGGL(decode_attn_split_fp8_kernel<64>, grid, dim3(DS_NT), 0, stream, *a); break;
    default: hipLaunchKernelGGL(decode_attn_split_fp8_kernel<128>, grid, dim3(DS_NT), 0, stream, *a); break;
  }
  int rc = (int)hipGetLastError();
  if (rc || a->nsplit == 1) return rc;
  DecodeSplitArgs cb = {};  // the combine reads o, ldo, H, hd, ws, nsplit
  cb.o = a->o;
  cb.ldo = a->ldo;
  cb.N = a->N;
  cb.H = a->H;
  cb.hd = a->hd;
  cb.ws = a->ws;
  cb.nsplit = a->nsplit;
  hipLaunchKernelGGL(decode_attn_combine_kernel, dim3((unsigned)(a->N * a->H)), dim3((unsigned)((a->hd + 63) / 64 * 64)),
                     0, stream, cb);
  return (int)hipGetLastError();
}
