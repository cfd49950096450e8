// Temperature / top-k / top-p sampling of one token per row of bf16 logits [N][ld].
//
// One workgroup of 1024 threads per row.  The definition is order-free and keeps ties
// (torch twin: ops/sample.py:sample_reference):
//   z_i = logit_i / T;  top-k keeps i iff #{j : z_j > z_i} < k;  top-p keeps i iff the softmax
//   mass (over the top-k survivors) of the strictly greater values is < p;  the token is the
//   first kept index whose inclusive prefix sum of w_i = exp(z_i - max) exceeds u * sum(w).
// T > 0 is monotone, so both cuts are thresholds on the raw 16-bit keys (the bf16 payload mapped
// to an unsigned integer of the same order).  Each threshold is "the largest key x whose
// cumulative weight over keys >= x reaches a target" -- weight 1 and target k for top-k, weight
// w and target p * Z for top-p -- found exactly by two 256-bin histogram passes (high byte,
// then low byte inside the chosen bin).
// The row is read once: every thread keeps its share of the keys in registers (wave w owns the
// columns [w * SEG, (w + 1) * SEG) in chunks of 8 per lane, so the waves and lanes are in index
// order), and every pass runs over the registers -- one workgroup has one CU's vector ALUs for
// 50K columns, so the passes are bound by instructions per column, not by memory.
// Every mass is a 64-bit fixed-point integer (w * 2^40, w <= 1): integer sums do not depend on
// the order the LDS atomics land in, so the same inputs give the same token on every run.
// The draw walks the row in index order: the waves' segment sums locate the wave that holds
// u * Z, and that wave scans its registers 512 columns at a time.
#include "common.h"

namespace dpc {

struct SampleArgs {
  const void* logits;      // [N][ld] bf16; columns >= V are never candidates
  long long* counters;     // [N] draws so far (the hash's counter; incremented here)
  const float* u;          // [N] explicit uniforms, or null: hash of (seed, row, counter)
  long long* out_tok;      // [N] the sampled token
  unsigned char* done;     // [N] or null: set -> emit eos; set when eos is drawn
  long long* seq;          // [N][seq_ld] or null: the token also goes to seq[n][step[n]]
  long long* step;         // [N] with seq: the column, incremented here
  long long* len;          // [N] or null: incremented here (the cache lengths of a decode loop)
  long long ld, seq_ld, eos;
  int N, V, top_k;
  float temperature, top_p;
  unsigned seed_lo, seed_hi;
};

constexpr int SM_NT = 1024;
constexpr int SM_NW = SM_NT / 64;
constexpr float SM_FIX = 1099511627776.f;  // 2^40

// bf16 payload -> 16-bit key with the order of the values (-0 is +0).  Key 0 -- the payload
// 0xffff, a NaN -- marks a column that is not there.
__device__ __forceinline__ unsigned key_of(unsigned b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

__device__ __forceinline__ float val_of_key(unsigned k) {
  const unsigned b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
  return __uint_as_float(b << 16);
}

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
  const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long shfl64_up(unsigned long long v, int d) {
  const unsigned lo = __shfl_up((unsigned)v, d, 64), hi = __shfl_up((unsigned)(v >> 32), d, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// host twin: ops/sample.py:sample_uniform
__device__ __forceinline__ float sample_uniform(unsigned seed_lo, unsigned seed_hi, unsigned row,
                                                unsigned long long counter) {
  unsigned x = fmix32(seed_lo);
  x = fmix32(x ^ (seed_hi * 0x9E3779B1u));
  x = fmix32(x ^ (row * 0x85EBCA77u + 0x632BE5ABu));
  x = fmix32(x ^ (unsigned)counter);
  x = fmix32(x ^ ((unsigned)(counter >> 32) * 0x9E3779B1u));
  return (float)(x >> 8) * (1.f / 16777216.f);
}

// The largest bin b whose cumulative weight over bins >= b reaches the target, and the weight
// of the bins above it.  The target is `target` (>= 1), or with frac >= 0 the fraction `frac` of
// the histogram's total, rounded up; it is capped at the total.  Wave 0 does the search (lane l
// owns bins 4l .. 4l+3) and leaves {bin, weight above, target} in res[0..2]; the caller
// synchronises before reading them.
template <class T>
__device__ __forceinline__ void hist_search(const T* hist, unsigned long long target, float frac,
                                            unsigned long long* res) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  unsigned long long h[4], own = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = (unsigned long long)hist[4 * lane + i];
    own += h[i];
  }
  // suffix sum over this lane and the lanes above it
  unsigned long long suf = own;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long t = shfl64(suf, lane + d < 64 ? lane + d : lane);
    if (lane + d < 64) suf += t;
  }
  const unsigned long long total = shfl64(suf, 0);
  if (frac >= 0.f) target = (unsigned long long)ceil((double)frac * (double)total);
  if (target > total) target = total;
  if (target < 1) target = 1;
  unsigned long long above = suf - own;  // bins > 4 lane + 3
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    const unsigned long long ge = above + h[i];
    if (above < target && ge >= target) {
      res[0] = (unsigned long long)(4 * lane + i);
      res[1] = above;
      res[2] = target;
    }
    above = ge;
  }
}

// ITERS chunks of 8 columns per lane: rows of up to SM_NW * 512 * ITERS columns
template <int ITERS>
__global__ __launch_bounds__(SM_NT) void sample_kernel(SampleArgs p) {
  __shared__ unsigned long long hist[256];
  __shared__ unsigned cnt[256];
  __shared__ unsigned long long res[3];
  __shared__ unsigned long long wsum[SM_NW];
  __shared__ unsigned redu[SM_NW];
  __shared__ long long pick;
  constexpr int NE = ITERS * 8, SEG = ITERS * 512;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = blockIdx.x, V = p.V;
  const bf16_t* row = static_cast<const bf16_t*>(p.logits) + (long long)n * p.ld;
  const int base = wv * SEG + lane * 8;  // element i of this thread: column base + (i / 8) * 512 + i % 8

  const long long counter = p.counters[n];
  const bool was_done = p.done && p.done[n];

  // ---- the row into registers: two 16-bit keys per dword
  unsigned kp[ITERS * 4];
  const bool aligned = ((uintptr_t)row % 16) == 0;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int j = base + it * 512;
    unsigned b[8];
    if (aligned && j + 8 <= V) {
      const uint4 v = *reinterpret_cast<const uint4*>(row + j);
      const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        b[2 * e] = w4[e] & 0xffffu;
        b[2 * e + 1] = w4[e] >> 16;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = j + e < V ? (unsigned)row[j + e] : 0xffffu;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) kp[it * 4 + e] = key_of(b[2 * e]) | (key_of(b[2 * e + 1]) << 16);
  }
  // f(key, column) for each of this thread's NE elements, in index order
  auto each = [&](auto&& f) {
    sfor<NE>([&](auto I) {
      constexpr int i = decltype(I)::value;
      f((kp[i >> 1] >> ((i & 1) * 16)) & 0xffffu, base + (i >> 3) * 512 + (i & 7));
    });
  };

  // ---- the largest key (tmax: this thread's own)
  unsigned tmax = 0;
  each([&](unsigned k, int) { tmax = max(tmax, k); });
  unsigned kmax = tmax;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor(kmax, o, 64));
  if (lane == 0) redu[wv] = kmax;
  __syncthreads();
  kmax = 0;
#pragma unroll
  for (int i = 0; i < SM_NW; ++i) kmax = max(kmax, redu[i]);
  __syncthreads();

  long long token;
  if (p.temperature <= 0.f) {
    // ---- greedy: the lowest index holding the largest value
    unsigned best = 0xffffffffu;
    each([&](unsigned k, int j) {
      if (k == kmax) best = min(best, (unsigned)j);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor(best, o, 64));
    if (lane == 0) redu[wv] = best;
    __syncthreads();
    best = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < SM_NW; ++i) best = min(best, redu[i]);
    token = (long long)min(best, (unsigned)(V - 1));
  } else {
    const float vmax = val_of_key(kmax);
    const float c = 1.4426950408889634f / p.temperature;
    // w = exp(z - zmax) in 2^-40 fixed point
    auto weight = [&](unsigned key) -> unsigned long long {
      return (unsigned long long)(__builtin_amdgcn_exp2f((val_of_key(key) - vmax) * c) * SM_FIX);
    };
    unsigned thr = 1;  // keep iff key >= thr (key 0: no column)

    // ---- top-k: the k-th largest key, by count
    if (p.top_k > 0 && p.top_k < V) {
      // The k-th largest of the threads' own maxima is a lower bound of the k-th largest key
      // (those k maxima are k columns): only keys from its bin up need counting, which spares
      // the LDS atomics of almost the whole row.
      unsigned lb = 1;
      if (p.top_k <= SM_NT) {
        if (tid < 256) cnt[tid] = 0;
        __syncthreads();
        atomicAdd(&cnt[tmax >> 8], 1u);
        __syncthreads();
        hist_search(cnt, (unsigned long long)p.top_k, -1.f, res);
        __syncthreads();
        lb = max(1u, (unsigned)res[0] << 8);
        __syncthreads();
      }
      unsigned long long target = (unsigned long long)p.top_k;
      unsigned hi_bin = 0;
      for (int level = 0; level < 2; ++level) {
        if (tid < 256) cnt[tid] = 0;
        __syncthreads();
        each([&](unsigned k, int) {
          if (k < lb) return;
          if (level == 0) atomicAdd(&cnt[k >> 8], 1u);
          else if ((k >> 8) == hi_bin) atomicAdd(&cnt[k & 255u], 1u);
        });
        __syncthreads();
        hist_search(cnt, target, -1.f, res);
        __syncthreads();
        if (level == 0) {
          hi_bin = (unsigned)res[0];
          target = res[2] - res[1];
        } else {
          thr = max(1u, (hi_bin << 8) | (unsigned)res[0]);
        }
        __syncthreads();
      }
    }

    // ---- top-p: the largest key whose mass of keys >= it reaches p * Z (Z over the survivors)
    if (p.top_p < 1.f) {
      unsigned long long target = 0;
      unsigned hi_bin = 0;
      const unsigned kthr = thr;
      for (int level = 0; level < 2; ++level) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        each([&](unsigned k, int) {
          if (k < kthr) return;
          if (level == 0) atomicAdd(&hist[k >> 8], weight(k));
          else if ((k >> 8) == hi_bin) atomicAdd(&hist[k & 255u], weight(k));
        });
        __syncthreads();
        hist_search(hist, target, level == 0 ? fmaxf(p.top_p, 0.f) : -1.f, res);
        __syncthreads();
        if (level == 0) {
          hi_bin = (unsigned)res[0];
          target = res[2] - res[1];
        } else {
          thr = max(kthr, (hi_bin << 8) | (unsigned)res[0]);
        }
        __syncthreads();
      }
    }

    // ---- draw in index order: wave wv holds the columns [wv * SEG, (wv + 1) * SEG)
    unsigned long long part = 0;
    each([&](unsigned k, int) {
      if (k >= thr) part += weight(k);
    });
    part = wave_sum64(part);
    if (lane == 0) wsum[wv] = part;
    if (tid == 0) pick = -1;
    __syncthreads();
    unsigned long long z = 0;
#pragma unroll
    for (int i = 0; i < SM_NW; ++i) z += wsum[i];
    const float uf = p.u ? p.u[n] : sample_uniform(p.seed_lo, p.seed_hi, (unsigned)n, (unsigned long long)counter);
    // prefix > u * Z  <=>  prefix > floor(u * Z) for integer prefixes
    unsigned long long target = (unsigned long long)((double)fminf(fmaxf(uf, 0.f), 1.f) * (double)z);
    if (z > 0 && target >= z) target = z - 1;
    unsigned long long before = 0;
    int owner = -1;
#pragma unroll
    for (int i = 0; i < SM_NW; ++i) {
      if (owner < 0 && before + wsum[i] > target) owner = i;
      if (owner < 0) before += wsum[i];
    }
    if (wv == owner) {
      unsigned long long run = before;
      bool found = false;
      sfor<ITERS>([&](auto IT) {
        constexpr int it = decltype(IT)::value;
        if (found) return;  // (wave-uniform)
        unsigned long long w[8], s = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned k = (kp[it * 4 + (e >> 1)] >> ((e & 1) * 16)) & 0xffffu;
          w[e] = k >= thr ? weight(k) : 0ull;
          s += w[e];
        }
        unsigned long long inc = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const unsigned long long t = shfl64_up(inc, d);
          if (lane >= d) inc += t;
        }
        // the first lane whose inclusive prefix exceeds the target holds the column
        const unsigned long long hit = __ballot(run + inc > target);
        if (hit) {
          found = true;
          if (lane == __builtin_ctzll(hit)) {
            unsigned long long acc = run + inc - s;
            int e_hit = -1;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              acc += w[e];
              if (e_hit < 0 && w[e] > 0 && acc > target) e_hit = e;
            }
            pick = (long long)(base + it * 512 + e_hit);
          }
        }
        run += shfl64(inc, 63);
      });
    }
    __syncthreads();
    token = pick;
    if (token < 0) {
      // nothing exceeded the target (every kept weight rounded to 0): the last kept index
      unsigned last = 0;
      each([&](unsigned k, int j) {
        if (k >= thr) last = max(last, (unsigned)j);
      });
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) last = max(last, (unsigned)__shfl_xor(last, o, 64));
      if (lane == 0) redu[wv] = last;
      __syncthreads();
      last = 0;
#pragma unroll
      for (int i = 0; i < SM_NW; ++i) last = max(last, redu[i]);
      token = (long long)last;
    }
  }

  if (tid == 0) {
    if (was_done) token = p.eos;
    else if (p.done && token == p.eos) p.done[n] = 1;
    p.out_tok[n] = token;
    p.counters[n] = counter + 1;
    if (p.seq) {
      const long long s = p.step[n];
      if (s >= 0 && s < p.seq_ld) p.seq[(long long)n * p.seq_ld + s] = token;
      p.step[n] = s + 1;
    }
    if (p.len) p.len[n] += 1;
  }
}

constexpr int SM_MAX_ITERS = 7;  // 28 key registers per thread; more spills at 1024 threads
constexpr int SM_MAX_V = SM_NW * 512 * SM_MAX_ITERS;

}  // namespace dpc

using namespace dpc;

// Requirements: 1 <= V <= min(ld, 57344).
DPC_API int dpc_sample(const SampleArgs* a, hipStream_t stream) {
  if (a->N <= 0) return 0;
  if (a->V <= 0 || a->V > SM_MAX_V || a->ld < a->V || !a->logits || !a->counters || !a->out_tok ||
      (a->seq && (!a->step || a->seq_ld <= 0)))
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)a->N), block(SM_NT);
  if (a->V <= SM_NW * 512) hipLaunchKernelGGL(sample_kernel<1>, grid, block, 0, stream, *a);
  else hipLaunchKernelGGL(sample_kernel<SM_MAX_ITERS>, grid, block, 0, stream, *a);
  return (int)hipGetLastError();
}
