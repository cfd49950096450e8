// bf16 MFMA GEMM for gfx950 with fused epilogues.
//
//   C[m, n] = epilogue( alpha * sum_k A[m, k] * B[n, k] )
//
// Operand storage (template flags):
//   A_KMAJ = true : A stored [M][lda] (k contiguous)   -- activations in forward / dgrad
//   A_KMAJ = false: A stored [K][lda] (m contiguous)   -- dY^T in wgrad
//   B_KMAJ = true : B stored [N][ldb] (k contiguous)   -- nn.Linear weight [out, in] in forward
//   B_KMAJ = false: B stored [K][ldb] (n contiguous)   -- weight in dgrad, X in wgrad
// so one kernel family covers the three products of a Linear layer without any explicit
// transpose pass (reference: every nn.Linear of models/gpt.py).
//
// Tiling (CDNA4): 128x128 output tile per 256-thread workgroup (4 waves in 2x2), each
// wave owns 64x64 = 4x4 tiles of v_mfma_f32_16x16x32_bf16.  BK = 64, two LDS stages
// (64 KiB -> 2 workgroups per CU), register-staged global->LDS copies issued one k-tile
// ahead (async-STAGE split: loads before the MFMA block, LDS writes after it).
//   * k-major tiles live in LDS as [row][64] bf16 (128-B rows) with a 16-B chunk XOR
//     swizzle  chunk ^ ((row >> 1) & 7)  -> fragment reads (ds_read_b128) are conflict free.
//   * mn-major tiles live as [k][128] bf16 (256-B rows) with a 32-B block XOR swizzle
//     blk ^ ((k & 3) | ((k >> 3) & 1) << 2) and are read with ds_read_b64_tr_b16, the
//     CDNA4 transposing LDS read, which yields the k-run per lane that MFMA wants.
//   * workgroup ids are remapped so consecutive tiles share an XCD (private L2), then
//     walked in GROUP_M-row supertiles for operand reuse.
#include "gemm9_kern.h"
// the persistent kernels' instantiations are compiled in gemm7_part*.hip (ops/gen_gemm_parts.py)
#define G7_SIG (dpc::GemmArgs, unsigned long long, unsigned long long, dpc::G7Plan)
#define G7_INST(F, K, ...) extern template __global__ void dpc::K<__VA_ARGS__> G7_SIG;
#include "gemm7_extern.inc"
#undef G7_INST

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace dpc {


// Which output tile and k-range a workgroup computes.  The grid is 1-D, ntiles x splits
// workgroups (splits = |ksplit|, set by the dispatcher; 0 = 1), and block b runs on XCD b % 8.
//  * default (ksplit >= 0): a bijective remap gives every XCD a contiguous run of work ids,
//    split-major (id = split * ntiles + tile), walked in GROUP_M supertiles: the workgroups
//    that share an XCD's L2 compute the SAME k-range of neighbouring tiles, so each k-slice of
//    both operands is fetched into that L2 once and read by all of them.  (A 2-D grid with the
//    split on blockIdx.y put block (x, y) on XCD (x + ntiles * y) % 8 -- every XCD mixed all
//    k-ranges, and the weight gradients streamed their operands from beyond L2.)
//  * ksplit < 0: split = b % splits pins each k-range to its own XCD(s) (sweeps only).
struct TileSlot {
  int bid, split, splits;
};
__device__ __forceinline__ TileSlot tile_slot(const GemmArgs& p, int ntiles) {
  TileSlot t;
  if (p.ksplit < -1) {
    t.splits = -p.ksplit;
    t.split = blockIdx.x % t.splits;
    t.bid = blockIdx.x / t.splits;
    return t;
  }
  t.splits = p.ksplit > 1 ? p.ksplit : 1;
  const int nwg = ntiles * t.splits;
  const int b = blockIdx.x, xcd = b & 7, q = nwg >> 3, r = nwg & 7;
  const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
  t.split = w / ntiles;
  t.bid = w - t.split * ntiles;
  return t;
}

// Split-K partial sums: the f32 tile rows staged in LDS (32 x 64 per wave, columns XOR-swizzled
// by ((row >> 2) & 3) << 4) are added with one float atomic per lane, lanes along the row, so
// every wave-instruction covers 256 contiguous bytes -- the full memory-side atomic rate.  (A
// lane-owns-4-columns pattern touches each 64-B segment four times and ran ~4x slower.)
__device__ __forceinline__ void split_rows_atomic(const float* ct, float* C, long long ldc, int mbase,
                                                  int ncol0, int M, int N, int lane) {
  const int n = ncol0 + lane;
  if (n >= N) return;
  const int rows = min(32, M - mbase);
  float* c = C + (long long)mbase * ldc + n;
#pragma unroll 8
  for (int row = 0; row < rows; ++row)
    atomicAdd(c + (long long)row * ldc, ct[row * 64 + (lane ^ (((row >> 2) & 3) << 4))]);
}

// Bias-gradient column sums of a wave's 64 columns [nb, nb + 64): lane l & 15 holds columns
// nb + 4 (l & 15) + e in cs[e], summed over its row group l >> 4.  Reduce over the four row
// groups, then hand column nb + l to lane l so ONE atomic instruction covers 256 contiguous
// bytes (four lane-owns-4-columns instructions hit every 64-B segment four times; with every
// M-tile adding to the same N columns the serialised atomics cost ~20 % of a dgrad GEMM).
__device__ __forceinline__ void colsum_flush(float (&cs)[4], float* colsum, int nb, int N, int lane) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    cs[e] += __shfl_xor(cs[e], 16, 64);
    cs[e] += __shfl_xor(cs[e], 32, 64);
  }
  const int src = lane >> 2, e = lane & 3;
  const float v0 = __shfl(cs[0], src, 64), v1 = __shfl(cs[1], src, 64);
  const float v2 = __shfl(cs[2], src, 64), v3 = __shfl(cs[3], src, 64);
  const float v = e == 0 ? v0 : (e == 1 ? v1 : (e == 2 ? v2 : v3));
  if (nb + lane < N) atomicAdd(colsum + nb + lane, v);
}

// ---- Shared epilogue of the LDS-DMA kernels (v2, v3).  A wave owns FM x 4 fragments of
// 16x16 (FM/2 passes of 32 rows x 64 columns).  Each pass stages its f32 rows through LDS
// ([32][64] per wave, columns XOR-swizzled by ((row >> 2) & 3) << 4) so that bias /
// residual / aux / C move 16 B (f32) or 8 B (bf16) per lane along rows.  Every global READ
// of a pass (aux_in for act', the f32 residual or the accumulated C) is issued as one batch
// one pass AHEAD, into a double buffer: one HBM round trip per pass overlapped with the
// previous pass, instead of one exposed round trip per 4 rows (the v12 epilogue waited on
// each row group's aux load before issuing the next: act' dgrad ran at ~65 % of the plain
// product's rate).  DB = false (kernels that need their registers: several workgroups per CU,
// or 128-row wave tiles) issues a pass's reads right after staging it instead, overlapping
// only the barrier and LDS re-read.
struct EpiIn {
  // per row group t: the f32 residual (or accumulated C) when there is one, else the act'
  // operand (bf16 x 4 in .x/.y) -- one 16-B slot, so the prefetch costs 32 VGPRs not 48
  // (no caller combines act' with a residual; if one did, its aux is read late)
  uint4 v[8];
};

__device__ __forceinline__ const float* epi_fsrc(const GemmArgs& p) {
  return p.residual ? p.residual : (p.out_f32 && p.accumulate ? static_cast<const float*>(p.C) : nullptr);
}

__device__ __forceinline__ void epi_load(const GemmArgs& p, EpiIn& e, int mb, int n, bool nok, int lane) {
  const bf16_t* aux_in = static_cast<const bf16_t*>(p.aux_in);
  const float* fsrc = epi_fsrc(p);
  const long long ldf = p.residual ? p.ldr : p.ldc;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int m = mb + (lane >> 4) + 4 * t;
    const bool ok = nok && m < p.M;
    e.v[t] = make_uint4(0u, 0u, 0u, 0u);
    if (ok && fsrc) {
      e.v[t] = *reinterpret_cast<const uint4*>(fsrc + (long long)m * ldf + n);
    } else if (ok && p.act_bwd) {
      const uint2 z = *reinterpret_cast<const uint2*>(aux_in + (long long)m * p.ld_aux_in + n);
      e.v[t].x = z.x;
      e.v[t].y = z.y;
    }
  }
}

template <int FM, bool DB>
__device__ __forceinline__ void epi_tile(const GemmArgs& p, floatx4 (&acc)[FM][4], float* ct, int splits,
                                         int mw, int nw, int lane) {
  constexpr int NP = FM / 2;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  float alpha = p.alpha;
  if (p.alpha_ptr) alpha *= *p.alpha_ptr;
  const int c4 = lane & 15;
  const int n = nw + c4 * 4;
  const bool nok = n < p.N;  // N % 4 == 0 is required by the host for v2+
  float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p.bias && nok) bias4 = *reinterpret_cast<const float4*>(p.bias + n);
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  bf16_t* aux_out = static_cast<bf16_t*>(p.aux_out);
  const float* fsrc = epi_fsrc(p);
  EpiIn e[DB ? 2 : 1];
  if (DB && splits <= 1) epi_load(p, e[0], mw, n, nok, lane);
#pragma unroll
  for (int h = 0; h < NP; ++h) {
    __syncthreads();  // the ring (h = 0) / previous pass (h > 0) fully consumed
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = ii * 16 + (lane >> 4) * 4 + r;
          const int col = (j * 16 + (lane & 15)) ^ (((row >> 2) & 3) << 4);
          ct[row * 64 + col] = acc[2 * h + ii][j][r] * alpha;
        }
    // (after the staging writes, so this pass's accumulators are dead before the loads land)
    if (!DB && splits <= 1) epi_load(p, e[0], mw + h * 32, n, nok, lane);
    __syncthreads();
    if (splits > 1) {  // f32 partial sums: atomics (no epilogue operands)
      split_rows_atomic(ct, static_cast<float*>(p.C), p.ldc, mw + h * 32, nw, p.M, p.N, lane);
      continue;
    }
    if (DB && h + 1 < NP) epi_load(p, e[(h + 1) & 1], mw + (h + 1) * 32, n, nok, lane);
    const EpiIn& cur = e[DB ? (h & 1) : 0];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int row = (lane >> 4) + 4 * t;
      const int m = mw + h * 32 + row;
      const int col = (c4 * 4) ^ (((row >> 2) & 3) << 4);
      const float4 v4 = *reinterpret_cast<const float4*>(ct + row * 64 + col);
      if (m >= p.M || !nok) continue;
      float v[4] = {v4.x + bias4.x, v4.y + bias4.y, v4.z + bias4.z, v4.w + bias4.w};
      if (p.act_bwd) {
        const uint2 z = fsrc ? *reinterpret_cast<const uint2*>(static_cast<const bf16_t*>(p.aux_in) +
                                                              (long long)m * p.ld_aux_in + n)
                             : make_uint2(cur.v[t].x, cur.v[t].y);
        v[0] *= act_grad(__uint_as_float(z.x << 16), p.act_bwd);
        v[1] *= act_grad(__uint_as_float(z.x & 0xffff0000u), p.act_bwd);
        v[2] *= act_grad(__uint_as_float(z.y << 16), p.act_bwd);
        v[3] *= act_grad(__uint_as_float(z.y & 0xffff0000u), p.act_bwd);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) cs[q] += v[q];
      if (aux_out) {  // the pre-activation, or act'(v) (aux_deriv)
        uint2 w;
        if (p.aux_deriv) {
          w.x = pack2bf(act_grad(v[0], p.act), act_grad(v[1], p.act));
          w.y = pack2bf(act_grad(v[2], p.act), act_grad(v[3], p.act));
        } else {
          w.x = pack2bf(v[0], v[1]);
          w.y = pack2bf(v[2], v[3]);
        }
        st8(aux_out + (long long)m * p.ld_aux_out + n, w, p.nt_store & 1);
      }
      if (p.act == ACT_GELU) {  // packed-f32 math (common.h:gelu_tanh2)
        const dpc_f2_t g01 = gelu_tanh2(dpc_f2_t{v[0], v[1]}), g23 = gelu_tanh2(dpc_f2_t{v[2], v[3]});
        v[0] = g01.x; v[1] = g01.y; v[2] = g23.x; v[3] = g23.y;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = act_fwd(v[q], p.act);
      }
      const long long ci = (long long)m * p.ldc + n;
      if (fsrc) {
        v[0] += __uint_as_float(cur.v[t].x); v[1] += __uint_as_float(cur.v[t].y);
        v[2] += __uint_as_float(cur.v[t].z); v[3] += __uint_as_float(cur.v[t].w);
      }
      if (p.out_f32) {
        float4* C = reinterpret_cast<float4*>(static_cast<float*>(p.C) + ci);
        if (p.accumulate && p.residual) {  // (no caller does both; C read late)
          const float4 o = *C;
          v[0] += o.x; v[1] += o.y; v[2] += o.z; v[3] += o.w;
        }
        st16(C, make_float4(v[0], v[1], v[2], v[3]), p.nt_store & 2);
      } else {
        uint2 w;
        w.x = pack2bf(v[0], v[1]);
        w.y = pack2bf(v[2], v[3]);
        st8(static_cast<bf16_t*>(p.C) + ci, w, p.nt_store & 1);
      }
    }
  }
  if (p.colsum) colsum_flush(cs, p.colsum, nw, p.N, lane);
}



// Load this thread's 4 x 16 B of a 128x64 (k-major) or 64x128 (mn-major) tile.
template <bool KMAJ>
__device__ __forceinline__ void g_load(uint4 (&r)[4], const bf16_t* __restrict__ P, long long ld,
                                       int mn0, int k0, int MN, int K) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = t + i * NT;
    int row, col, rlim, clim;
    if (KMAJ) { row = c >> 3; col = (c & 7) * 8; rlim = MN - mn0; clim = K - k0; }
    else      { row = c >> 4; col = (c & 15) * 8; rlim = K - k0; clim = MN - mn0; }
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row < rlim && col < clim) {
      const bf16_t* src = KMAJ ? P + (long long)(mn0 + row) * ld + (k0 + col)
                               : P + (long long)(k0 + row) * ld + (mn0 + col);
      v = *reinterpret_cast<const uint4*>(src);
      // the operand's extent ends inside this chunk (k-major: K % 8 != 0; mn-major: an operand
      // stored with fewer columns than the product has rows): zero the rest
      if (clim - col < 8) {
        const int keep = clim - col;
        unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e >= keep) w[e >> 1] &= (e & 1) ? 0x0000ffffu : 0xffff0000u;
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    r[i] = v;
  }
}

template <bool KMAJ>
__device__ __forceinline__ void s_store(const uint4 (&r)[4], bf16_t* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = t + i * NT;
    int off;
    if (KMAJ) off = kmaj_off(c >> 3, c & 7);
    else      off = mnmaj_off(c >> 4, (c & 15) * 8);
    *reinterpret_cast<uint4*>(lds + off) = r[i];
  }
}

template <bool AK, bool BK>
__global__ __launch_bounds__(NT, 2) void gemm_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) bf16_t smem[4 * TILE_ELEMS];  // [stage][A|B]
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  const int nwg = tiles_m * tiles_n;
  const TileSlot ts = tile_slot(p, nwg);
  const int bid = ts.bid;
  // grouped ordering for L2 reuse
  const int group = GROUP_M * tiles_n;
  const int gid = bid / group, first_m = gid * GROUP_M;
  const int gsz = min(tiles_m - first_m, GROUP_M);
  const int tm = first_m + (bid % group) % gsz;
  const int tn = (bid % group) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const bf16_t* A = static_cast<const bf16_t*>(p.A);
  const bf16_t* B = static_cast<const bf16_t*>(p.B);

  floatx4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int nk = (p.K + BKT - 1) / BKT;
  uint4 ra[4], rb[4];
  const int a_mn = AK ? p.a_r : p.a_c, a_k = AK ? min(p.K, p.a_c) : min(p.K, p.a_r);
  const int b_mn = BK ? p.b_r : p.b_c, b_k = BK ? min(p.K, p.b_c) : min(p.K, p.b_r);
  g_load<AK>(ra, A, p.lda, m0, 0, a_mn, a_k);
  g_load<BK>(rb, B, p.ldb, n0, 0, b_mn, b_k);
  s_store<AK>(ra, smem);
  s_store<BK>(rb, smem + TILE_ELEMS);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) {
      g_load<AK>(ra, A, p.lda, m0, (kt + 1) * BKT, a_mn, a_k);
      g_load<BK>(rb, B, p.ldb, n0, (kt + 1) * BKT, b_mn, b_k);
    }
    const bf16_t* la = smem + cur * 2 * TILE_ELEMS;
    const bf16_t* lb = la + TILE_ELEMS;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = frag<AK>(la, wr * 64 + i * 16, ks, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = frag<BK>(lb, wc * 64 + j * 16, ks, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      bf16_t* nxt = smem + (cur ^ 1) * 2 * TILE_ELEMS;
      s_store<AK>(ra, nxt);
      s_store<BK>(rb, nxt + TILE_ELEMS);
    }
    __syncthreads();
  }

  // ---- epilogue: C/D map of 16x16x32: col = lane & 15, row = 4 (lane >> 4) + r ----
  float alpha = p.alpha;
  if (p.alpha_ptr) alpha *= *p.alpha_ptr;
  const bf16_t* aux_in = static_cast<const bf16_t*>(p.aux_in);
  bf16_t* aux_out = static_cast<bf16_t*>(p.aux_out);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wc * 64 + j * 16 + (lane & 15);
    const bool nok = n < p.N;
    const float bn = (p.bias && nok) ? p.bias[n] : 0.f;
    float csum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wr * 64 + i * 16 + (lane >> 4) * 4 + r;
        if (m >= p.M || !nok) continue;
        float v = acc[i][j][r] * alpha + bn;
        if (p.act_bwd) v *= act_grad(bf2f(aux_in[(long long)m * p.ld_aux_in + n]), p.act_bwd);
        csum += v;
        if (aux_out) aux_out[(long long)m * p.ld_aux_out + n] = f2bf(p.aux_deriv ? act_grad(v, p.act) : v);
        v = act_fwd(v, p.act);
        if (p.residual) v += p.residual[(long long)m * p.ldr + n];
        const long long ci = (long long)m * p.ldc + n;
        if (p.out_f32) {
          float* C = static_cast<float*>(p.C);
          if (p.accumulate) v += C[ci];
          C[ci] = v;
        } else {
          static_cast<bf16_t*>(p.C)[ci] = f2bf(v);
        }
      }
    }
    if (p.colsum) {  // reduce over the 4 row-groups of lanes sharing this column
      csum += __shfl_xor(csum, 16, 64);
      csum += __shfl_xor(csum, 32, 64);
      if ((lane >> 4) == 0 && nok) atomicAdd(p.colsum + n, csum);
    }
  }
}

// =====================================================================================
// v2: LDS-DMA pipeline.  Operand tiles stream HBM/L2 -> LDS with buffer_load_dwordx4 ... lds
// (no VGPR round trip, no ds_write), STAGES-deep ring with ONE raw s_barrier per k-tile and a
// counted vmcnt that keeps STAGES-2 tiles in flight across it.  The buffer descriptor's
// num_records bounds every operand, so out-of-range rows / k-rows land in LDS as zeros (the
// M/N/K edges need no predicates).  Because the DMA writes LDS lane-linearly (1 KiB per
// wave-instruction), the bank swizzle is applied to the per-lane SOURCE address and read back
// with the same involution.  Epilogue: the f32 tile goes through LDS so that bias / residual /
// aux / C traffic is 16-B-per-lane row-contiguous.
// =====================================================================================



// buffer descriptor whose base is `off` bytes into the operand and whose range ends with it
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned long long total,
                                                            unsigned long long off) {
  const unsigned long long left = off < total ? total - off : 0ull;
  const unsigned nrec = left > 0xffffffffull ? 0xffffffffu : (unsigned)left;
  return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)base + off), 0, nrec, 0x00020000);
}

template <int NL>
__device__ __forceinline__ void issue_tile(const void* base, unsigned long long total, unsigned long long off,
                                           const int* voff, bf16_t* lds_tile, int wave) {
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, total, off);
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int j = wave * NL + i;  // wave-instruction index: 1 KiB of the tile
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t)(lds_tile + j * 512), 16, voff[i], 0, 0, 0);
  }
}


template <int KB, int STAGES>
struct V2Cfg {
  static constexpr int TILE = BM * KB;                  // bf16 elements per operand per stage
  static constexpr int PIPE = STAGES * 2 * TILE;        // pipeline ring (elements)
  static constexpr int EPI = 4 * 32 * 64 * 2;           // epilogue: 4 waves x [32][64] f32 (as bf16 units)
  static constexpr int SMEM = PIPE > EPI ? PIPE : EPI;
  static constexpr int WGS = (160 * 1024) / (SMEM * 2) > 4 ? 4 : (160 * 1024) / (SMEM * 2);
};

template <int KB, int STAGES, bool AK, bool BK>
__global__ __launch_bounds__(NT, (V2Cfg<KB, STAGES>::WGS)) void gemm2_kernel(GemmArgs p, unsigned long long a_bytes,
                                                                          unsigned long long b_bytes) {
  using Cfg = V2Cfg<KB, STAGES>;
  constexpr int NL = KB / 16;
  __shared__ __attribute__((aligned(16))) bf16_t smem[Cfg::SMEM];
  const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
  const int nwg = tiles_m * tiles_n;
  const TileSlot ts = tile_slot(p, nwg);
  const int bid = ts.bid;
  const int group = GROUP_M * tiles_n;
  const int gid = bid / group, first_m = gid * GROUP_M;
  const int gsz = min(tiles_m - first_m, GROUP_M);
  const int tm = first_m + (bid % group) % gsz;
  const int tn = (bid % group) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wid >> 1, wc = wid & 1;

  // Per-lane source byte offsets relative to the tile origin of the current k-tile.  The
  // descriptor base itself moves (64-bit scalar math) with the tile origin and k, so the
  // 32-bit voffsets stay small for operands of any size, and num_records = bytes left in the
  // operand makes every out-of-range lane read zeros.
  int va[NL], vb[NL];
  dma_offsets<KB, AK>(va, p.lda, wid, lane);
  dma_offsets<KB, BK>(vb, p.ldb, wid, lane);
  const unsigned long long a_org = AK ? (unsigned long long)m0 * p.lda * 2 : (unsigned long long)m0 * 2;
  const unsigned long long b_org = BK ? (unsigned long long)n0 * p.ldb * 2 : (unsigned long long)n0 * 2;
  const unsigned long long a_step = AK ? KB * 2ull : (unsigned long long)KB * p.lda * 2;
  const unsigned long long b_step = BK ? KB * 2ull : (unsigned long long)KB * p.ldb * 2;
  floatx4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  // split-K: each split owns a contiguous run of k-tiles (the host only splits plain
  // f32-accumulating products, whose partial tiles are combined with f32 atomics)
  const int nk_all = (p.K + KB - 1) / KB;
  const int splits = ts.splits;
  const int per = (nk_all + splits - 1) / splits;
  const int kt0 = ts.split * per;
  const int nk = max(0, min(nk_all, kt0 + per) - kt0);
#define DPC_ISSUE(it_)                                                                              \
  do {                                                                                              \
    bf16_t* base_ = smem + ((it_) % STAGES) * 2 * Cfg::TILE;                                        \
    const unsigned long long ktg_ = (unsigned long long)(kt0 + (it_));                              \
    issue_tile<NL>(p.A, a_bytes, a_org + a_step * ktg_, va, base_, wid);                            \
    issue_tile<NL>(p.B, b_bytes, b_org + b_step * ktg_, vb, base_ + Cfg::TILE, wid);                \
  } while (0)
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nk) DPC_ISSUE(s);

  for (int kt = 0; kt < nk; ++kt) {
    // tile kt landed for THIS wave: the tiles issued after it (at most STAGES-2, fewer at the
    // tail) may stay in flight -- 2*NL loads each
    const int after = min(STAGES - 2, nk - 1 - kt);
    if (STAGES >= 4 && after >= 2) wait_vm<(STAGES >= 4 ? 4 * NL : 0)>();
    else if (STAGES >= 3 && after >= 1) wait_vm<(STAGES >= 3 ? 2 * NL : 0)>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();  // ... and for every wave; also: all waves finished tile kt-1
    asm volatile("" ::: "memory");
    if (kt + STAGES - 1 < nk) DPC_ISSUE(kt + STAGES - 1);
    const bf16_t* la = smem + (kt % STAGES) * 2 * Cfg::TILE;
    const bf16_t* lb = la + Cfg::TILE;
#pragma unroll
    for (int ks = 0; ks < KB / 32; ++ks) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = frag_k<KB, AK>(la, wr * 64 + i * 16, ks, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = frag_k<KB, BK>(lb, wc * 64 + j * 16, ks, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }

  // ---------------- epilogue through LDS, two passes of 32 rows per wave: the f32 tile is
  // re-read row-contiguously so bias / residual / aux / C move 16 B per lane
  epi_tile<4, (Cfg::WGS <= 2)>(p, acc, reinterpret_cast<float*>(smem) + wid * 32 * 64, splits, m0 + wr * 64, n0 + wc * 64, lane);
}

// =====================================================================================
// v3: large tiles.  A 128x128 tile re-reads each operand byte from L2 once per 128 output
// columns: at the MFMA rate that is ~39 TB/s of L2->LDS traffic chip-wide, the whole L2
// bandwidth, so v2 is L2-bound (PMC: WAIT_ANY 44 %).  v3 keeps v2's LDS-DMA pipeline,
// swizzles and epilogue but runs 8 waves on a 256x256 (or 256x128) tile: half (3/4) the
// L2 bytes per FLOP, and each wave owns a 128x64 (64x64) sub-tile, so per k-step a wave
// reads 12 (8) fragments for 32 (16) MFMAs.  mn-major operand tiles wider than 128 are
// stored as 128-column halves so the v2 transposed-read swizzle applies unchanged.
template <int BM_, int BN_, int WM, int WN, int KB, int STAGES>
struct V3Cfg {
  static constexpr int NW = WM * WN, NTH = 64 * NW;
  static constexpr int WTM = BM_ / WM, WTN = BN_ / WN;
  static constexpr int FM = WTM / 16, FN = WTN / 16;
  static constexpr int TA = BM_ * KB, TB = BN_ * KB;        // bf16 elements per stage
  static constexpr int NLA = TA / 512 / NW, NLB = TB / 512 / NW;  // 1-KiB DMA instr per wave
  static constexpr int PIPE = STAGES * (TA + TB);
  static constexpr int EPI = NW * 32 * WTN * 2;              // [32][WTN] f32 per wave
  static constexpr int SMEM = PIPE > EPI ? PIPE : EPI;
  static constexpr int WGS = (160 * 1024) / (SMEM * 2) >= 2 ? 2 : 1;
  static_assert(WTN == 64 && (WTM == 64 || WTM == 128), "wave tile 64x64 or 128x64");
  static_assert(NLA * 512 * NW == TA && NLB * 512 * NW == TB, "DMA split");
  static_assert(SMEM * 2 <= 160 * 1024, "LDS");
};



template <int BM_, int BN_, int WM, int WN, int KB, int STAGES, bool AK, bool BK>
__global__ __launch_bounds__((V3Cfg<BM_, BN_, WM, WN, KB, STAGES>::NTH), (V3Cfg<BM_, BN_, WM, WN, KB, STAGES>::WGS)) void gemm3_kernel(
    GemmArgs p, unsigned long long a_bytes, unsigned long long b_bytes) {
  using Cfg = V3Cfg<BM_, BN_, WM, WN, KB, STAGES>;
  constexpr int FM = Cfg::FM, FN = Cfg::FN, NLA = Cfg::NLA, NLB = Cfg::NLB;
  __shared__ __attribute__((aligned(16))) bf16_t smem[Cfg::SMEM];
  const int tiles_m = (p.M + BM_ - 1) / BM_, tiles_n = (p.N + BN_ - 1) / BN_;
  const int nwg = tiles_m * tiles_n;
  const TileSlot ts = tile_slot(p, nwg);
  const int bid = ts.bid;
  const int group = GROUP_M * tiles_n;
  const int gid = bid / group, first_m = gid * GROUP_M;
  const int gsz = min(tiles_m - first_m, GROUP_M);
  const int tm = first_m + (bid % group) % gsz;
  const int tn = (bid % group) / gsz;
  const int m0 = tm * BM_, n0 = tn * BN_;

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wid / WN, wc = wid % WN;

  int va[NLA], vb[NLB];
  dma_offsets3<KB, AK, NLA>(va, p.lda, wid, lane);
  dma_offsets3<KB, BK, NLB>(vb, p.ldb, wid, lane);
  const unsigned long long a_org = AK ? (unsigned long long)m0 * p.lda * 2 : (unsigned long long)m0 * 2;
  const unsigned long long b_org = BK ? (unsigned long long)n0 * p.ldb * 2 : (unsigned long long)n0 * 2;
  const unsigned long long a_step = AK ? KB * 2ull : (unsigned long long)KB * p.lda * 2;
  const unsigned long long b_step = BK ? KB * 2ull : (unsigned long long)KB * p.ldb * 2;
  floatx4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int nk_all = (p.K + KB - 1) / KB;
  const int splits = ts.splits;
  const int per = (nk_all + splits - 1) / splits;
  const int kt0 = ts.split * per;
  const int nk = max(0, min(nk_all, kt0 + per) - kt0);
#define DPC_ISSUE3(it_)                                                                             \
  do {                                                                                              \
    bf16_t* base_ = smem + ((it_) % STAGES) * (Cfg::TA + Cfg::TB);                                  \
    const unsigned long long ktg_ = (unsigned long long)(kt0 + (it_));                              \
    issue_tile<NLA>(p.A, a_bytes, a_org + a_step * ktg_, va, base_, wid);                           \
    issue_tile<NLB>(p.B, b_bytes, b_org + b_step * ktg_, vb, base_ + Cfg::TA, wid);                 \
  } while (0)
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nk) DPC_ISSUE3(s);

  constexpr int PER_TILE = NLA + NLB;  // DMA instructions per wave per k-tile
  for (int kt = 0; kt < nk; ++kt) {
    const int after = min(STAGES - 2, nk - 1 - kt);
    if (STAGES >= 4 && after >= 2) wait_vm<(STAGES >= 4 ? 2 * PER_TILE : 0)>();
    else if (STAGES >= 3 && after >= 1) wait_vm<(STAGES >= 3 ? PER_TILE : 0)>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kt + STAGES - 1 < nk) DPC_ISSUE3(kt + STAGES - 1);
    const bf16_t* la = smem + (kt % STAGES) * (Cfg::TA + Cfg::TB);
    const bf16_t* lb = la + Cfg::TA;
#pragma unroll
    for (int ks = 0; ks < KB / 32; ++ks) {
      bf16x8 fa[FM], fb[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) fb[j] = frag3<KB, BK>(lb, wc * Cfg::WTN + j * 16, ks, lane);
#pragma unroll
      for (int i = 0; i < FM; ++i) fa[i] = frag3<KB, AK>(la, wr * Cfg::WTM + i * 16, ks, lane);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }
#undef DPC_ISSUE3

  // ---------------- epilogue (as v2): WTM/32 passes of 32 rows per wave through LDS
  epi_tile<FM, (FM == 4 && Cfg::WGS == 1)>(p, acc, reinterpret_cast<float*>(smem) + wid * 32 * 64, splits, m0 + wr * Cfg::WTM, n0 + wc * 64, lane);
}

// ---- the reduction passes behind the persistent kernels (gemm_run launches them)
// colsum[n] += sum over the R rows of ws [R][N] (g7_epilogue_act_lds's per-tile partial column
// sums): 4 columns per thread, 16 rows per workgroup row (grid.y), one atomic per column per 16
// rows
static __global__ __launch_bounds__(256) void g7_colsum_reduce(float* colsum, const float* ws, int R, int N) {
  const int c4 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (c4 >= N) return;
  const int r0 = blockIdx.y * 16, r1 = min(R, r0 + 16);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 16
  for (int r = r0; r < r1; ++r) {
    const float4 v = *reinterpret_cast<const float4*>(ws + (long long)r * N + c4);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  atomicAdd(colsum + c4, s.x);
  atomicAdd(colsum + c4 + 1, s.y);
  atomicAdd(colsum + c4 + 2, s.z);
  atomicAdd(colsum + c4 + 3, s.w);
}

// C (=, or += when accumulating) the sum of the s workspace slabs [s][M][N]; 4 columns per
// thread (N % 8 == 0, ldc % 8 == 0: 16-B rows)
static __global__ __launch_bounds__(256) void g7_splitk_reduce(float* C, long long ldc, const float* ws, int M, int N,
                                                       int s, int accumulate, int nt = 0) {
  const long long nq = (long long)M * (N >> 2);
  const long long slab = (long long)M * N;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nq; i += (long long)gridDim.x * 256) {
    const long long m = i / (N >> 2), n = (i - m * (N >> 2)) << 2;
    const float* w = ws + m * N + n;
    float4 v = *reinterpret_cast<const float4*>(w);
    // four slabs' loads in flight before their adds (the one-at-a-time loop waited for each:
    // 2.9 TB/s), the adds in the same order as before (bitwise the same sums)
    int k = 1;
    for (; k + 3 < s; k += 4) {
      const float4 u0 = *reinterpret_cast<const float4*>(w + k * slab);
      const float4 u1 = *reinterpret_cast<const float4*>(w + (k + 1) * slab);
      const float4 u2 = *reinterpret_cast<const float4*>(w + (k + 2) * slab);
      const float4 u3 = *reinterpret_cast<const float4*>(w + (k + 3) * slab);
      v.x += u0.x; v.y += u0.y; v.z += u0.z; v.w += u0.w;
      v.x += u1.x; v.y += u1.y; v.z += u1.z; v.w += u1.w;
      v.x += u2.x; v.y += u2.y; v.z += u2.z; v.w += u2.w;
      v.x += u3.x; v.y += u3.y; v.z += u3.z; v.w += u3.w;
    }
    for (; k < s; ++k) {
      const float4 u = *reinterpret_cast<const float4*>(w + k * slab);
      v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    float4* c = reinterpret_cast<float4*>(C + m * ldc + n);
    if (accumulate) {
      const float4 o = *c;
      v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    st16(c, v, nt);
  }
}

// (v5, the 256x256 eight-wave ping-pong kernel, was removed in round 5: no tuned-table entry and
// no policy branch chose it once v7 took the weight gradients)

}  // namespace dpc

using namespace dpc;

// ---- the dispatcher.  gemm_plan.h decides (which implementation, kernel instantiation, grid,
// split-K plan, reduction passes: a pure function, pinned on the CPU by
// tests/test_gemm_plan_cpu.py); gemm_run below launches what a plan says and decides nothing.
//
// The persistent family's design and synchronisation notes: the top of gemm7_kern.h (v7 / v8 /
// v7d) and of gemm9_kern.h (v9).
static_assert(GP_ACT_GELU == ACT_GELU && GP_ACT_MUL == ACT_MUL && GP_G7_KB == G7_KB && G_SP_DEFAULT == 3,
              "gemm_plan.h's copies of the kernels' constants");

static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// The process-wide settings: the environment is read here, once; the setters below write to it.
static GemmSettings& settings() {
  static GemmSettings g = [] {
    GemmSettings s;
    if (const char* e = getenv("DPC_GEMM_POLICY")) {
      const char* names[5] = {"fs", "fl", "ds", "dl", "w"};
      for (int c = 0; c < 5; ++c) {
        char key[8];
        snprintf(key, sizeof key, "%s=", names[c]);
        for (const char* q = e; (q = strstr(q, key)) != nullptr; ++q)
          if (q == e || q[-1] == ',') { s.policy[c] = atoi(q + strlen(key)); break; }
      }
    }
    s.nt_store = env_int("DPC_GEMM_NT", s.nt_store);
    s.act_lds_env = env_int("DPC_G7_ACTLDS", 1);
    s.res_lds_env = env_int("DPC_G7_RESLDS", 1);
    s.cus = 0;  // asked of the device by the first product (settings_for_launch)
    return s;
  }();
  return g;
}

static const GemmSettings& settings_for_launch() {
  GemmSettings& s = settings();
  if (s.cus <= 0) {
    int dev = 0, n = 0;
    const bool ok = hipGetDevice(&dev) == hipSuccess &&
                    hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0;
    s.cus = ok ? n : 256;
  }
  return s;
}

DPC_API void dpc_gemm_set_impl(int impl) { settings().impl = impl; }
DPC_API void dpc_gemm_set_xcd_split(int on) { settings().xcd_split = on; }
DPC_API void dpc_gemm_set_splits(int s) { settings().force_splits = s; }
DPC_API void dpc_gemm7_set_act_lds(int v) { settings().act_lds = v; }  // -1: DPC_G7_ACTLDS; 0 / 1 forced
DPC_API void dpc_gemm7_set_res_lds(int v) { settings().res_lds = v; }  // -1: DPC_G7_RESLDS; 0 / 1 forced
DPC_API void dpc_set_cu_reserve(int r) { settings().cu_reserve = r < 0 ? 0 : r; }
DPC_API int dpc_get_cu_reserve() { return settings().cu_reserve; }

// GemmPlan::last_kernel of the last product launched (tests assert that a forced implementation
// really ran instead of falling back)
static int g_last_kernel = 0;
DPC_API int dpc_gemm_last_kernel() { return g_last_kernel; }

// kernel identity of a plan -> its instantiation; nullptr: not compiled in any part
typedef void(*G7KernelFn) G7_SIG;
static G7KernelFn g7_kernel_fn(const GemmKernelId& k) {
  switch (gemm_kernel_key(k)) {
#define G7_INST(F, K, ...) case gemm_kernel_key({F, {__VA_ARGS__}}): return K<__VA_ARGS__>;
#include "gemm7_extern.inc"
#undef G7_INST
    default: return nullptr;
  }
}

// K<..., AK, BK> for a runtime layout
#define DPC_BY_LAYOUT(ak, bk, K, ...)                                                            \
  ((ak) ? ((bk) ? K<__VA_ARGS__ true, true> : K<__VA_ARGS__ true, false>)                        \
        : ((bk) ? K<__VA_ARGS__ false, true> : K<__VA_ARGS__ false, false>))

// Launches the steps of a plan; the one place that maps a kernel identity to its instantiation
// (the persistent families: g7_kernel_fn, from the generated list gemm7_extern.inc).
static int gemm_run(const GemmPlan& p, const GemmArgs& a, hipStream_t stream) {
  g_last_kernel = p.last_kernel;
  if (p.rc != 0) return p.rc;
  GemmArgs b = a;  // the dispatcher-owned fields
  b.ksplit = p.ksplit;
  b.nt_store = p.nt_store;
  if (p.drop_ws) b.ws = nullptr;
  const GemmKernelId& k = p.kernel;
  const dim3 grid(p.grid), block(p.block);
  for (int i = 0; i < p.nsteps; ++i) {
    switch (p.steps[i]) {
      case GS_CLEAR:
        (void)hipMemset2DAsync(a.C, (size_t)a.ldc * 4, 0, (size_t)a.N * 4, (size_t)a.M, stream);
        break;
      case GS_SPLITK_REDUCE:
        hipLaunchKernelGGL(g7_splitk_reduce, dim3(p.red_x), dim3(256), 0, stream, static_cast<float*>(a.C), a.ldc,
                           static_cast<const float*>(a.ws), a.M, a.N, p.g7.splits, a.accumulate, p.nt_store & 2);
        break;
      case GS_COLSUM_REDUCE:
        hipLaunchKernelGGL(g7_colsum_reduce, dim3(p.red_x, p.red_y), dim3(256), 0, stream, a.colsum,
                           static_cast<const float*>(a.ws), 2 * p.g7.tiles_m, a.N);
        break;
      case GS_KERNEL:
        if (k.family >= GK_V7) {
          const G7KernelFn fn = g7_kernel_fn(k);
          if (!fn) return (int)hipErrorInvalidDeviceFunction;  // not in gemm_parts.txt
          hipLaunchKernelGGL(fn, grid, block, 0, stream, b, p.a_bytes, p.b_bytes, p.g7);
        } else if (k.family == GK_V1) {
          hipLaunchKernelGGL(DPC_BY_LAYOUT(k.t[0], k.t[1], gemm_kernel, ), grid, block, 0, stream, b);
        } else {
          void (*fn)(GemmArgs, unsigned long long, unsigned long long) = nullptr;
          if (k.family == GK_V2 && k.t[0] == 64 && k.t[1] == 2) fn = DPC_BY_LAYOUT(k.t[2], k.t[3], gemm2_kernel, 64, 2, );
          else if (k.family == GK_V2 && k.t[0] == 64 && k.t[1] == 3) fn = DPC_BY_LAYOUT(k.t[2], k.t[3], gemm2_kernel, 64, 3, );
          else if (k.family == GK_V2 && k.t[0] == 32 && k.t[1] == 3) fn = DPC_BY_LAYOUT(k.t[2], k.t[3], gemm2_kernel, 32, 3, );
          else if (k.family == GK_V3 && k.t[0] == 256 && k.t[1] == 128 && k.t[4] == 32 && k.t[5] == 3)
            fn = DPC_BY_LAYOUT(k.t[6], k.t[7], gemm3_kernel, 256, 128, 4, 2, 32, 3, );
          if (!fn) return (int)hipErrorInvalidDeviceFunction;
          hipLaunchKernelGGL(fn, grid, block, 0, stream, b, p.a_bytes, p.b_bytes);
        }
        break;
      default: break;
    }
  }
  return (int)hipGetLastError();
}

DPC_API int dpc_gemm(const GemmArgs* a, hipStream_t stream) {
  return gemm_run(gemm_plan(*a, settings_for_launch()), *a, stream);
}

// The plan of a product as one line of text (gemm_plan.h: gemm_plan_text), ending in the
// dpc_gemm_last_kernel() code the launch would leave; launches nothing.  Returns the length.
DPC_API int dpc_gemm_explain(const GemmArgs* a, char* buf, int cap) {
  return gemm_plan_text(gemm_plan(*a, settings_for_launch()), buf, cap);
}
