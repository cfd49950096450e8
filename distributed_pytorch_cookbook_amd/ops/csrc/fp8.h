// OCP e4m3 (torch.float8_e4m3fn) for the 1-byte KV cache: the gfx950 converts, four elements per
// dword, byte i of a 16-B chunk = element i.
//
// Quantise: byte = fp8_rne(clamp(float(x_bf16) * inv_scale, -448, 448)), inv_scale = float32(1 / scale)
// formed once on the host.  The clamp is a v_med3_f32 ahead of the convert: e4m3fn has no infinity,
// an overflowing convert would store NaN (0x7F), and a NaN in the cache poisons every later step.
// Dequantise: v_cvt_pk_f32_fp8 (exact); the scale is not applied here -- the kernels fold k_scale
// into the score scale and v_scale into the accumulator on its way out.
#pragma once
#include "common.h"

namespace dpc {

typedef unsigned char fp8_t;  // raw e4m3 payload

struct KvScales {             // per cache: x = byte * scale, byte = fp8(x * inv)
  float k_scale, k_inv, v_scale, v_inv;
};

__device__ __forceinline__ float fp8_clamp(float x) { return __builtin_amdgcn_fmed3f(x, -448.f, 448.f); }

// four floats (already scaled) -> one dword of 4 x e4m3
__device__ __forceinline__ unsigned fp8_pack4(float a, float b, float c, float d) {
  int r = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_clamp(a), fp8_clamp(b), 0, false);
  r = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_clamp(c), fp8_clamp(d), r, true);
  return (unsigned)r;
}

// 16 bf16 (two 16-B chunks) x inv -> 16 e4m3 (one 16-B chunk)
__device__ __forceinline__ uint4 fp8_quant16(const uint4& lo, const uint4& hi, float inv) {
  float f[16];
  unpack8(lo, f);
  unpack8(hi, f + 8);
#pragma unroll
  for (int e = 0; e < 16; ++e) f[e] *= inv;
  uint4 r;
  r.x = fp8_pack4(f[0], f[1], f[2], f[3]);
  r.y = fp8_pack4(f[4], f[5], f[6], f[7]);
  r.z = fp8_pack4(f[8], f[9], f[10], f[11]);
  r.w = fp8_pack4(f[12], f[13], f[14], f[15]);
  return r;
}

// one dword of 4 x e4m3 -> f[0..3]
__device__ __forceinline__ void fp8_unpack4(unsigned w, float* f) {
  const dpc_f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const dpc_f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo.x;
  f[1] = lo.y;
  f[2] = hi.x;
  f[3] = hi.y;
}

__device__ __forceinline__ void fp8_unpack16(const uint4& v, float* f) {
  fp8_unpack4(v.x, f);
  fp8_unpack4(v.y, f + 4);
  fp8_unpack4(v.z, f + 8);
  fp8_unpack4(v.w, f + 12);
}

// one dword of 4 x e4m3 -> two dwords of 2 x bf16 each (every e4m3 value is a bf16 value: the
// pack is the upper half of the f32)
__device__ __forceinline__ uint2 fp8_to_bf16x4(unsigned w) {
  const dpc_f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const dpc_f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  uint2 r;
  r.x = (__float_as_uint(lo.x) >> 16) | (__float_as_uint(lo.y) & 0xffff0000u);
  r.y = (__float_as_uint(hi.x) >> 16) | (__float_as_uint(hi.y) & 0xffff0000u);
  return r;
}

}  // namespace dpc
