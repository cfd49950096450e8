// OCP MXFP4 for the 4-bit weights: elements e2m1 (sign, two exponent bits, one mantissa bit: 0, .5,
// 1, 1.5, 2, 3, 4, 6), two per byte -- element 2j in the low nibble of byte j -- and one e8m0 scale
// byte (value 2^(byte - 127)) per block of 32 consecutive k.  ops/gemm.py:mx_quantize_ref is the
// definition of the format; the functions below are its pieces, bit for bit.
//
// Dequantise: v_cvt_scalef32_pk_bf16_fp4 takes one byte of a dword (two e2m1) and an f32 scale and
// returns two bf16 with the scale applied (low nibble in the low half).  Every e2m1 value times a
// power of two within the quantiser's clamp is a normal bf16 value, so the widening is exact.
// Quantise: the block's exponent from the f32 bits of its amax (no log2), the elements by plain
// compares -- round to nearest, ties to the even code, saturating at 6.
#pragma once
#include "common.h"

namespace dpc {

constexpr int MX_BLOCK = 32;  // k per scale byte

// e8m0 byte -> the power of two as f32 (1 <= byte <= 254: a normal float)
__device__ __forceinline__ float mx_scale(unsigned byte) { return __uint_as_float(byte << 23); }

// one dword of 8 x e2m1 (8 consecutive k) x scale -> one bf16x8 MFMA operand
__device__ __forceinline__ bf16x8 mx_widen8(unsigned w, float s) {
  uint4 r;
  r.x = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 0));
  r.y = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 1));
  r.z = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 2));
  r.w = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 3));
  return __builtin_bit_cast(bf16x8, r);
}

// The block exponent e, the smallest integer with 6 * 2^e >= amax, clamped to [-125, 125], from the
// bits of amax >= 0 as f32: amax = m * 2^x with .5 <= m < 1 (frexp) gives x - 3 for m <= .75, else
// x - 2.  A block of zeros takes 0; a denormal amax lands below the clamp either way.
__device__ __forceinline__ int mx_exponent(unsigned amax_bits) {
  if (amax_bits == 0u) return 0;
  const int x = (int)(amax_bits >> 23) - 126;
  const int e = x - ((amax_bits & 0x7fffffu) <= 0x400000u ? 3 : 2);
  return min(max(e, -125), 125);
}

// v = |w| * 2^-e -> the e2m1 magnitude code 0..7: each compare is one step of the grid, the tie
// at its midpoint going to the even code
__device__ __forceinline__ unsigned mx_code(float v) {
  return (unsigned)(v > 0.25f) + (unsigned)(v >= 0.75f) + (unsigned)(v > 1.25f) + (unsigned)(v >= 1.75f) +
         (unsigned)(v > 2.5f) + (unsigned)(v >= 3.5f) + (unsigned)(v > 5.f);
}

}  // namespace dpc
