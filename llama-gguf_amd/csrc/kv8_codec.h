// kv8_codec.h — the byte KV formats' codecs (internal): int8 rows with one f32 scale per row, FP8 E4M3 / E5M2 without scales, as the
// reference's QuantizedKVCache writes and reads them (kv_quantized.rs).  Shared by the decode and prompt kernels of attention.hip and
// the group decode kernel of attention_group_kv8.hip: every kernel that stores a row stores the same bits.
#pragma once

#include "device_utils.h"

namespace lgh {

__device__ __forceinline__ f32x4 unpack_i8x4(uint32_t w, float scale) {
  f32x4 r;
  r.x = (float)(int)(int8_t)(w & 0xFFu) * scale;
  r.y = (float)(int)(int8_t)((w >> 8) & 0xFFu) * scale;
  r.z = (float)(int)(int8_t)((w >> 16) & 0xFFu) * scale;
  r.w = (float)(int)(int8_t)(w >> 24) * scale;
  return r;
}

// quantize_int8: the scale of a row whose largest magnitude is amax, and one value's byte
__device__ __forceinline__ float i8_row_scale(float amax) { return amax > 1e-10f ? amax / 127.0f : 1.0f; }
__device__ __forceinline__ uint32_t i8_quantize(float v, float scale) {
  float r = roundf(v / scale);                           // f32::round: halves away from zero
  r = r < -128.0f ? -128.0f : (r > 127.0f ? 127.0f : r);
  return (uint32_t)(int)r & 0xFFu;
}

// quantizes the f32 row held 4 elements per lane by the LPR lanes of a row group; returns the packed int8 word and the scale
template <int LPR>
__device__ __forceinline__ uint32_t quantize_row_i8(f32x4 x, float& scale) {
  float amax = fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w)));
  amax = fmaxf(amax, dpp_f<0xB1>(amax));
  amax = fmaxf(amax, dpp_f<0x4E>(amax));
  amax = fmaxf(amax, dpp_f<0x141>(amax));
  amax = fmaxf(amax, dpp_f<0x140>(amax));
  if (LPR == 32) amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
  scale = i8_row_scale(amax);
  return i8_quantize(x.x, scale) | i8_quantize(x.y, scale) << 8 | i8_quantize(x.z, scale) << 16 | i8_quantize(x.w, scale) << 24;
}

// ---- the reference's FP8 KV formats (kv_quantized.rs:413-565; FMT 2 = E4M3, 3 = E5M2): one byte per element, no scales ----
// dequantize_fp8_*: case by case it is the standard decode of the format (E4M3 without infinities, 0x7F / 0xFF = NaN), except
// that both zeros read back as +0.  E5M2 is the upper byte of an IEEE half.
template <int FMT>
__device__ __forceinline__ float fp8_decode(uint32_t b) {
  const uint32_t mag = b & 0x7Fu;
  if (mag == 0) return 0.0f;
  if (FMT == 3) return (float)__builtin_bit_cast(_Float16, (uint16_t)(b << 8));
  if (mag == 0x7Fu) return __uint_as_float(0x7FC00000u);
  const uint32_t e = mag >> 3, mt = mag & 7u;
  const float v = e ? __uint_as_float((e + 120u) << 23 | mt << 20) : (float)mt * 0x1p-9f;
  return __uint_as_float(__float_as_uint(v) | (b & 0x80u) << 24);
}
// quantize_fp8_e4m3 / _e5m2 as written in the reference: the mantissa is truncated, magnitudes past the largest exponent
// saturate to 0x7E / 0x7C, and an E4M3 magnitude in [480, 512) becomes the NaN pattern 0x7F
template <int FMT>
__device__ __forceinline__ uint32_t fp8_encode(float value) {
  constexpr bool e4 = FMT == 2;
  const uint32_t bits = __float_as_uint(value);
  const uint32_t sign = (bits >> 31) << 7;
  if (value != value) return 0xFFu;
  if ((bits & 0x7FFFFFFFu) == 0x7F800000u) return e4 ? (sign ? 0xFFu : 0x7Fu) : (sign ? 0xFCu : 0x7Cu);
  if (value == 0.0f) return 0x00u;
  const int exponent = (int)((bits >> 23) & 0xFFu) - 127;
  uint32_t mantissa = bits & 0x7FFFFFu;
  if (exponent != -127) mantissa |= 0x800000u;
  if (e4) {
    const int e = exponent + 7;
    if (e > 15) return sign | 0x7Eu;
    if (e > -3 && e <= 0) return sign | ((mantissa >> (24 - (uint32_t)(3 + e))) & (0x7u >> (uint32_t)(-e)));
    if (e <= -3) return sign;
    return sign | (uint32_t)e << 3 | ((mantissa >> 20) & 0x7u);
  }
  const int e = exponent + 15;
  if (e > 31) return sign | 0x7Cu;
  if (e >= -1 && e <= 0) return sign | ((mantissa >> (24 - (uint32_t)(2 + e))) & (0x3u >> (uint32_t)(-e)));
  if (e < -1) return sign;
  return sign | (uint32_t)e << 2 | ((mantissa >> 21) & 0x3u);
}
// four cached values of one dword, any byte format (FMT 1 = int8 with the row's scale)
template <int FMT>
__device__ __forceinline__ f32x4 unpack_kv4(uint32_t w, float scale) {
  if (FMT == 1) return unpack_i8x4(w, scale);
  f32x4 r;
  r.x = fp8_decode<FMT>(w & 0xFFu); r.y = fp8_decode<FMT>((w >> 8) & 0xFFu);
  r.z = fp8_decode<FMT>((w >> 16) & 0xFFu); r.w = fp8_decode<FMT>(w >> 24);
  return r;
}

// Four cached values of one dword for the matrix-core kernels, which put an int8 row's scale on its score (K) and its probability (V)
// instead of its elements: int8 widened without the scale, FP8 by the hardware's OCP converters (v_cvt_pk_f32_fp8 / _bf8).  They agree
// with fp8_decode on every code except that 0x80 reads as -0, which adds nothing to a dot product either way
// (tests/test_gpu_kv8_prefill.py runs every code through both operands).
template <int FMT>
__device__ __forceinline__ f32x4 kv8_widen4(uint32_t w) {
  f32x4 r;
  if (FMT == 1) {
    r.x = (float)(int)(int8_t)(w & 0xFFu); r.y = (float)(int)(int8_t)((w >> 8) & 0xFFu);
    r.z = (float)(int)(int8_t)((w >> 16) & 0xFFu); r.w = (float)(int)(int8_t)(w >> 24);
  } else if (FMT == 2) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    r.x = lo[0]; r.y = lo[1]; r.z = hi[0]; r.w = hi[1];
  } else {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true);
    r.x = lo[0]; r.y = lo[1]; r.z = hi[0]; r.w = hi[1];
  }
  return r;
}

}  // namespace lgh
