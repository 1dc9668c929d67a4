// device_utils.h — small gfx950 device helpers (internal).
#pragma once

#include "common.h"

namespace lgh {

// streamed-once weights: non-temporal 16-byte loads straight to VGPRs (no LDS round trip for GEMV)
__device__ __forceinline__ u32x4 ldg_nt128(const void* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}
__device__ __forceinline__ u32x2 ldg_nt64(const void* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
}
__device__ __forceinline__ uint32_t ldg_nt32(const void* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
}
__device__ __forceinline__ uint16_t ldg_nt16(const void* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p));
}

__device__ __forceinline__ float h2f(uint32_t bits16) {
  _Float16 h;
  uint16_t b = (uint16_t)bits16;
  __builtin_memcpy(&h, &b, 2);
  return (float)h;  // v_cvt_f32_f16, subnormals preserved
}

__device__ __forceinline__ float ub0(uint32_t v) { return (float)(v & 0xFFu); }
__device__ __forceinline__ float ub1(uint32_t v) { return (float)((v >> 8) & 0xFFu); }
__device__ __forceinline__ float ub2(uint32_t v) { return (float)((v >> 16) & 0xFFu); }
__device__ __forceinline__ float ub3(uint32_t v) { return (float)(v >> 24); }

// 4 FMAs of the 4 bytes of `v` against x[0..3]
__device__ __forceinline__ float fma4(uint32_t v, const float* x, float acc) {
  acc = __builtin_fmaf(ub0(v), x[0], acc);
  acc = __builtin_fmaf(ub1(v), x[1], acc);
  acc = __builtin_fmaf(ub2(v), x[2], acc);
  acc = __builtin_fmaf(ub3(v), x[3], acc);
  return acc;
}

// Makes `v` opaque to the optimizer at this point (no instruction is emitted).  Used after nibble masks so
// that `(m >> 8) & 0xFF` stays a single v_cvt_f32_ubyte1 instead of being re-folded into v_bfe_u32 + cvt.
__device__ __forceinline__ uint32_t opaque(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

// the 4 bytes of `v` dotted with x[0..3], as a fresh chain (first term is a plain multiply)
__device__ __forceinline__ float fma4z(uint32_t v, const float* x) {
  float acc = ub0(v) * x[0];
  acc = __builtin_fmaf(ub1(v), x[1], acc);
  acc = __builtin_fmaf(ub2(v), x[2], acc);
  acc = __builtin_fmaf(ub3(v), x[3], acc);
  return acc;
}

// A wave-uniform word (a position, a slot, a count) by SCALAR load, waited for: what follows (loop bounds, base addresses) depends on
// it, and a vector load would be a full memory round trip into VGPRs first.  The second form requests two words and waits once.
__device__ __forceinline__ uint32_t sload_u32(const void* p) {
  uint32_t w;
  asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w) : "s"(p) : "memory");
  return w;
}
__device__ __forceinline__ void sload_u32x2(const void* pa, const void* pb, uint32_t& a, uint32_t& b) {
  asm volatile("s_load_dword %0, %2, 0x0\n\ts_load_dword %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a), "=&s"(b) : "s"(pa), "s"(pb) : "memory");
}

// full-wave (64 lanes) sum; every lane gets the result; fixed order -> deterministic
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// DPP lane permutation of a float (gfx9 DPP controls): no LDS crossbar, full-rate VALU
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false));
}

// 64-lane sum by DPP; the total is valid in LANE 63 only.  Fixed order -> deterministic.
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
  v += dpp_f<0xB1>(v);        // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);        // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);       // row_half_mirror
  v += dpp_f<0x140>(v);       // row_mirror  -> every lane of a 16-lane row holds the row sum
  v += dpp_f<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
  v += dpp_f<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3
  return v;
}

// 64-lane maximum by DPP (the steps of wave_sum_to_lane63; a row the mask leaves out keeps its own value), lane 63's total to every lane
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_max(float v) {
  const int b = __builtin_bit_cast(int, v);
  return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, CTRL, ROW_MASK, 0xF, false)));
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  v = dpp_max<0xB1>(v);
  v = dpp_max<0x4E>(v);
  v = dpp_max<0x141>(v);
  v = dpp_max<0x140>(v);
  v = dpp_max<0x142, 0xA>(v);
  v = dpp_max<0x143, 0xC>(v);
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// arg-max with the reference's tie rule (the LAST maximal element wins): misc.hip's two stages and the output projection's
// static plan (matvec_mfma.hip) merge with the same rule, so the result does not depend on how the rows are partitioned
__device__ __forceinline__ void amax_merge(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i > bi)) { bv = v; bi = i; }
}

__device__ __forceinline__ void amax_block_reduce(float& bv, int& bi, float* sv, int* si) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    float ov = __shfl_xor(bv, off, 64);
    int oi = __shfl_xor(bi, off, 64);
    amax_merge(bv, bi, ov, oi);
  }
  const uint32_t tid = threadIdx.x;
  if ((tid & 63) == 0) { sv[tid >> 6] = bv; si[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w < (blockDim.x >> 6); w++) amax_merge(bv, bi, sv[w], si[w]);
  }
}

}  // namespace lgh
