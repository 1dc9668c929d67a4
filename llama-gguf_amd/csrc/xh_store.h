// xh_store.h — the one writer of an XH chunk (device code; prefill.hip's row-wise kernels and tp_prefill.hip share it, so that every
// producer of an XH image rounds the same way).
#pragma once

#include "prefill.h"

namespace lgh {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// chunk `ch` (8 consecutive elements starting at 8*ch) of token t
__device__ __forceinline__ void xh_store_chunk(uint8_t* xh, uint32_t t, uint32_t ch, const float v[8]) {
  const uint32_t b = ch >> 5, q = ch & 31;
  // Every element is f16(f32 value), two roundings when the caller passes an f32 product.  The empty asm keeps that product an f32
  // value: without it hipcc folds the caller's multiply into the conversion for SOME elements of the chunk (v_fma_mix{lo,hi}_f16, one
  // rounding of the exact product; the others go through v_cvt_pk_f16_f32), and the same product is rounded differently depending on
  // its place in the chunk (found by tests/test_gpu_prefill_ref.py: the next XH against f16(hidden * norm_w) of the returned hidden).
  // NOT dead code: nothing checks it at build time, only the bit-exact XH checks of test_linear_step, test_ffn_step and test_moe_step
  // on the GPU fail without it (or when a compiler finds another way to fold the product into the conversion).
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    r[j] = v[j];
    asm("" : "+v"(r[j]));
  }
  h16x8 o = {(_Float16)r[0], (_Float16)r[2], (_Float16)r[1], (_Float16)r[3], (_Float16)r[4], (_Float16)r[6], (_Float16)r[5], (_Float16)r[7]};
  *reinterpret_cast<h16x8*>(xh + (size_t)b * kPfSlabBytes + t * 512 + ((q ^ (t & 15)) << 4)) = o;
}

}  // namespace lgh
