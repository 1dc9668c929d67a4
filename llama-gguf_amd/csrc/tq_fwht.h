// tq_fwht.h — the Walsh-Hadamard butterflies of the TurboQuant rotation (src/model/turboquant/rotation.rs:113-130), shared by the
// decode attention over the code caches (attention_tq.hip) and the prompt pass's TurboQuant epilogue (attention.hip).
#pragma once

#include "device_utils.h"

namespace lgh {

// In-place Walsh-Hadamard butterflies over `rows` vectors of D floats in LDS (rotation.rs:113-130): stage `half` combines (i, i +
// half) exactly as the reference's loop does; all threads of the workgroup take part (barriers inside).
template <int D>
__device__ __forceinline__ void tq_fwht_rows(float* buf, uint32_t rows) {
  for (uint32_t half = 1; half < (uint32_t)D; half <<= 1) {
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < rows * (D / 2); j += blockDim.x) {
      const uint32_t r = j / (D / 2), jj = j % (D / 2);
      const uint32_t i = (jj / half) * 2 * half + (jj % half);
      float* v = buf + r * D;
      const float a = v[i], b = v[i + half];
      v[i] = a + b;
      v[i + half] = a - b;
    }
  }
  __syncthreads();
}

// The same butterflies for ONE vector per wave, in registers: lane l holds elements l (and l + 64 when D = 128).  Stage `half`
// pairs (i, i + half), i without bit `half`: new[i] = a + b, new[i + half] = a - b with a the lower element — the partner comes
// through a cross-lane exchange, the operations and their operands are the reference's (rotation.rs:113-130): bit-identical to
// tq_fwht_rows, without its barrier per stage.
template <int D>
__device__ __forceinline__ void tq_fwht_wave(float& x0, float& x1, uint32_t lane) {
#pragma unroll
  for (uint32_t half = 1; half < 64 && half < (uint32_t)D; half <<= 1) {
    const bool upper = (lane & half) != 0;
    const float p0 = __shfl_xor(x0, (int)half, 64);
    x0 = upper ? p0 - x0 : x0 + p0;
    if (D == 128) {
      const float p1 = __shfl_xor(x1, (int)half, 64);
      x1 = upper ? p1 - x1 : x1 + p1;
    }
  }
  if (D == 128) {   // half = 64: the lane's own two elements
    const float a = x0, b = x1;
    x0 = a + b;
    x1 = a - b;
  }
}

}  // namespace lgh
