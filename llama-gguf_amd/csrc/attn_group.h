// attn_group.h — what the group decode kernels share (internal): attn_group_kernel over the f32 cache (attention_group.hip) and
// attn_group_kv8_kernel over the byte caches (attention_group_kv8.hip).  Both hold the query heads of a kv group as the N index of
// v_mfma_f32_16x16x4_f32, lane (n, c) = (lane & 15, lane >> 4) standing for head column n and the cached rows kv0 + 4c + i of a tile;
// here are the tile's entry into the online softmax of a head column and the workgroup's tail (waves merged through LDS, one
// unnormalised (m, l, acc) partial per real head).  No expression here may change its operands or their order: the f32 kernel's results
// are compared with its parent's.
#pragma once

#include "attn_split.h"

namespace lgh {

template <int D, int NW>
struct AttnGroupLds {
  static constexpr int DP = D + 4;   // padded row of the merge buffer
  static constexpr int kFloats = NW * 16 * DP + 2 * NW * 16;   // s_o [NW][16][DP], s_m, s_l [NW][16]
  static constexpr size_t kBytes = (size_t)kFloats * 4;
};

// The tile at rows kv0 .. kv0 + 15 enters the online softmax of head column n: st[i] = <q(head n), k(row kv0 + 4c + i)>, unscaled
// (AttnBlockCore::update without the causal term: every head sees rows < kv_len).  A row at or past kv_len is masked: weight 0.
// Leaves the rows' weights in pv (the B operand of O^T += V^T P^T) and the accumulators rescaled
template <int DQ>
__device__ __forceinline__ void attn_group_update(const f32x4& st, uint32_t kv0, uint32_t c, uint32_t kv_len, float scale, float& m_run,
                                                  float& l_run, f32x4 (&acc)[DQ], float (&pv)[4]) {
  float sv[4], mx = kNegBig;
  bool ok[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    ok[i] = kv0 + 4 * c + i < kv_len;
    sv[i] = ok[i] ? st[i] * scale : kNegBig;
    mx = fmaxf(mx, sv[i]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float mn = fmaxf(m_run, mx);
  const float alpha = __expf(m_run - mn);
  float ps = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; i++) { pv[i] = ok[i] ? __expf(sv[i] - mn) : 0.0f; ps += pv[i]; }
  ps += __shfl_xor(ps, 16, 64);
  ps += __shfl_xor(ps, 32, 64);
  l_run = __builtin_fmaf(l_run, alpha, ps);
  m_run = mn;
#pragma unroll
  for (int x = 0; x < DQ; x++) acc[x] = acc[x] * alpha;
}

// The workgroup's tail: every wave's (m, l, acc) -> LDS (a wave without a tile leaves kNegBig, 0, 0: weight 0 in every merge that has a
// real row), the NW states merged, wave 0 first (expf, as AttnBlockCore::merge), thread t taking output elements t, t + 64 NW, ... of
// the real heads; pbase: the partial slot of the group's head 0 in this split.  grp_lds: AttnGroupLds<D, NW>::kFloats floats
template <int D, int NW>
__device__ __forceinline__ void attn_group_merge_store(float* grp_lds, uint32_t wave, uint32_t n, uint32_t c, float m_run, float l_run,
                                                       const f32x4 (&acc)[D / 16], uint32_t g_per_kv, size_t pbase, float* part_ml,
                                                       float* part_acc) {
  constexpr int DQ = D / 16, DP = AttnGroupLds<D, NW>::DP;
  float (*s_o)[16][DP] = reinterpret_cast<float (*)[16][DP]>(grp_lds);
  float (*s_m)[16] = reinterpret_cast<float (*)[16]>(grp_lds + NW * 16 * DP);
  float (*s_l)[16] = s_m + NW;
  if (c == 0) { s_m[wave][n] = m_run; s_l[wave][n] = l_run; }
#pragma unroll
  for (int x = 0; x < DQ; x++) {
    s_o[wave][n][DQ * (4 * c + 0) + x] = acc[x].x;
    s_o[wave][n][DQ * (4 * c + 1) + x] = acc[x].y;
    s_o[wave][n][DQ * (4 * c + 2) + x] = acc[x].z;
    s_o[wave][n][DQ * (4 * c + 3) + x] = acc[x].w;
  }
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < g_per_kv * D; e += NW * 64) {
    const uint32_t g = e / D, dim = e % D;
    float mn = s_m[0][g];
#pragma unroll
    for (int w = 1; w < NW; w++) mn = fmaxf(mn, s_m[w][g]);
    float lsum = 0.0f, a = 0.0f;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const float f = expf(s_m[w][g] - mn);
      lsum += s_l[w][g] * f;
      a += s_o[w][g][dim] * f;
    }
    attn_store_partial<D>(part_ml, part_acc, pbase + g, dim, mn, lsum, a);
  }
}

// attention_group_kv8.hip: the byte layouts' launch of attn_group_launch (common.h), which checked the shape and the step's fields
hipError_t attn_group_kv8_launch(const KvLayout& l, const KvCache& kv, const AttnDecode& a);

}  // namespace lgh
