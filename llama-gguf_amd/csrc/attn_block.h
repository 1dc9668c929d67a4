// attn_block.h — the block-softmax core of the prompt pass's attention, shared by the f32 cache and the TurboQuant scratch
// (attention.hip: attn_pf_mfma_kernel) and the byte caches (attn_pf_kv8_kernel); attn_split.h's counterpart (internal).
//
// A workgroup = one query head x 16 prompt tokens; its NW waves take the kv tiles (16 cached rows each) round-robin, each with its
// own online-softmax state, merged through LDS at the end.  Lane (n, c) of a wave stands for token n of the tile and, per kv tile,
// for the four cached rows kv0 + 4c + i: it holds their scores S^T[4c + i][n] and, of the output, O^T[dim DQ (4c + i) + x][n].
// What a kernel keeps is how a cached tile becomes the operands of its matrix instructions, its prefetch and its epilogue.  The
// update uses the fast __expf, the merge expf; no expression here may change its operands or their order: the kernels' results are
// compared bit for bit with their parents' (tools/attn_bits.py).
#pragma once

#include "attn_split.h"

namespace lgh {

template <int D, int NW>
struct AttnBlockCore {
  static constexpr int DJ = D / 4;    // contraction steps of S^T (dims per lane group)
  static constexpr int DQ = D / 16;   // output dims per M index
  static constexpr int DP = D + 4;    // padded row of the merge buffer
  static constexpr size_t kLdsBytes = (size_t)(NW * 16 * DP + 2 * NW * 16) * 4;   // s_o, s_m, s_l: the launch's dynamic LDS

  uint32_t head, tt, kvh, lane, wave, n, c;
  uint32_t tok;       // this lane's token of the block (past its end in a part-filled tile: computed, never stored)
  uint32_t kv_last;   // last cached row
  uint32_t n_tiles;   // tiles the last token of this tile can see
  float (*s_o)[16][DP];   // [NW][16][DP]
  float (*s_m)[16];       // [NW][16]
  float (*s_l)[16];

  __device__ __forceinline__ AttnBlockCore(uint32_t g_per_kv, uint32_t pos0, uint32_t m_tokens) {
    extern __shared__ __attribute__((aligned(16))) float pf_lds[];
    s_o = reinterpret_cast<float (*)[16][DP]>(pf_lds);
    s_m = reinterpret_cast<float (*)[16]>(pf_lds + NW * 16 * DP);
    s_l = s_m + NW;
    head = blockIdx.x; tt = blockIdx.y; kvh = head / g_per_kv;
    lane = threadIdx.x & 63; wave = threadIdx.x >> 6; n = lane & 15; c = lane >> 4;
    tok = tt * 16 + n;
    kv_last = pos0 + m_tokens - 1;
    n_tiles = (pos0 + tt * 16 + 16 + 15) / 16;
  }

  // a cached row a fragment may read: rows past the block are clamped here and masked in update()
  __device__ __forceinline__ uint32_t row(uint32_t r) const { return r < kv_last ? r : kv_last; }

  // the query fragment: dims [c DJ, (c+1) DJ) of token n (the block's last token in a part-filled tile)
  __device__ __forceinline__ void load_q(float (&qf)[DJ], const float* __restrict__ q, uint32_t n_heads, uint32_t m_tokens) const {
    const uint32_t tokc = tok < m_tokens ? tok : m_tokens - 1;
    const float* qp = q + ((size_t)tokc * n_heads + head) * D + c * DJ;
#pragma unroll
    for (int j = 0; j < DJ; j += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(qp + j);
      qf[j] = v.x; qf[j + 1] = v.y; qf[j + 2] = v.z; qf[j + 3] = v.w;
    }
  }

  // the tile of rows kv0 .. kv0 + 15 enters the online softmax: st[i] = <q(token n), k(row kv0 + 4c + i)>, unscaled; token n sees
  // rows <= pos0 + tok.  Leaves the probabilities pv and the accumulator scaled for them
  __device__ __forceinline__ void update(f32x4 st, uint32_t kv0, uint32_t pos0, float scale, float& m_run, float& l_run, f32x4 (&acc)[DQ], float (&pv)[4]) const {
    float sv[4], mx = kNegBig;
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      ok[i] = kv0 + 4 * c + i <= pos0 + tok;
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

  // the wave's (m, l, acc) -> LDS, for all waves
  __device__ __forceinline__ void stash(float m_run, float l_run, const f32x4 (&acc)[DQ]) const {
    if (c == 0) { s_m[wave][n] = m_run; s_l[wave][n] = l_run; }
#pragma unroll
    for (int x = 0; x < DQ; x++) {
      s_o[wave][n][DQ * (4 * c + 0) + x] = acc[x].x;
      s_o[wave][n][DQ * (4 * c + 1) + x] = acc[x].y;
      s_o[wave][n][DQ * (4 * c + 2) + x] = acc[x].z;
      s_o[wave][n][DQ * (4 * c + 3) + x] = acc[x].w;
    }
    __syncthreads();
  }

  // the NW stashed states merged, wave 0 first: epi(t, dim, value) gets the normalised output element `dim` of the tile's token t,
  // for the tokens the block has.  The calling thread alone reads s_o[.][t][dim]: epi may store there
  template <typename Epi>
  __device__ __forceinline__ void merge(uint32_t m_tokens, Epi epi) const {
    for (uint32_t e = threadIdx.x; e < 16u * D; e += NW * 64) {
      const uint32_t t = e / D, dim = e % D;
      if (tt * 16 + t >= m_tokens) continue;
      float mn = s_m[0][t];
#pragma unroll
      for (int w = 1; w < NW; w++) mn = fmaxf(mn, s_m[w][t]);
      float lsum = 0.0f, a = 0.0f;
#pragma unroll
      for (int w = 0; w < NW; w++) {
        const float f = expf(s_m[w][t] - mn);
        lsum += s_l[w][t] * f;
        a += s_o[w][t][dim] * f;
      }
      epi(t, dim, a * (1.0f / lsum));   // simd.rs:718-720: multiply by 1/sum
    }
  }
};

}  // namespace lgh
