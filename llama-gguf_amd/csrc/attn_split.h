// attn_split.h — the split-softmax core of decode attention, shared by the f32 cache (attention.hip: attn_partial_kernel), the
// byte caches (attn_partial_q8_kernel) and the TurboQuant caches (attention_tq.hip: attn_tq_partial_kernel), and the table of shapes
// those kernels are instantiated for (internal).
//
// Every partial kernel deals the cached rows round-robin over splits x waves; a lane group of LPR lanes shares a row and keeps an
// online-softmax state (m, l, acc) per query head of the kv group.  The tail is the same everywhere: the row slots of a wave merge
// by xor shuffles (attn_merge_rows), the waves through LDS (attn_stash, attn_merge_waves), the workgroup leaves one (m, l, acc)
// partial per head (attn_store_partial), and a second kernel merges the splits (attn_combine_splits).  The steps use the fast
// __expf, the merges expf; no expression here may change its operands or their order: the callers' results are compared bit for bit
// with their parents' (tools/attn_bits.py).  Two callers spell a passage out where the function cost them a wave of occupancy (the
// stash of attn_partial_q8_kernel, the wave merge + store of attn_tq_partial_kernel; figures there and in profiles/attn_core_isa.md):
// a change to such a passage here has to be made there too, and tools/isa_compare.py shows whether the copy can go.
#pragma once

#include <type_traits>

#include "device_utils.h"

namespace lgh {

constexpr float kNegBig = -1e30f;   // "no row yet": exp(kNegBig - m) is 0 for every real score m

// one row enters the online softmax of a head: m, l take it in; returns a, the factor for what was accumulated so far; pe = the
// row's weight (0 when the lane's row is past the end)
__device__ __forceinline__ float osm_update(float& m, float& l, float s, bool valid, float& pe) {
  const float mn = valid ? fmaxf(m, s) : m;
  const float a = __expf(m - mn);            // v_exp_f32: ~2 ulp, far inside the attention tolerance
  pe = valid ? __expf(s - mn) : 0.0f;
  l = __builtin_fmaf(l, a, pe);
  m = mn;
  return a;
}

// a K / V row held 4 floats per lane by LPR lanes against the G query heads of its kv group
template <int G, int LPR>
__device__ __forceinline__ void attn_step4(const f32x4 (&qv)[G], f32x4 k4, f32x4 v4, float scale, bool valid, float (&m)[G], float (&l)[G],
                                           f32x4 (&acc)[G]) {
#pragma unroll
  for (int g = 0; g < G; g++) {
    float s = qv[g].x * k4.x;
    s = __builtin_fmaf(qv[g].y, k4.y, s);
    s = __builtin_fmaf(qv[g].z, k4.z, s);
    s = __builtin_fmaf(qv[g].w, k4.w, s);
    // sum over the LPR lanes of the row, in every lane: DPP inside a 16-lane row (no LDS crossbar), one cross-row
    // exchange when a row spans 32 lanes
    s += dpp_f<0xB1>(s);
    s += dpp_f<0x4E>(s);
    s += dpp_f<0x141>(s);
    s += dpp_f<0x140>(s);
    if (LPR == 32) s += __shfl_xor(s, 16, 64);
    s *= scale;
    float pe;
    const float a = osm_update(m[g], l[g], s, valid, pe);
    acc[g] = acc[g] * a + v4 * pe;
  }
}

// a head's accumulator is an f32x4 (4 output dims per lane) or N floats: acc = acc * a + (the accumulator `off` lanes away) * b
__device__ __forceinline__ void attn_merge_acc(f32x4& acc, int off, float a, float b) {
  f32x4 oa;
  oa.x = __shfl_xor(acc.x, off, 64); oa.y = __shfl_xor(acc.y, off, 64);
  oa.z = __shfl_xor(acc.z, off, 64); oa.w = __shfl_xor(acc.w, off, 64);
  acc = acc * a + oa * b;
}
template <int N>
__device__ __forceinline__ void attn_merge_acc(float (&acc)[N], int off, float a, float b) {
#pragma unroll
  for (int c = 0; c < N; c++) acc[c] = acc[c] * a + __shfl_xor(acc[c], off, 64) * b;
}
__device__ __forceinline__ void attn_stash_acc(float* dst, const f32x4& acc) { *reinterpret_cast<f32x4*>(dst) = acc; }   // dst: 16-byte aligned
template <int N>
__device__ __forceinline__ void attn_stash_acc(float* dst, const float (&acc)[N]) {
#pragma unroll
  for (int c = 0; c < N; c++) dst[c] = acc[c];
}

// merges the 64 / LPR row slots of the wave (lanes with equal lane % LPR hold the same output dims)
template <int G, int LPR, typename Acc>
__device__ __forceinline__ void attn_merge_rows(float (&m)[G], float (&l)[G], Acc (&acc)[G]) {
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
#pragma unroll
    for (int g = 0; g < G; g++) {
      const float om = __shfl_xor(m[g], off, 64), ol = __shfl_xor(l[g], off, 64);
      const float mn = fmaxf(m[g], om);
      const float a = expf(m[g] - mn), b = expf(om - mn);
      l[g] = l[g] * a + ol * b;
      attn_merge_acc(acc[g], off, a, b);
      m[g] = mn;
    }
  }
}

// the wave's merged state -> LDS, by the lanes of row slot 0: s_ml [NW][G][2], s_acc [NW][G][D]; a lane holds N = D / LPR dims of a row
template <int G, int N, int LPR, typename Acc>
__device__ __forceinline__ void attn_stash(float* s_ml, float* s_acc, uint32_t wave, uint32_t sub, uint32_t li, const float (&m)[G],
                                           const float (&l)[G], const Acc (&acc)[G]) {
  if (sub == 0) {
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (li == 0) { s_ml[(wave * G + g) * 2] = m[g]; s_ml[(wave * G + g) * 2 + 1] = l[g]; }
      attn_stash_acc(&s_acc[((size_t)wave * G + g) * (LPR * N) + li * N], acc[g]);
    }
  }
}

// output element (head g of the group, dim) of the workgroup: the NW stashed states merged -> its max, sum and accumulator
template <int NW, int G, int D>
__device__ __forceinline__ void attn_merge_waves(const float* s_ml, const float* s_acc, uint32_t g, uint32_t dim, float& mn, float& lsum, float& a) {
  mn = s_ml[g * 2];
#pragma unroll
  for (int w = 1; w < NW; w++) mn = fmaxf(mn, s_ml[(w * G + g) * 2]);
  lsum = 0.0f; a = 0.0f;
#pragma unroll
  for (int w = 0; w < NW; w++) {
    const float f = expf(s_ml[(w * G + g) * 2] - mn);
    lsum += s_ml[(w * G + g) * 2 + 1] * f;
    a += s_acc[((size_t)w * G + g) * D + dim] * f;
  }
}

// the split's partial of head slot p (= (kv head * n_splits + split) * G + g): the layout attn_combine_splits reads
template <int D>
__device__ __forceinline__ void attn_store_partial(float* part_ml, float* part_acc, size_t p, uint32_t dim, float mn,
                                                   float lsum, float a) {
  part_acc[p * D + dim] = a;
  if (dim == 0) { part_ml[p * 2] = mn; part_ml[p * 2 + 1] = lsum; }
}

// the tail of a partial kernel that leaves split partials: waves merged through LDS, thread t takes output elements t, t + 64 NW, ...
template <int NW, int G, int D>
__device__ __forceinline__ void attn_merge_store(const float* s_ml, const float* s_acc, float* part_ml, float* part_acc,
                                                 size_t pbase) {
  for (uint32_t e = threadIdx.x; e < (uint32_t)(G * D); e += NW * 64) {
    const uint32_t g = e / D, dim = e % D;
    float mn, lsum, a;
    attn_merge_waves<NW, G, D>(s_ml, s_acc, g, dim, mn, lsum, a);
    attn_store_partial<D>(part_ml, part_acc, pbase + g, dim, mn, lsum, a);
  }
}

// Merge of the splits for output element `dim` (one per thread; blockDim >= 64) of the head whose split s lives at p0 + s * g_per_kv:
//   sum_s acc_s * e^{m_s - m*} / sum_s l_s * e^{m_s - m*}.
// Every partial this thread will need is requested up front, so the kernel is ONE memory round trip long instead of two dependent
// ones (m/l first, accumulators after the barrier); lane s of the first wave owns split s.  s_f: 64 floats of LDS, s_linv: one.
// active: this thread has an output element (dim < head_dim); the others take part in the barrier and get 0 terms.
__device__ __forceinline__ float attn_combine_splits(const float* part_ml, const float* part_acc, size_t p0,
                                                     uint32_t g_per_kv, uint32_t head_dim, uint32_t n_splits, uint32_t dim, bool active,
                                                     float* s_f, float* s_linv) {
  float pa[32];
#pragma unroll
  for (uint32_t sidx = 0; sidx < 32; sidx++)
    pa[sidx] = (sidx < n_splits && active) ? part_acc[(p0 + (size_t)sidx * g_per_kv) * head_dim + dim] : 0.0f;
  if (threadIdx.x < 64) {
    const uint32_t sidx = threadIdx.x;
    const bool ok = sidx < n_splits;
    const float m = ok ? part_ml[(p0 + (size_t)sidx * g_per_kv) * 2] : kNegBig;
    const float l = ok ? part_ml[(p0 + (size_t)sidx * g_per_kv) * 2 + 1] : 0.0f;
    const float mn = wave_max(m);
    const float f = expf(m - mn);
    const float lsum = wave_sum(l * f);
    s_f[sidx] = f;
    if (sidx == 0) *s_linv = 1.0f / lsum;  // simd.rs:718-720: multiply by 1/sum
  }
  __syncthreads();
  float a = 0.0f;
#pragma unroll
  for (uint32_t sidx = 0; sidx < 32; sidx++) a += pa[sidx] * s_f[sidx];   // s_f of absent splits is exp(-1e30 - m) = 0
  return a * *s_linv;
}

// ---- host: the (head_dim, query heads per kv head) shapes the split kernels are instantiated for.  f(D, G) gets them as
// std::integral_constant<int, .>; any other shape is hipErrorInvalidValue.
template <int D, typename F>
static hipError_t attn_dispatch_group(uint32_t g, F& f) {
  using std::integral_constant;
  switch (g) {
    case 1: return f(integral_constant<int, D>{}, integral_constant<int, 1>{});
    case 2: return f(integral_constant<int, D>{}, integral_constant<int, 2>{});
    case 4: return f(integral_constant<int, D>{}, integral_constant<int, 4>{});
    case 8: return f(integral_constant<int, D>{}, integral_constant<int, 8>{});
    default: return hipErrorInvalidValue;
  }
}
template <typename F>
static hipError_t attn_dispatch(uint32_t head_dim, uint32_t g, F f) {
  if (head_dim == 128) return attn_dispatch_group<128>(g, f);
  if (head_dim == 64) return attn_dispatch_group<64>(g, f);
  return hipErrorInvalidValue;
}

}  // namespace lgh
