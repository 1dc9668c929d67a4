// attention_group.hip — decode attention over the f32 cache for ANY group size 1 .. 16 (query heads per kv head) on the matrix cores:
// the prompt pass's block attention (attn_block.h, attention.hip: attn_pf_mfma_kernel) turned on its side.  Where that kernel has the 16
// prompt tokens of one head as the N index of v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation), this one has the up-to-16
// query heads of one kv group, so a cached K / V row is read once per kv head whatever the group size is, and the group size is a
// run-time value: one kernel per head size, none per group.  It serves the shapes attn_dispatch (attn_split.h) has no split kernel for
// (3, 5, 6, 7 ... heads per kv head: Llama-3.2-3B, Qwen2.5, Yi-34B, InternLM2), on contexts that ask for it (LGH_ATTN_GROUP_MATRIX).
//
// Grid: n_kv * n_splits workgroups of NW waves.  A wave takes kv tiles of 16 cached rows, dealt round-robin over splits x waves as
// attn_partial_kernel deals rows, each wave with its own online-softmax state.  Lane (n, c) = (lane & 15, lane >> 4) stands for head
// column n of the group and, per tile, for the cached rows kv0 + 4c + i:
//   S^T = K Q^T   M = cached row, N = head; the contraction runs over d, lane group c owning dims [c D/4, (c+1) D/4) of both operands,
//                 so the K and Q fragments are plain 16-byte loads: D / 4 matrix instructions, the query fragment loaded once per wave;
//   O^T += V^T P^T  the D layout of S^T gives lane (n, c) the scores of rows 4c .. 4c+3 for head n, which is the B operand of four
//                 instructions whose contraction index stands for row 4c + i: the probabilities never leave their registers.  The A
//                 operand is V^T with output row m standing for dims D/16 m .. D/16 m + D/16 - 1: D / 16 x 4 matrix instructions.
// Head columns n >= G take head G - 1's query: computed, never stored.  A row index past the context is clamped to the last visible row
// for the load and its score masked to kNegBig in the update, so nothing stored past the context is ever read.  The next tile's K and V
// fragments are requested before the current tile's matrix work begins.  The waves merge through LDS (expf, as AttnBlockCore::merge) and
// the workgroup leaves one unnormalised (m, l, acc) partial per real head in the layout attn_store_partial / attn_combine_splits read;
// attn_combine_kernel (attention.hip) merges the splits unchanged and leaves wo's XQ image.
#include "attn_split.h"

namespace lgh {

template <int D, int NW>
struct AttnGroupLds {
  static constexpr int DP = D + 4;   // padded row of the merge buffer
  static constexpr size_t kBytes = (size_t)(NW * 16 * DP + 2 * NW * 16) * 4;   // s_o [NW][16][DP], s_m, s_l [NW][16]
};

template <int D, int NW>
__global__ void __launch_bounds__(NW * 64) attn_group_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ vc,
                                                             uint32_t g_per_kv, uint32_t max_seq, float scale, const int* pos_ptr,
                                                             uint32_t n_splits, float* __restrict__ part_ml, float* __restrict__ part_acc) {
  constexpr int DJ = D / 4;    // contraction steps of S^T (dims per lane group)
  constexpr int DQ = D / 16;   // output dims per M index
  constexpr int DP = AttnGroupLds<D, NW>::DP;
  extern __shared__ __attribute__((aligned(16))) float grp_lds[];
  float (*s_o)[16][DP] = reinterpret_cast<float (*)[16][DP]>(grp_lds);
  float (*s_m)[16] = reinterpret_cast<float (*)[16]>(grp_lds + NW * 16 * DP);
  float (*s_l)[16] = s_m + NW;

  const uint32_t kvh = blockIdx.x / n_splits, sp = blockIdx.x % n_splits;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, c = lane >> 4;
  // the position word by SCALAR load: the loop bounds depend on it
  const uint32_t kv_len = sload_u32(pos_ptr) + 1;
  const uint32_t kv_last = kv_len - 1, n_tiles = (kv_len + 15) / 16;
  auto row = [&](uint32_t r) { return r < kv_last ? r : kv_last; };   // clamped here, masked in the update

  // the query fragment: dims [c DJ, (c+1) DJ) of head column n (the group's last head in a padded column)
  float qf[DJ];
  {
    const uint32_t hq = n < g_per_kv ? n : g_per_kv - 1;
    const float* qp = q + ((size_t)kvh * g_per_kv + hq) * D + c * DJ;
#pragma unroll
    for (int j = 0; j < DJ; j += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(qp + j);
      qf[j] = v.x; qf[j + 1] = v.y; qf[j + 2] = v.z; qf[j + 3] = v.w;
    }
  }
  const float* kbase = kc + (size_t)kvh * max_seq * D;
  const float* vbase = vc + (size_t)kvh * max_seq * D;
  float m_run = kNegBig, l_run = 0.0f;
  f32x4 acc[DQ];   // acc[x][i] = O^T[dim DQ (4c + i) + x][head n] of this wave's tiles
#pragma unroll
  for (int x = 0; x < DQ; x++) acc[x] = (f32x4)(0.0f);

  // a tile's K fragment (row kv0 + n, dims [c DJ, (c+1) DJ)) and V fragments (rows kv0 + 4c + i, dims [n DQ, (n+1) DQ)); the cache is
  // read once per step: non-temporal
  f32x4 kn[DJ / 4], vn[4][DQ / 4];
  auto load_tile = [&](uint32_t tile) {
    const uint32_t kv0 = tile * 16;
    const float* kp = kbase + (size_t)row(kv0 + n) * D + c * DJ;
#pragma unroll
    for (int j = 0; j < DJ / 4; j++) kn[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(kp + 4 * j));
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float* vp = vbase + (size_t)row(kv0 + 4 * c + i) * D + n * DQ;
#pragma unroll
      for (int x = 0; x < DQ / 4; x++) vn[i][x] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vp + 4 * x));
    }
  };
  const uint32_t first = sp * NW + wave, stride = n_splits * NW;
  if (first < n_tiles) load_tile(first);
  for (uint32_t tile = first; tile < n_tiles; tile += stride) {   // wave-uniform
    f32x4 kf[DJ / 4], vf[4][DQ / 4];
#pragma unroll
    for (int j = 0; j < DJ / 4; j++) kf[j] = kn[j];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int x = 0; x < DQ / 4; x++) vf[i][x] = vn[i][x];
    if (tile + stride < n_tiles) load_tile(tile + stride);   // in flight while this tile is computed
    f32x4 st = (f32x4)(0.0f);
#pragma unroll
    for (int j = 0; j < DJ; j++) st = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j / 4][j % 4], qf[j], st, 0, 0, 0);
    // the tile enters the online softmax of head column n: st[i] = <q(head n), k(row kv0 + 4c + i)>, unscaled (AttnBlockCore::update
    // without the causal term: every head sees rows < kv_len)
    const uint32_t kv0 = tile * 16;
    float sv[4], pv[4], mx = kNegBig;
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
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int x = 0; x < DQ; x++) acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[i][x / 4][x % 4], pv[i], acc[x], 0, 0, 0);
  }

  // the wave's (m, l, acc) -> LDS (a wave without a tile leaves kNegBig, 0, 0: weight 0 in every merge that has a real row)
  if (c == 0) { s_m[wave][n] = m_run; s_l[wave][n] = l_run; }
#pragma unroll
  for (int x = 0; x < DQ; x++) {
    s_o[wave][n][DQ * (4 * c + 0) + x] = acc[x].x;
    s_o[wave][n][DQ * (4 * c + 1) + x] = acc[x].y;
    s_o[wave][n][DQ * (4 * c + 2) + x] = acc[x].z;
    s_o[wave][n][DQ * (4 * c + 3) + x] = acc[x].w;
  }
  __syncthreads();
  // the NW states merged, wave 0 first; thread t takes output elements t, t + 64 NW, ... of the real heads
  const size_t pbase = ((size_t)kvh * n_splits + sp) * g_per_kv;
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

template <int D, int NW>
static hipError_t attn_group_go(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  constexpr size_t lds = AttnGroupLds<D, NW>::kBytes;
  static bool attr_set[64] = {};
  if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(&attn_group_kernel<D, NW>), (int)lds, attr_set); e != hipSuccess) return e;
  hipLaunchKernelGGL((attn_group_kernel<D, NW>), dim3(l.n_kv * a.n_splits), dim3(NW * 64), lds, a.st, a.q, kv.k_f32(), kv.v_f32(), a.n_heads / l.n_kv,
                     l.max_seq, a.scale, a.pos, a.n_splits, a.part_ml, a.part_acc);
  return hipGetLastError();
}

bool attn_group_covers(uint32_t head_dim, uint32_t group) { return (head_dim == 64 || head_dim == 128) && group >= 1 && group <= 16; }

// The partial launch of a split step on the group kernel: the context's own f32 cache, the position from the device word.  The wave
// count follows the cache capacity as the split kernels' does (attn_f32_dispatch): 4 waves below 2048 rows, 8 from there
hipError_t attn_group_launch(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  if (!l.f32() || l.n_kv == 0 || a.n_heads % l.n_kv || !attn_group_covers(l.d, a.n_heads / l.n_kv) || !a.pos || a.n_seq || a.n_splits < 1 ||
      a.n_splits > 32 || !a.part_ml || !a.part_acc)
    return hipErrorInvalidValue;
  const bool long_ctx = l.max_seq >= 2048;
  if (l.d == 128) return long_ctx ? attn_group_go<128, 8>(l, kv, a) : attn_group_go<128, 4>(l, kv, a);
  return long_ctx ? attn_group_go<64, 8>(l, kv, a) : attn_group_go<64, 4>(l, kv, a);
}

}  // namespace lgh
