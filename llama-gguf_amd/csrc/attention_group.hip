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
// attn_combine_kernel (attention.hip) merges the splits unchanged and leaves wo's XQ image.  The softmax update and the tail are
// attn_group.h's, shared with the byte caches' kernel (attention_group_kv8.hip).
#include "attn_group.h"

namespace lgh {

template <int D, int NW>
__global__ void __launch_bounds__(NW * 64) attn_group_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ vc,
                                                             uint32_t g_per_kv, uint32_t max_seq, float scale, const int* pos_ptr,
                                                             uint32_t n_splits, float* __restrict__ part_ml, float* __restrict__ part_acc) {
  constexpr int DJ = D / 4;    // contraction steps of S^T (dims per lane group)
  constexpr int DQ = D / 16;   // output dims per M index
  extern __shared__ __attribute__((aligned(16))) float grp_lds[];

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
    float pv[4];
    attn_group_update<DQ>(st, tile * 16, c, kv_len, scale, m_run, l_run, acc, pv);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int x = 0; x < DQ; x++) acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[i][x / 4][x % 4], pv[i], acc[x], 0, 0, 0);
  }

  attn_group_merge_store<D, NW>(grp_lds, wave, n, c, m_run, l_run, acc, g_per_kv, ((size_t)kvh * n_splits + sp) * g_per_kv, part_ml, part_acc);
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

// The partial launch of a split step on the group kernels: the context's own cache, f32 here or int8 / FP8 (attention_group_kv8.hip:
// the launch also quantizes and stores the current token's rows, a.kv_new), the position from the device word.  The wave count follows
// the cache capacity as the split kernels' does (attn_f32_dispatch): 4 waves below 2048 rows, 8 from there
hipError_t attn_group_launch(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  if (l.tq() || l.n_kv == 0 || a.n_heads % l.n_kv || !attn_group_covers(l.d, a.n_heads / l.n_kv) || !a.pos || a.n_seq || a.n_splits < 1 ||
      a.n_splits > 32 || !a.part_ml || !a.part_acc)
    return hipErrorInvalidValue;
  if (l.staged()) return attn_group_kv8_launch(l, kv, a);
  const bool long_ctx = l.max_seq >= 2048;
  if (l.d == 128) return long_ctx ? attn_group_go<128, 8>(l, kv, a) : attn_group_go<128, 4>(l, kv, a);
  return long_ctx ? attn_group_go<64, 8>(l, kv, a) : attn_group_go<64, 4>(l, kv, a);
}

}  // namespace lgh
