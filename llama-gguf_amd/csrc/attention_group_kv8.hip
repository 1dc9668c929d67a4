// attention_group_kv8.hip — decode attention over the byte caches (int8 + row scales, FP8 E4M3 / E5M2; FMT 1 / 2 / 3) for ANY group size
// 1 .. 16 on the matrix cores: attn_group_kernel (attention_group.hip) reading bytes the way attn_pf_kv8_kernel (attention.hip) does.
// Grid, tile dealing, lane roles, the online softmax and the tail are the f32 kernel's (attn_group.h): n_kv * n_splits workgroups of NW
// waves, tiles of 16 cached rows round-robin over splits x waves, lane (n, c) = (lane & 15, lane >> 4) for head column n, columns
// n >= G computed on head G - 1's query and never stored, the group size a kernel argument.
//
// Operands: the K fragment of lane (n, c) is the D / 4 contiguous BYTES of row kv0 + n at byte c D / 4 (one 16-byte load at D = 64, two
// at 128), the V fragments the D / 16 bytes of rows kv0 + 4c + i at byte n D / 16 (4 or 8 bytes per row); for int8 the K and V scales of
// rows kv0 + 4c + i, the rows of this lane's scores, travel with them.  The next tile is requested as raw dwords before the current
// tile's matrix work starts (D = 128: 8 + 8 registers where the f32 kernel holds 32 + 32) and widened to f32 only once it is the current
// tile (kv8_codec.h: kv8_widen4, the hardware's converters for FP8).  An int8 row's scale multiplies its score (K) and its probability
// (V), not its elements.  Products run on v_mfma_f32_16x16x4_f32, D / 4 for S^T = K Q^T and D / 4 for O^T += V^T P^T per tile.
//
// The current token's row: rows [0, pos) are cached, row pos arrives as f32 (AttnDecode::kv_new).  Wave 0 of every workgroup quantizes
// its kv head's K and V rows with the decode path's quantizers (the same bits in every workgroup) into an LDS row, split 0 also stores
// them to the cache at row pos; after a barrier a lane whose row index is pos OR PAST it takes its fragment from the LDS row.  So the
// token attends to row pos through its stored values, a masked row (score kNegBig, probability 0) has a finite V operand, and nothing at
// or past row pos is ever read from the cache.  Only the last tile has such rows: a wave's first tile, when it lies wholly below pos, is
// requested before the quantization and the barrier.
#include "attn_group.h"
#include "kv8_codec.h"

namespace lgh {

template <int D, int NW>
struct AttnGroupKv8Lds {
  static constexpr int kRowAt = AttnGroupLds<D, NW>::kFloats;   // behind the merge buffer: K row, V row (D / 4 dwords each), K, V scale
  static constexpr size_t kBytes = (size_t)(kRowAt + 2 * (D / 4) + 2) * 4;
};

template <int D, int NW, int FMT>
__global__ void __launch_bounds__(NW * 64) attn_group_kv8_kernel(const float* __restrict__ q, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                                 float* __restrict__ ksc, float* __restrict__ vsc,
                                                                 const float* __restrict__ k_new, const float* __restrict__ v_new,
                                                                 uint32_t g_per_kv, uint32_t max_seq, float scale, const int* pos_ptr,
                                                                 uint32_t n_splits, float* __restrict__ part_ml, float* __restrict__ part_acc) {
  constexpr int DJ = D / 4;    // contraction steps of S^T = bytes of the K fragment
  constexpr int DQ = D / 16;   // output dims per M index = bytes of a V row's fragment
  constexpr int KW = DJ / 4, VW = DQ / 4;   // dwords of the K fragment, of one V row's fragment
  constexpr int LPR = D / 4;   // lanes (= dwords) of a staged row
  extern __shared__ __attribute__((aligned(16))) float grp_lds[];
  uint32_t* s_row = reinterpret_cast<uint32_t*>(grp_lds + AttnGroupKv8Lds<D, NW>::kRowAt);   // [K, V][LPR]
  float* s_sc = reinterpret_cast<float*>(s_row + 2 * LPR);                                    // [K, V] (int8)

  const uint32_t kvh = blockIdx.x / n_splits, sp = blockIdx.x % n_splits;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, c = lane >> 4;
  // the position word by SCALAR load: the loop bounds depend on it.  Rows [0, pos) come from the cache, row pos from the staged rows
  const uint32_t pos = sload_u32(pos_ptr);
  const uint32_t kv_len = pos + 1, n_tiles = pos / 16 + 1;
  const size_t hrow = (size_t)kvh * max_seq;   // first row of this kv head

  // a tile's raw K fragment, V fragments and (int8) the scales of rows kv0 + 4c + i; the cache is read once per step: non-temporal
  uint32_t kn[KW], vn[4][VW];
  float ksn[4], vsn[4];
  auto load_tile = [&](uint32_t tile) {
    const uint32_t kv0 = tile * 16;
    if (kv0 + n < pos) {
      const uint8_t* kp = kc + (hrow + kv0 + n) * D + c * DJ;
#pragma unroll
      for (int j = 0; j < KW; j += 4) {
        const u32x4 v = ldg_nt128(kp + 4 * j);
        kn[j] = v.x; kn[j + 1] = v.y; kn[j + 2] = v.z; kn[j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < KW; j++) kn[j] = s_row[c * KW + j];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t r = kv0 + 4 * c + i;
      if (r < pos) {
        const uint8_t* vp = vc + (hrow + r) * D + n * DQ;
        if (VW == 2) {
          const u32x2 v = ldg_nt64(vp);
          vn[i][0] = v.x; vn[i][VW - 1] = v.y;
        } else {
          vn[i][0] = ldg_nt32(vp);
        }
        if (FMT == 1) { ksn[i] = __builtin_nontemporal_load(ksc + hrow + r); vsn[i] = __builtin_nontemporal_load(vsc + hrow + r); }
      } else {
#pragma unroll
        for (int x = 0; x < VW; x++) vn[i][x] = s_row[LPR + n * VW + x];
        if (FMT == 1) { ksn[i] = s_sc[0]; vsn[i] = s_sc[1]; }
      }
    }
  };
  const uint32_t first = sp * NW + wave, stride = n_splits * NW;
  const bool first_cached = first + 1 < n_tiles;   // wave-uniform: not the last tile, every row of it below pos
  if (first_cached) load_tile(first);

  // the current token's rows: row group 0 of wave 0 takes K, row group 1 V (D = 64 has two more groups, which compute along and store
  // nothing); quantized here (every split the same bits), kept in LDS, stored by split 0
  if (wave == 0) {
    const uint32_t sub = (lane / LPR) & 1, li = lane % LPR;
    const f32x4 x = *reinterpret_cast<const f32x4*>((sub ? v_new : k_new) + (size_t)kvh * D + li * 4);
    float sc = 1.0f;
    uint32_t w;
    if (FMT == 1) w = quantize_row_i8<LPR>(x, sc);
    else w = fp8_encode<FMT>(x.x) | fp8_encode<FMT>(x.y) << 8 | fp8_encode<FMT>(x.z) << 16 | fp8_encode<FMT>(x.w) << 24;
    if (lane < 2 * LPR) {
      s_row[sub * LPR + li] = w;
      if (FMT == 1 && li == 0) s_sc[sub] = sc;
      if (sp == 0) {
        *reinterpret_cast<uint32_t*>((sub ? vc : kc) + (hrow + pos) * D + li * 4) = w;
        if (FMT == 1 && li == 0) (sub ? vsc : ksc)[hrow + pos] = sc;
      }
    }
  }
  __syncthreads();
  if (!first_cached && first < n_tiles) load_tile(first);

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
  float m_run = kNegBig, l_run = 0.0f;
  f32x4 acc[DQ];   // acc[x][i] = O^T[dim DQ (4c + i) + x][head n] of this wave's tiles
#pragma unroll
  for (int x = 0; x < DQ; x++) acc[x] = (f32x4)(0.0f);

  for (uint32_t tile = first; tile < n_tiles; tile += stride) {   // wave-uniform
    uint32_t kf[KW], vf[4][VW];
    float ks[4], vs[4];
#pragma unroll
    for (int j = 0; j < KW; j++) kf[j] = kn[j];
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
      for (int x = 0; x < VW; x++) vf[i][x] = vn[i][x];
      if (FMT == 1) { ks[i] = ksn[i]; vs[i] = vsn[i]; }
    }
    if (tile + stride < n_tiles) load_tile(tile + stride);   // raw bytes in flight while this tile is computed
    f32x4 st = (f32x4)(0.0f);
#pragma unroll
    for (int j = 0; j < KW; j++) {
      const f32x4 k4 = kv8_widen4<FMT>(kf[j]);
#pragma unroll
      for (int e = 0; e < 4; e++) st = __builtin_amdgcn_mfma_f32_16x16x4f32(k4[e], qf[4 * j + e], st, 0, 0, 0);
    }
    if (FMT == 1) {   // an int8 row's scale on its score
#pragma unroll
      for (int i = 0; i < 4; i++) st[i] = st[i] * ks[i];
    }
    float pv[4];
    attn_group_update<DQ>(st, tile * 16, c, kv_len, scale, m_run, l_run, acc, pv);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float p = FMT == 1 ? pv[i] * vs[i] : pv[i];   // ... and on its probability
#pragma unroll
      for (int x = 0; x < VW; x++) {
        const f32x4 v4 = kv8_widen4<FMT>(vf[i][x]);
#pragma unroll
        for (int e = 0; e < 4; e++) acc[4 * x + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(v4[e], p, acc[4 * x + e], 0, 0, 0);
      }
    }
  }
  attn_group_merge_store<D, NW>(grp_lds, wave, n, c, m_run, l_run, acc, g_per_kv, ((size_t)kvh * n_splits + sp) * g_per_kv, part_ml, part_acc);
}

template <int D, int NW, int FMT>
static hipError_t attn_group_kv8_go(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  constexpr size_t lds = AttnGroupKv8Lds<D, NW>::kBytes;
  static bool attr_set[64] = {};
  if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(&attn_group_kv8_kernel<D, NW, FMT>), (int)lds, attr_set); e != hipSuccess) return e;
  hipLaunchKernelGGL((attn_group_kv8_kernel<D, NW, FMT>), dim3(l.n_kv * a.n_splits), dim3(NW * 64), lds, a.st, a.q, kv.k_bytes(), kv.v_bytes(),
                     kv.kscale(), kv.vscale(), a.kv_new, a.kv_new + (size_t)l.n_kv * D, a.n_heads / l.n_kv, l.max_seq, a.scale, a.pos, a.n_splits,
                     a.part_ml, a.part_acc);
  return hipGetLastError();
}

template <int D, int NW>
static hipError_t attn_group_kv8_fmt(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  if (l.type == LGH_KV_INT8) return attn_group_kv8_go<D, NW, 1>(l, kv, a);
  if (l.type == LGH_KV_FP8_E4M3) return attn_group_kv8_go<D, NW, 2>(l, kv, a);
  return attn_group_kv8_go<D, NW, 3>(l, kv, a);
}

// attn_group_launch's byte layouts: the staged rows a.kv_new (K row | V row per kv head, f32), the scale arrays for int8
hipError_t attn_group_kv8_launch(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  if (l.type < LGH_KV_INT8 || l.type > LGH_KV_FP8_E5M2 || !a.kv_new || !kv.t[KV_K] || !kv.t[KV_V] || (l.has_scales() && (!kv.kscale() || !kv.vscale())))
    return hipErrorInvalidValue;
  const bool long_ctx = l.max_seq >= 2048;
  if (l.d == 128) return long_ctx ? attn_group_kv8_fmt<128, 8>(l, kv, a) : attn_group_kv8_fmt<128, 4>(l, kv, a);
  return long_ctx ? attn_group_kv8_fmt<64, 8>(l, kv, a) : attn_group_kv8_fmt<64, 4>(l, kv, a);
}

}  // namespace lgh
