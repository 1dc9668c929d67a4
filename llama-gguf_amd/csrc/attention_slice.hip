// attention_slice.hip — single-launch decode attention for contexts of at most 256 rows, the V product split by columns.
//
// attn_head_kernel (attention.hip) runs one workgroup per query head: 32 of 256 CUs on Llama-3-8B, each pulling the head's whole K and
// whole V through one CU's return path.  The scores need the full head dimension, the V product does not: output column d needs only
// V[:, d].  Here S workgroups serve a query head (grid x = kv head, y = head of the group, z = slice): every one of them repeats the
// head's scores and softmax — attn_head_kernel's passes 1 and 2, the same instructions — and then accumulates only the columns
// [z D / S, (z + 1) D / S) of the output, so it reads all of K but 1 / S of V.  No workgroup needs anything from another one: no
// partial, no merge, no counter, no second node.
//
// The bits are attn_head_kernel's, for the f32 output and for wo's XQ image.  There the sum of an output column is a fixed tree:
// row r = c 128 + j 16 RPW + chain (RPW = 256 / D; chain = wave RPW + vsub, 16 RPW of them) is accumulated per chain in the order (c, j)
// by FMA from 0, then the RPW chains of a wave by the xor tree, then the 16 waves in order, then x (1 / sum).  This kernel keeps that
// row-to-chain assignment and those orders; only the lanes that hold the chains differ: a row slice is D / (4 S) lanes wide, chain ch
// sits in threads [ch D / (4 S), (ch + 1) D / (4 S)), and the 16 RPW D / (4 S) = 1024 / S threads that carry chains are whole waves
// (the "V waves": they alone request and consume V).
//
// Everything is requested at entry, as on attn_head_kernel's path for these contexts: two 128-row chunks of K, and on the V waves the
// slice of all 256 rows, clamped to the last visible row.  No row loops, no refills.
#include "attn_split.h"
#include "xq.h"

namespace lgh {

template <int D, int G, int S>
__global__ void __launch_bounds__(1024) attn_slice_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ vc,
                                                          const int* pos_ptr, float* __restrict__ out, uint8_t* __restrict__ xq_out, uint32_t max_seq,
                                                          float scale, uint32_t cap_rows) {
  constexpr int NW = 16, CH = 128;             // waves; rows per chunk
  constexpr int NB = D / 32;                   // f32x4 per lane and chunk (K: the pieces of its row; V: the rows of its chain)
  constexpr int NCHAIN = NW * (256 / D);       // attn_head_kernel's (wave, row slot) pairs
  constexpr int W = D / S, LPS = W / 4;        // the slice: floats, lanes per row
  constexpr int VW = NCHAIN * LPS / 64;        // V waves
  static_assert(W % 16 == 0, "a slice is whole XQ chunks");
  static_assert(NCHAIN * LPS % 64 == 0 && (256 / D) * LPS <= 64, "chains fill whole waves; a wave's row slots meet inside it");
  static_assert(NCHAIN * NB == CH && NW * 8 == CH, "a chunk is one K sweep and NB rows of every chain");
  __shared__ float s_sc[kAttnSliceMaxRows];    // scaled score
  __shared__ float s_p[kAttnSliceMaxRows];     // exp(score - max), 0 from kv_len to the end of its chunk
  __shared__ __attribute__((aligned(16))) float s_acc[NW * W];
  __shared__ float s_sum[NW];

  const uint32_t kvh = blockIdx.x, head = kvh * G + blockIdx.y, col0 = blockIdx.z * W;
  const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t kl = lane & 7, ksub = lane >> 3;                   // K: piece of the row, row of the wave's 8
  const uint32_t ch = threadIdx.x / LPS, ls = threadIdx.x % LPS;    // V (threads of the V waves): chain, piece of the row slice
  const bool vwave = wave < (uint32_t)VW;                           // wave-uniform
  f32x4 qv[NB];
#pragma unroll
  for (int j = 0; j < NB; j++) qv[j] = *reinterpret_cast<const f32x4*>(q + (size_t)head * D + j * 32 + kl * 4);
  uint32_t kv_len = sload_u32(pos_ptr) + 1;   // scalar: the chunk count and the row clamp depend on it
  kv_len = kv_len < cap_rows ? kv_len : cap_rows;
  const uint32_t n_ch = (kv_len + CH - 1) / CH, last = kv_len - 1;   // n_ch <= 2: cap_rows <= kAttnSliceMaxRows

  const char* const kbase = reinterpret_cast<const char*>(kc + (size_t)kvh * max_seq * D);
  const char* const vbase = reinterpret_cast<const char*>(vc + (size_t)kvh * max_seq * D);
  const uint32_t krow0 = wave * 8 + ksub;
  // (unconditional requests, clamped to the last visible row, as in attn_head_kernel)
  auto load_k = [&](f32x4 (&k)[NB], uint32_t c) {
    const uint32_t r = c * CH + krow0, off = (r < last ? r : last) * (D * 4) + kl * 16;
#pragma unroll
    for (int j = 0; j < NB; j++) k[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(kbase + off + j * 128));
  };
  f32x4 kb[2][NB], vb[2][NB];
  load_k(kb[0], 0);
  load_k(kb[1], 1);
  // the query takes the scale here, behind the first requests
#pragma unroll
  for (int j = 0; j < NB; j++) qv[j] = qv[j] * scale;

  // ---- 1. scores: attn_head_kernel's
  // (computed for a row group wholly past the end too, and not stored: a wave that skipped it would carry its pending requests into the
  // join below, where the V waves' waits would count for them)
  auto score = [&](const f32x4 (&k)[NB], uint32_t c) {
    float s = qv[0].x * k[0].x;
    s = __builtin_fmaf(qv[0].y, k[0].y, s); s = __builtin_fmaf(qv[0].z, k[0].z, s); s = __builtin_fmaf(qv[0].w, k[0].w, s);
#pragma unroll
    for (int j = 1; j < NB; j++) {
      s = __builtin_fmaf(qv[j].x, k[j].x, s); s = __builtin_fmaf(qv[j].y, k[j].y, s);
      s = __builtin_fmaf(qv[j].z, k[j].z, s); s = __builtin_fmaf(qv[j].w, k[j].w, s);
    }
    s += dpp_f<0xB1>(s);    // the 8 lanes of the row: quad_perm x2, row_half_mirror
    s += dpp_f<0x4E>(s);
    s += dpp_f<0x141>(s);
    const uint32_t r = c * CH + krow0;
    if (kl == 0 && r < kv_len) s_sc[r] = s;
  };
  // The V waves request their slice of all rows behind K.  Two copies of the score pass, not a branch around the requests alone: behind
  // such a branch every wait would count for its worse side, and a V wave would wait for V before its first score.
  if (vwave) {
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int j = 0; j < NB; j++) {
        const uint32_t r = c * CH + j * NCHAIN + ch, off = (r < last ? r : last) * (D * 4) + (col0 + ls * 4) * 4;
        vb[c][j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vbase + off));
      }
    score(kb[0], 0);
    score(kb[1], 1);
  } else {
    score(kb[0], 0);
    score(kb[1], 1);
  }
  __syncthreads();

  // ---- 2. the head's maximum (every wave for itself), then p and its sum, each row once: attn_head_kernel's
  float mx = kNegBig;
  for (uint32_t b = 0; b < kv_len; b += 64) {
    const uint32_t r = b + lane;
    const float s = s_sc[r < last ? r : last];
    mx = s > mx ? s : mx;
  }
  mx = wave_max_dpp(mx);
  float ps = 0.0f;
  for (uint32_t b = wave * 64; b < n_ch * CH; b += NW * 64) {
    const uint32_t r = b + lane;
    const float p = r < kv_len ? __expf(s_sc[r < last ? r : last] - mx) : 0.0f;
    s_p[r] = p;
    ps += p;
  }
  ps = wave_sum_to_lane63(ps);
  if (lane == 63) s_sum[wave] = ps;
  __syncthreads();

  // ---- 3. out[col0 .. col0 + W) = sum_r p_r V[r]: a chain's rows in the order (c, j), then the row slots of a wave by the xor tree
  if (vwave) {
    f32x4 acc = (f32x4)(0.0f);
#pragma unroll
    for (int c = 0; c < 2; c++) {
      if ((uint32_t)c >= n_ch) continue;   // (s_p ends with the last chunk that has a visible row; in it rows past the end have p = 0)
      float p[NB];
#pragma unroll
      for (int j = 0; j < NB; j++) p[j] = s_p[c * CH + j * NCHAIN + ch];
#pragma unroll
      for (int j = 0; j < NB; j++) {
        acc.x = __builtin_fmaf(p[j], vb[c][j].x, acc.x); acc.y = __builtin_fmaf(p[j], vb[c][j].y, acc.y);
        acc.z = __builtin_fmaf(p[j], vb[c][j].z, acc.z); acc.w = __builtin_fmaf(p[j], vb[c][j].w, acc.w);
      }
    }
#pragma unroll
    for (int off = LPS; off < (256 / D) * LPS; off <<= 1) {
      acc.x += __shfl_xor(acc.x, off, 64); acc.y += __shfl_xor(acc.y, off, 64);
      acc.z += __shfl_xor(acc.z, off, 64); acc.w += __shfl_xor(acc.w, off, 64);
    }
    if (ch % (256 / D) == 0) *reinterpret_cast<f32x4*>(&s_acc[ch / (256 / D) * W + ls * 4]) = acc;   // [attn_head_kernel's wave][column of the slice]
  }
  __syncthreads();

  // ---- 4. the 16 waves' sums in order, x (1 / sum)
  if (threadIdx.x < (uint32_t)W) {   // whole 16-lane rows: an XQ chunk each
    const uint32_t dim = threadIdx.x;
    float o = s_acc[dim], sum = s_sum[0];
#pragma unroll
    for (int w = 1; w < NW; w++) { o += s_acc[w * W + dim]; sum += s_sum[w]; }
    o = o * (1.0f / sum);   // simd.rs:718-720: multiply by 1/sum
    out[(size_t)head * D + col0 + dim] = o;
    if (xq_out) xq_store_chunk(xq_out, (head * D + col0 + dim) >> 4, o);   // wo's input as XQ records
  }
}

// One S per head size, from the node's duration at 72 .. 256 rows (profiles/attn_slice.md): at D = 128, 4 and 8 tie and 2 is slower; at
// D = 64, 4 (a slice of one XQ chunk, the narrowest there is) beats 2
template <int D> constexpr int kAttnSliceS = 4;

hipError_t attn_slice_launch(const float* q, const float* kcache, const float* vcache, uint32_t n_heads, uint32_t n_kv, uint32_t head_dim,
                             uint32_t max_seq, float scale, const int* pos, uint32_t max_rows, float* out, uint8_t* xq_out, hipStream_t st) {
  if (n_kv == 0 || n_heads % n_kv || !pos || max_rows == 0 || max_seq == 0) return hipErrorInvalidValue;
  const uint32_t rows = max_rows < max_seq ? max_rows : max_seq;
  if (rows > kAttnSliceMaxRows) return hipErrorInvalidValue;
  const uint32_t cap_rows = (rows + 127) / 128 * 128;
  return attn_dispatch(head_dim, n_heads / n_kv, [&](auto d, auto gg) {
    constexpr int D = decltype(d)::value, G = decltype(gg)::value, S = kAttnSliceS<D>;
    hipLaunchKernelGGL((attn_slice_kernel<D, G, S>), dim3(n_kv, G, S), dim3(1024), 0, st, q, kcache, vcache, pos, out, xq_out, max_seq, scale, cap_rows);
    return hipGetLastError();
  });
}

}  // namespace lgh
