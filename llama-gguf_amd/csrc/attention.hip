// attention.hip — single-token GQA attention over the HBM-resident f32 KV cache.
//
// Replaces `flash_attention_cached` (src/backend/cuda/kernels.rs:1395-1458: one workgroup per query
// head, a SERIAL loop over kv positions with two block-wide reductions per position) and follows the
// CPU backend's `attention_cached` (src/backend/cpu/ops.rs:1479-1537): score = <q,k>*scale, softmax over
// kv_len, out = sum_p w_p * V[p].  KV layout is the reference's [n_kv_heads, max_seq, head_dim] f32
// (src/model/mod.rs:64-108).
//
// Decode attention is a latency problem at short context and an HBM stream at long context, so:
//   * work is split over (kv head) x (n_splits) workgroups, each with 4 waves; positions are dealt
//     round-robin so every workgroup has work from the first cached token on;
//   * the G = n_heads/n_kv_heads query heads of a kv group are processed together: one 16-byte K/V load
//     per lane serves all G heads (GQA reuse), K/V rows go straight to VGPRs (no LDS staging);
//   * a row of head_dim floats is spread over head_dim/4 lanes, so one wave-instruction covers 2 rows
//     (d=128) or 4 rows (d=64), fully coalesced 512-byte / 256-byte rows;
//   * online softmax per lane group; partial (m, l, acc) states merge in registers, then LDS, then in
//     a tiny combine kernel across splits.
// The reference CPU path skips softmax weights <= 1e-8 (ops.rs:1529); like the reference's own GPU
// kernel this one does not (each skipped term is < 1e-8 of the output scale).
#include <cstdlib>

#include "attn_block.h"
#include "tq_fwht.h"
#include "xq.h"
#include "prefill.h"
#include "timeline.h"

LGH_TL_DEFINE(attn)

namespace lgh {

// NW waves per workgroup (positions are dealt round-robin over splits x waves): 4 is faster at short context (608 vs 600
// tokens/s at kv 272), 8 at long (543 vs 524 at kv 4000); the launcher picks by the cache capacity.
// PF (prefill.hip): blockIdx.y = token t of a block of prompt tokens; it sees kv_len_fixed + t cache rows (causal), its
// query is q + t * n_heads * D, there is one split, and the normalised output goes, as f16, into the XH matrix at
// `part_acc` (prefill.h: the wo GEMM's input).
// DIRECT: one workgroup of NW = 16 waves per kv head and no second kernel: the workgroup merges its waves and writes the
// normalised output (f32 at part_acc, XQ records at part_ml when not null) itself.  It saves one launch floor per layer but
// every lane of a row repeats the online-softmax update and every merge is full of exponentials: bound by vector issue, it only
// paid below ~100 rows.  The engine's single launch is attn_head_kernel below; this one stays for lgh_op_attention_decode path 1.
// MULTI (multi-sequence decode, engine_batch.hip): blockIdx.y = sequence s of the step; its query is q + s * n_heads * D, its
// position pos_ptr[s], its K / V the cache slot slot[s] (slot_stride floats apart), its partials the s-th block of
// part_ml / part_acc.  Per sequence the arithmetic is the single-sequence kernel's.
template <int D, int G, int NW, bool PF = false, bool DIRECT = false, bool MULTI = false>
__global__ void __launch_bounds__(NW * 64) attn_partial_kernel(const float* __restrict__ q, const float* __restrict__ kc,
                                                           const float* __restrict__ vc, uint32_t max_seq, float scale,
                                                           const int* pos_ptr, int kv_len_fixed, uint32_t n_splits,
                                                           float* __restrict__ part_ml, float* __restrict__ part_acc,
                                                           const int* __restrict__ slot = nullptr, uint64_t slot_stride = 0) {
  constexpr int LPR = D / 4;       // lanes per row
  constexpr int RPW = 64 / LPR;    // rows per wave-instruction
  __shared__ float s_ml[NW * G * 2];
  __shared__ __attribute__((aligned(16))) float s_acc[NW * G * D];
  LGH_TL_BEGIN(attn, lgh::TL_ATTN, n_splits);

  const uint32_t kvh = blockIdx.x / n_splits, sp = blockIdx.x % n_splits;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t sub = lane / LPR, li = lane % LPR;
  // the position word by SCALAR load: the loop bounds depend on it, and a vector load here would be a full memory round
  // trip before the first K/V row can be requested
  uint32_t kv_len = (uint32_t)kv_len_fixed;
  if (PF) {
    kv_len += blockIdx.y;
    q += (size_t)blockIdx.y * gridDim.x * G * D;   // gridDim.x = kv heads (one split)
  } else if (MULTI) {
    const uint32_t sq = blockIdx.y;
    uint32_t pw, sl;
    sload_u32x2(pos_ptr + sq, slot + sq, pw, sl);
    kv_len = pw + 1;
    q += (size_t)sq * (gridDim.x / n_splits) * G * D;
    kc += (size_t)sl * slot_stride;
    vc += (size_t)sl * slot_stride;
    part_ml += (size_t)sq * gridDim.x * G * 2;
    part_acc += (size_t)sq * gridDim.x * G * D;
  } else if (pos_ptr) {
    kv_len = sload_u32(pos_ptr) + 1;
  }

  f32x4 qv[G];
#pragma unroll
  for (int g = 0; g < G; g++) qv[g] = *reinterpret_cast<const f32x4*>(q + ((size_t)kvh * G + g) * D + li * 4);

  float m[G], l[G];
  f32x4 acc[G];
#pragma unroll
  for (int g = 0; g < G; g++) { m[g] = kNegBig; l[g] = 0.0f; acc[g] = (f32x4)(0.0f); }

  const float* kbase = kc + (size_t)kvh * max_seq * D + li * 4;
  const float* vbase = vc + (size_t)kvh * max_seq * D + li * 4;
  const uint32_t stride = n_splits * NW * RPW;
  auto row_of = [&](uint32_t base) { const uint32_t p = base + sub; return p < kv_len ? p : kv_len - 1; };   // clamped: loads are unconditional
  // (through this lambda, not called in the loop directly: that cost the <128, 4, *> instantiations a wave of occupancy, 97-98 VGPRs for 94-96)
  auto step = [&](uint32_t base, f32x4 k4, f32x4 v4) { attn_step4<G, LPR>(qv, k4, v4, scale, base + sub < kv_len, m, l, acc); };
  // Batches of kAhead iterations: all their K/V rows are requested before the first one is used (clamped when past the
  // end, so the loads are unconditional).  At decode lengths a workgroup has 1-3 iterations and everything is in flight
  // at once; at 4K context it has ~30, and with a single iteration ahead the kernel ran at 1 TB/s (latency-bound).
  constexpr int kAhead = 4;   // (8 measured slower: 604 / 518 vs 614 / 528 tokens/s at kv 272 / 4000)
  for (uint32_t base = (sp * NW + wave) * RPW; base < kv_len; base += kAhead * stride) {
    f32x4 kk[kAhead], vv[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; j++) {
      const uint32_t r = row_of(base + j * stride);
      kk[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(kbase + (size_t)r * D));
      vv[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vbase + (size_t)r * D));
    }
#pragma unroll
    for (int j = 0; j < kAhead; j++)
      if (base + j * stride < kv_len) step(base + j * stride, kk[j], vv[j]);   // wave-uniform
  }

  attn_merge_rows<G, LPR>(m, l, acc);
  attn_stash<G, 4, LPR>(s_ml, s_acc, wave, sub, li, m, l, acc);
  __syncthreads();
  // merge the NW waves; thread t handles output elements t, t + 64 NW, ...
  const size_t pbase = ((size_t)kvh * n_splits + sp) * G;
  for (uint32_t e = threadIdx.x; e < (uint32_t)(G * D); e += NW * 64) {
    const uint32_t g = e / D, dim = e % D;
    float mn, lsum, a;
    attn_merge_waves<NW, G, D>(s_ml, s_acc, g, dim, mn, lsum, a);
    if (DIRECT) {
      const float o = a * (1.0f / lsum);   // simd.rs:718-720: multiply by 1/sum
      part_acc[(pbase + g) * D + dim] = o;
      if (part_ml) xq_store_chunk(reinterpret_cast<uint8_t*>(part_ml), (uint32_t)((pbase + g) * D + dim) >> 4, o);   // wo's input as XQ records
    } else if (PF) {
      const _Float16 o = (_Float16)(a * (1.0f / lsum));   // simd.rs:718-720: multiply by 1/sum
      *reinterpret_cast<_Float16*>(reinterpret_cast<uint8_t*>(part_acc) + xh_offset(blockIdx.y, (uint32_t)(pbase + g) * D + dim)) = o;
    } else {
      attn_store_partial<D>(part_ml, part_acc, pbase + g, dim, mn, lsum, a);
    }
  }
  LGH_TL_END();
}

// ------------------------------------------------------------------------------------------------
// HEAD: decode attention in one launch, one workgroup of 16 waves per QUERY head (grid x = kv head, y = head of the group: the
// G workgroups that re-read a kv head's K / V follow each other n_kv apart in dispatch order, so with n_kv % 8 == 0 they share
// an XCD's L2 — for speed only).  A softmax in two passes instead of an online one per row:
//   1. scores: a K row is spread over 8 lanes (D / 8 floats each, every load instruction covers 128-byte pieces of 8 rows), the
//      lane sum is 3 DPP steps, the score goes to LDS, one float per visible row.  The score is (q * scale) . k, the query scaled
//      once at entry, where the split kernels compute (q . k) * scale: one rounding per term apart, so the bits of the two differ;
//   2. every wave takes the maximum over all scores itself (no barrier), the workgroup computes p = exp(s - max) once per row
//      into LDS and each wave leaves the sum of the p it computed;
//   3. out[d] = sum_r p_r V[r][d] with V rows spread over D / 4 lanes as in attn_partial_kernel, p_r from LDS;
//   4. row slots (xor shuffles) and waves (LDS) merge by plain additions in a fixed order: one maximum for the whole head, so
//      no exponential in any merge; the result times 1 / sum goes out as f32 and as wo's XQ image.
// Rows are dealt in chunks of 128 (K: 8 per wave; V: D / 32 sweeps of 64 / (D / 4) per wave) and a thread has four chunk buffers.
// Up to 256 rows, two chunks of K and two of V — everything the head needs — are requested before the first is used.  Longer
// contexts keep four chunks in flight: four of K at entry, and every buffer is refilled as soon as it has been consumed, with the K
// chunk four ahead or, after the last group of four, with V chunk 0..3, so that V streams in under the remaining scores and the
// softmax; the V loop refills the same way.  Every request is clamped to the last visible row (unconditional requests keep the
// counted waits in front of their uses exact); a row past the end has no score stored and p = 0, so nothing of it reaches the result.
// cap_rows (a multiple of 128): the rows the LDS arrays hold.  A position past it would be attended to as cap_rows rows (the clamp
// below keeps every LDS index inside the arrays); no caller lets it happen: attention_forward refuses such a position on the host.
// ------------------------------------------------------------------------------------------------
template <int D, int G>
__global__ void __launch_bounds__(1024) attn_head_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ vc,
                                                         const int* pos_ptr, float* __restrict__ out, uint8_t* __restrict__ xq_out, uint32_t max_seq,
                                                         float scale, uint32_t cap_rows) {
  constexpr int NW = 16, CH = 128;             // waves; rows per chunk
  constexpr int NB = D / 32;                   // f32x4 per lane and chunk (K: the pieces of its row; V: sweeps)
  constexpr int LPR = D / 4, RPW = 64 / LPR;   // V: lanes per row, rows per wave-instruction
  static_assert(NW * RPW * NB == CH && NW * 8 == CH, "a chunk is one K sweep and NB V sweeps");
  extern __shared__ __attribute__((aligned(16))) float ah_lds[];
  float* const s_sc = ah_lds;                  // [cap_rows] scaled score
  float* const s_p = s_sc + cap_rows;          // [cap_rows] exp(score - max), 0 from kv_len to the end of its chunk
  float* const s_acc = s_p + cap_rows;         // [NW][D]
  float* const s_sum = s_acc + NW * D;         // [NW]
  LGH_TL_BEGIN(attn, lgh::TL_ATTN, 1);

  const uint32_t kvh = blockIdx.x, head = kvh * G + blockIdx.y;
  const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t kl = lane & 7, ksub = lane >> 3;      // K: piece of the row, row of the wave's 8
  const uint32_t li = lane % LPR, vsub = lane / LPR;   // V: as attn_partial_kernel
  f32x4 qv[NB];
#pragma unroll
  for (int j = 0; j < NB; j++) qv[j] = *reinterpret_cast<const f32x4*>(q + (size_t)head * D + j * 32 + kl * 4);
  uint32_t kv_len = sload_u32(pos_ptr) + 1;   // scalar: the loop bounds and the row clamp depend on it
  kv_len = kv_len < cap_rows ? kv_len : cap_rows;
  const uint32_t n_ch = (kv_len + CH - 1) / CH, last = kv_len - 1;

  // byte offsets inside the kv head (< cap_rows * D * 4 <= 2^23): scalar base + 32-bit lane offset
  const char* const kbase = reinterpret_cast<const char*>(kc + (size_t)kvh * max_seq * D);
  const char* const vbase = reinterpret_cast<const char*>(vc + (size_t)kvh * max_seq * D);
  const uint32_t krow0 = wave * 8 + ksub, vrow0 = wave * RPW + vsub;
  auto k_has = [&](uint32_t c) { return c * CH + wave * 8 < kv_len; };                         // wave-uniform
  // (the requests are unconditional, so that the waits in front of their uses are counted exactly: a row group wholly past the end
  // asks for the last row in every lane, one cache line per instruction)
  auto load_k = [&](f32x4 (&k)[NB], uint32_t c) {
    const uint32_t r = c * CH + krow0, off = (r < last ? r : last) * (D * 4) + kl * 16;
#pragma unroll
    for (int j = 0; j < NB; j++) k[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(kbase + off + j * 128));
  };
  auto load_v = [&](f32x4 (&v)[NB], uint32_t c) {
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const uint32_t r = c * CH + j * (NW * RPW) + vrow0, off = (r < last ? r : last) * (D * 4) + li * 16;
      v[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vbase + off));
    }
  };
  // a long context's K chunk kch or, up to 256 rows, V chunk vch: picked by address, not by a branch (a branch around requests makes
  // every wait behind it count for its worse side)
  const bool longc = n_ch > 2;
  auto load_k_or_v = [&](f32x4 (&b)[NB], uint32_t kch, uint32_t vch) {
    const char* const base = longc ? kbase : vbase;
    const uint32_t rk = kch * CH + krow0, offk = (rk < last ? rk : last) * (D * 4) + kl * 16;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const uint32_t rv = vch * CH + j * (NW * RPW) + vrow0, offv = (rv < last ? rv : last) * (D * 4) + li * 16;
      b[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + (longc ? offk + j * 128 : offv)));
    }
  };
  f32x4 buf[4][NB];
  load_k(buf[0], 0);
  load_k(buf[1], 1);
  // the query takes the scale here, behind the first requests: every later wait then stands behind the query's arrival on every path
#pragma unroll
  for (int j = 0; j < NB; j++) qv[j] = qv[j] * scale;

  // ---- 1. scores
  auto score = [&](const f32x4 (&k)[NB], uint32_t c) {
    if (!k_has(c)) return;
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
  load_k_or_v(buf[2], 2, 0);
  load_k_or_v(buf[3], 3, 1);
  uint32_t c = 0;
  for (; c + 4 < n_ch; c += 4) {
#pragma unroll
    for (int i = 0; i < 4; i++) { score(buf[i], c + i); load_k(buf[i], c + 4 + i); }
  }
  score(buf[0], c);
  score(buf[1], c + 1);
  if (longc) {   // the last group: V 0..3 take the buffers, in the order the V loop consumes them (2, 3, 0, 1)
    score(buf[2], c + 2);
    load_v(buf[2], 0);
    score(buf[3], c + 3);
    load_v(buf[3], 1);
    load_v(buf[0], 2);
    load_v(buf[1], 3);
  }
  __syncthreads();

  // ---- 2. the head's maximum (every wave for itself), then p and its sum, each row once
  float mx = kNegBig;
  for (uint32_t b = 0; b < kv_len; b += 64) {
    const uint32_t r = b + lane;
    const float s = s_sc[r < last ? r : last];
    mx = s > mx ? s : mx;   // (finite scores: no need for fmaxf's NaN rules)
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

  // ---- 3. out = sum_r p_r V[r]
  f32x4 acc = (f32x4)(0.0f);
  auto accum = [&](const f32x4 (&v)[NB], uint32_t c) {
    if (c >= n_ch) return;   // (s_p ends with the last chunk that has a visible row; in it rows past the end have p = 0)
    float p[NB];
#pragma unroll
    for (int j = 0; j < NB; j++) p[j] = s_p[c * CH + j * (NW * RPW) + vrow0];
#pragma unroll
    for (int j = 0; j < NB; j++) {
      acc.x = __builtin_fmaf(p[j], v[j].x, acc.x); acc.y = __builtin_fmaf(p[j], v[j].y, acc.y);
      acc.z = __builtin_fmaf(p[j], v[j].z, acc.z); acc.w = __builtin_fmaf(p[j], v[j].w, acc.w);
    }
  };
  for (c = 0; c + 4 < n_ch; c += 4) {
#pragma unroll
    for (int i = 0; i < 4; i++) { accum(buf[(i + 2) & 3], c + i); load_v(buf[(i + 2) & 3], c + 4 + i); }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) accum(buf[(i + 2) & 3], c + i);

  // ---- 4. row slots, then waves: additions in a fixed order
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
    acc.x += __shfl_xor(acc.x, off, 64); acc.y += __shfl_xor(acc.y, off, 64);
    acc.z += __shfl_xor(acc.z, off, 64); acc.w += __shfl_xor(acc.w, off, 64);
  }
  if (vsub == 0) *reinterpret_cast<f32x4*>(&s_acc[wave * D + li * 4]) = acc;
  __syncthreads();
  if (threadIdx.x < (uint32_t)D) {   // whole waves
    const uint32_t dim = threadIdx.x;
    float o = s_acc[dim], sum = s_sum[0];
#pragma unroll
    for (int w = 1; w < NW; w++) { o += s_acc[w * D + dim]; sum += s_sum[w]; }
    o = o * (1.0f / sum);   // simd.rs:718-720: multiply by 1/sum
    out[(size_t)head * D + dim] = o;
    if (xq_out) xq_store_chunk(xq_out, (head * D + dim) >> 4, o);   // wo's input as XQ records
  }
  LGH_TL_END();
}

// ------------------------------------------------------------------------------------------------
// int8 KV cache (LGH_FLAG_KV_INT8): the reference's QuantizedKVCache with KVCacheFormat::Int8
// (src/model/kv_quantized.rs:143-300, 385-410).  Per layer K and V are int8 [kv_head][max_seq][D] plus one f32 scale per
// (kv_head, position): scale = max|x| / 127 (1 for an all-zero row), q = round(x / scale) clamped, and attention reads
// back scale * q.  The QKV launch leaves the current token's rows as f32 in a staging vector; every attention workgroup of
// a kv head quantizes that row itself (D values, the same bits everywhere), split 0 also stores it into the cache, and the
// row takes part in the softmax through its dequantized values — exactly what a later token will read.
// The split / online-softmax structure is attn_partial_kernel's (attn_split.h); a row is D bytes (one dword per lane).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 unpack_i8x4(uint32_t w, float scale) {
  f32x4 r;
  r.x = (float)(int)(int8_t)(w & 0xFFu) * scale;
  r.y = (float)(int)(int8_t)((w >> 8) & 0xFFu) * scale;
  r.z = (float)(int)(int8_t)((w >> 16) & 0xFFu) * scale;
  r.w = (float)(int)(int8_t)(w >> 24) * scale;
  return r;
}

// quantize_int8: the scale of a row whose largest magnitude is amax, and one value's byte
__device__ __forceinline__ float i8_row_scale(float amax) { return amax > 1e-10f ? amax / 127.0f : 1.0f; }
__device__ __forceinline__ uint32_t i8_quantize(float v, float scale) {
  float r = roundf(v / scale);                           // f32::round: halves away from zero
  r = r < -128.0f ? -128.0f : (r > 127.0f ? 127.0f : r);
  return (uint32_t)(int)r & 0xFFu;
}

// quantizes the f32 row held 4 elements per lane by the LPR lanes of a row group; returns the packed int8 word and the scale
template <int LPR>
__device__ __forceinline__ uint32_t quantize_row_i8(f32x4 x, float& scale) {
  float amax = fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w)));
  amax = fmaxf(amax, dpp_f<0xB1>(amax));
  amax = fmaxf(amax, dpp_f<0x4E>(amax));
  amax = fmaxf(amax, dpp_f<0x141>(amax));
  amax = fmaxf(amax, dpp_f<0x140>(amax));
  if (LPR == 32) amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
  scale = i8_row_scale(amax);
  return i8_quantize(x.x, scale) | i8_quantize(x.y, scale) << 8 | i8_quantize(x.z, scale) << 16 | i8_quantize(x.w, scale) << 24;
}

// ---- the reference's FP8 KV formats (kv_quantized.rs:413-565; FMT 2 = E4M3, 3 = E5M2): one byte per element, no scales ----
// dequantize_fp8_*: case by case it is the standard decode of the format (E4M3 without infinities, 0x7F / 0xFF = NaN), except
// that both zeros read back as +0.  E5M2 is the upper byte of an IEEE half.
template <int FMT>
__device__ __forceinline__ float fp8_decode(uint32_t b) {
  const uint32_t mag = b & 0x7Fu;
  if (mag == 0) return 0.0f;
  if (FMT == 3) return (float)__builtin_bit_cast(_Float16, (uint16_t)(b << 8));
  if (mag == 0x7Fu) return __uint_as_float(0x7FC00000u);
  const uint32_t e = mag >> 3, mt = mag & 7u;
  const float v = e ? __uint_as_float((e + 120u) << 23 | mt << 20) : (float)mt * 0x1p-9f;
  return __uint_as_float(__float_as_uint(v) | (b & 0x80u) << 24);
}
// quantize_fp8_e4m3 / _e5m2 as written in the reference: the mantissa is truncated, magnitudes past the largest exponent
// saturate to 0x7E / 0x7C, and an E4M3 magnitude in [480, 512) becomes the NaN pattern 0x7F
template <int FMT>
__device__ __forceinline__ uint32_t fp8_encode(float value) {
  constexpr bool e4 = FMT == 2;
  const uint32_t bits = __float_as_uint(value);
  const uint32_t sign = (bits >> 31) << 7;
  if (value != value) return 0xFFu;
  if ((bits & 0x7FFFFFFFu) == 0x7F800000u) return e4 ? (sign ? 0xFFu : 0x7Fu) : (sign ? 0xFCu : 0x7Cu);
  if (value == 0.0f) return 0x00u;
  const int exponent = (int)((bits >> 23) & 0xFFu) - 127;
  uint32_t mantissa = bits & 0x7FFFFFu;
  if (exponent != -127) mantissa |= 0x800000u;
  if (e4) {
    const int e = exponent + 7;
    if (e > 15) return sign | 0x7Eu;
    if (e > -3 && e <= 0) return sign | ((mantissa >> (24 - (uint32_t)(3 + e))) & (0x7u >> (uint32_t)(-e)));
    if (e <= -3) return sign;
    return sign | (uint32_t)e << 3 | ((mantissa >> 20) & 0x7u);
  }
  const int e = exponent + 15;
  if (e > 31) return sign | 0x7Cu;
  if (e >= -1 && e <= 0) return sign | ((mantissa >> (24 - (uint32_t)(2 + e))) & (0x3u >> (uint32_t)(-e)));
  if (e < -1) return sign;
  return sign | (uint32_t)e << 2 | ((mantissa >> 21) & 0x3u);
}
// four cached values of one dword, any byte format (FMT 1 = int8 with the row's scale)
template <int FMT>
__device__ __forceinline__ f32x4 unpack_kv4(uint32_t w, float scale) {
  if (FMT == 1) return unpack_i8x4(w, scale);
  f32x4 r;
  r.x = fp8_decode<FMT>(w & 0xFFu); r.y = fp8_decode<FMT>((w >> 8) & 0xFFu);
  r.z = fp8_decode<FMT>((w >> 16) & 0xFFu); r.w = fp8_decode<FMT>(w >> 24);
  return r;
}

// MULTI (multi-sequence decode, engine_batch.hip): blockIdx.y = sequence s of the step; its query is q + s * n_heads * D, its position
// pos_ptr[s], its cache the slot slot[s] of [slot][kv_head][max_seq][D] bytes (and [slot][kv_head][max_seq] scales), its staged rows
// k_new / v_new + s * x_stride, its partials the s-th block of part_ml / part_acc.  Per sequence the arithmetic is the single-sequence
// kernel's (same NW, same split strides, same merges): the outputs are bit-identical.
template <int D, int G, int NW, int FMT, bool MULTI = false>
__global__ void __launch_bounds__(NW * 64) attn_partial_q8_kernel(const float* __restrict__ q, int8_t* __restrict__ k8, int8_t* __restrict__ v8,
                                                                  float* __restrict__ kscale, float* __restrict__ vscale,
                                                                  const float* __restrict__ k_new, const float* __restrict__ v_new,
                                                                  uint32_t max_seq, float scale, const int* pos_ptr, uint32_t n_splits,
                                                                  float* __restrict__ part_ml, float* __restrict__ part_acc,
                                                                  const int* __restrict__ slot = nullptr, uint32_t x_stride = 0) {
  constexpr int LPR = D / 4, RPW = 64 / LPR;
  __shared__ float s_ml[NW * G * 2];
  __shared__ __attribute__((aligned(16))) float s_acc[NW * G * D];
  const uint32_t kvh = blockIdx.x / n_splits, sp = blockIdx.x % n_splits;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t sub = lane / LPR, li = lane % LPR;
  uint32_t pw, sl = 0;
  if (MULTI) {
    const uint32_t sq = blockIdx.y, n_kv = gridDim.x / n_splits;
    sload_u32x2(pos_ptr + sq, slot + sq, pw, sl);
    q += (size_t)sq * n_kv * G * D;
    k_new += (size_t)sq * x_stride;
    v_new += (size_t)sq * x_stride;
    part_ml += (size_t)sq * gridDim.x * G * 2;
    part_acc += (size_t)sq * gridDim.x * G * D;
    sl *= n_kv;   // the slot's first kv head, in heads
  } else {
    pw = sload_u32(pos_ptr);
  }
  const uint32_t pos = pw;   // rows [0, pos) come from the cache, row `pos` from the staging vectors
  f32x4 qv[G];
#pragma unroll
  for (int g = 0; g < G; g++) qv[g] = *reinterpret_cast<const f32x4*>(q + ((size_t)kvh * G + g) * D + li * 4);
  float m[G], l[G];
  f32x4 acc[G];
#pragma unroll
  for (int g = 0; g < G; g++) { m[g] = kNegBig; l[g] = 0.0f; acc[g] = (f32x4)(0.0f); }
  auto step = [&](bool valid, f32x4 k4, f32x4 v4) { attn_step4<G, LPR>(qv, k4, v4, scale, valid, m, l, acc); };
  const size_t hrow = MULTI ? ((size_t)sl + kvh) * max_seq : (size_t)kvh * max_seq;   // first row of this kv head (of this slot)
  const uint32_t stride = n_splits * NW * RPW;
  constexpr int kAhead = 4;
  for (uint32_t base = (sp * NW + wave) * RPW; base < pos; base += kAhead * stride) {
    uint32_t kk[kAhead], vv[kAhead];
    float ks[kAhead], vs[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; j++) {
      const uint32_t p = base + j * stride + sub, r = p < pos ? p : pos - 1;
      kk[j] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(k8 + (hrow + r) * D + li * 4));
      vv[j] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(v8 + (hrow + r) * D + li * 4));
      ks[j] = FMT == 1 ? kscale[hrow + r] : 1.0f;
      vs[j] = FMT == 1 ? vscale[hrow + r] : 1.0f;
    }
#pragma unroll
    for (int j = 0; j < kAhead; j++)
      if (base + j * stride < pos) step(base + j * stride + sub < pos, unpack_kv4<FMT>(kk[j], ks[j]), unpack_kv4<FMT>(vv[j], vs[j]));
  }
  if (wave == 0) {   // the current token's row: quantized here (every split the same bits), stored by split 0
    const f32x4 kx = *reinterpret_cast<const f32x4*>(k_new + (size_t)kvh * D + li * 4);
    const f32x4 vx = *reinterpret_cast<const f32x4*>(v_new + (size_t)kvh * D + li * 4);
    float ksc = 1.0f, vsc = 1.0f;
    uint32_t kq, vq;
    if (FMT == 1) {
      kq = quantize_row_i8<LPR>(kx, ksc);
      vq = quantize_row_i8<LPR>(vx, vsc);
    } else {
      kq = fp8_encode<FMT>(kx.x) | fp8_encode<FMT>(kx.y) << 8 | fp8_encode<FMT>(kx.z) << 16 | fp8_encode<FMT>(kx.w) << 24;
      vq = fp8_encode<FMT>(vx.x) | fp8_encode<FMT>(vx.y) << 8 | fp8_encode<FMT>(vx.z) << 16 | fp8_encode<FMT>(vx.w) << 24;
    }
    if (sp == 0) {
      if (sub == 0) {
        *reinterpret_cast<uint32_t*>(k8 + (hrow + pos) * D + li * 4) = kq;
        *reinterpret_cast<uint32_t*>(v8 + (hrow + pos) * D + li * 4) = vq;
        if (FMT == 1 && li == 0) { kscale[hrow + pos] = ksc; vscale[hrow + pos] = vsc; }
      }
      step(sub == 0, unpack_kv4<FMT>(kq, ksc), unpack_kv4<FMT>(vq, vsc));
    }
  }
  attn_merge_rows<G, LPR>(m, l, acc);
  // (attn_stash spelled out: through the shared function attn_partial_q8_kernel<64, 8, 4, 1, true> takes 130 VGPRs instead of 127 and
  // loses a wave of occupancy, 4 -> 3)
  if (sub == 0) {
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (li == 0) { s_ml[(wave * G + g) * 2] = m[g]; s_ml[(wave * G + g) * 2 + 1] = l[g]; }
      *reinterpret_cast<f32x4*>(&s_acc[((size_t)wave * G + g) * D + li * 4]) = acc[g];
    }
  }
  __syncthreads();
  attn_merge_store<NW, G, D>(s_ml, s_acc, part_ml, part_acc, ((size_t)kvh * n_splits + sp) * G);
}

// n_seq 0: the single-sequence launch; else grid y = the sequences of a step over cache slots (engine_batch.hip).  NW = 4 whatever
// max_seq is, for both: with another wave count the rows would be dealt differently and the sums would differ in their last bits.
// Caches [slot][n_kv][max_seq][D] bytes, scales (int8) [slot][n_kv][max_seq]; sequence s's staged (K row | V row) pair x_stride floats on.
template <int D, int G, int FMT>
static hipError_t attn_q8_go(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  const float *k_new = a.kv_new, *v_new = a.kv_new + (size_t)l.n_kv * D;
  const uint32_t x_stride = 2 * l.n_kv * D;
  const dim3 grid(l.n_kv * a.n_splits, a.n_seq ? a.n_seq : 1);
  if (a.n_seq)
    hipLaunchKernelGGL((attn_partial_q8_kernel<D, G, 4, FMT, true>), grid, dim3(256), 0, a.st, a.q, kv.k_i8(), kv.v_i8(), kv.kscale(), kv.vscale(), k_new,
                       v_new, l.max_seq, a.scale, a.pos, a.n_splits, a.part_ml, a.part_acc, a.slot, x_stride);
  else
    hipLaunchKernelGGL((attn_partial_q8_kernel<D, G, 4, FMT>), grid, dim3(256), 0, a.st, a.q, kv.k_i8(), kv.v_i8(), kv.kscale(), kv.vscale(), k_new,
                       v_new, l.max_seq, a.scale, a.pos, a.n_splits, a.part_ml, a.part_acc);
  return hipGetLastError();
}

// FMT: the layout's type (1 = int8 + scales, 2 = FP8 E4M3, 3 = FP8 E5M2; the scale arrays are unused for 2 and 3)
static hipError_t attn_q8_dispatch(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  return attn_dispatch(l.d, a.n_heads / l.n_kv, [&](auto d, auto gg) {
    constexpr int D = decltype(d)::value, G = decltype(gg)::value;
    if (l.type == LGH_KV_INT8) return attn_q8_go<D, G, 1>(l, kv, a);
    if (l.type == LGH_KV_FP8_E4M3) return attn_q8_go<D, G, 2>(l, kv, a);
    if (l.type == LGH_KV_FP8_E5M2) return attn_q8_go<D, G, 3>(l, kv, a);
    return hipErrorInvalidValue;
  });
}

// one row of n values through a byte KV format and back (the quantizers of attn_partial_q8_kernel, stand-alone): bytes and,
// for int8, the row's scale; `back` = what attention would read
template <int FMT>
__global__ void __launch_bounds__(64) kv_roundtrip_kernel(const float* __restrict__ x, uint32_t n, uint8_t* __restrict__ bytes,
                                                          float* __restrict__ scale_out, float* __restrict__ back) {
  const uint32_t lane = threadIdx.x;
  float scale = 1.0f;
  if (FMT == 1) {   // quantize_int8: one scale per row
    float amax = 0.0f;
    for (uint32_t i = lane; i < n; i += 64) amax = fmaxf(amax, fabsf(x[i]));
    amax = wave_max(amax);
    scale = i8_row_scale(amax);
    if (lane == 0) *scale_out = scale;
  }
  for (uint32_t i = lane; i < n; i += 64) {
    uint32_t b;
    if (FMT == 1) {
      b = i8_quantize(x[i], scale);
      back[i] = (float)(int)(int8_t)b * scale;
    } else {
      b = fp8_encode<FMT>(x[i]);
      back[i] = fp8_decode<FMT>(b);
    }
    bytes[i] = (uint8_t)b;
  }
}

hipError_t kv_roundtrip_launch(int fmt, const float* x, uint32_t n, uint8_t* bytes, float* scale_out, float* back, hipStream_t st) {
  if (fmt == 1) hipLaunchKernelGGL(kv_roundtrip_kernel<1>, dim3(1), dim3(64), 0, st, x, n, bytes, scale_out, back);
  else if (fmt == 2) hipLaunchKernelGGL(kv_roundtrip_kernel<2>, dim3(1), dim3(64), 0, st, x, n, bytes, scale_out, back);
  else if (fmt == 3) hipLaunchKernelGGL(kv_roundtrip_kernel<3>, dim3(1), dim3(64), 0, st, x, n, bytes, scale_out, back);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// The batched prompt pass over a byte cache (engine_prefill.hip): the block's m K rows after RoPE and V rows, f32 [kv head][src_rows][D]
// (row r of a head = position pos0 + r), into rows pos0 .. pos0+m-1 of the cache's byte tensors and, for int8, of its scale tensors.
// LPR = D / 4 lanes hold a row, 4 elements each (one 16-byte load, one dword store), and quantize it with attn_partial_q8_kernel's own
// functions: the bytes and scales are the ones the decode launch would have stored for the same f32 row.  grid = (row groups, kv
// heads, K | V); no LDS.
template <int D, int FMT>
__global__ void __launch_bounds__(256) kv8_pf_store_kernel(const float* __restrict__ krows, const float* __restrict__ vrows, uint32_t src_rows,
                                                           uint32_t m, uint32_t pos0, uint32_t max_seq, uint8_t* __restrict__ k8,
                                                           uint8_t* __restrict__ v8, float* __restrict__ kscale, float* __restrict__ vscale) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const uint32_t kvh = blockIdx.y, isv = blockIdx.z;
  const uint32_t sub = threadIdx.x / LPR, li = threadIdx.x % LPR;
  const uint32_t r = blockIdx.x * RPB + sub, rr = r < m ? r : m - 1;   // (whole row groups stay active for the row maximum)
  const f32x4 x = *reinterpret_cast<const f32x4*>((isv ? vrows : krows) + ((size_t)kvh * src_rows + rr) * D + li * 4);
  float sc = 1.0f;
  uint32_t w;
  if (FMT == 1) w = quantize_row_i8<LPR>(x, sc);
  else w = fp8_encode<FMT>(x.x) | fp8_encode<FMT>(x.y) << 8 | fp8_encode<FMT>(x.z) << 16 | fp8_encode<FMT>(x.w) << 24;
  if (r >= m) return;
  const size_t row = (size_t)kvh * max_seq + pos0 + r;
  *reinterpret_cast<uint32_t*>((isv ? v8 : k8) + row * D + li * 4) = w;
  if (FMT == 1 && li == 0) (isv ? vscale : kscale)[row] = sc;
}

template <int D, int FMT>
static hipError_t kv8_pf_store_go(const float* krows, const float* vrows, uint32_t src_rows, const KvCache& kv, uint32_t n_kv, uint32_t max_seq,
                                  uint32_t pos0, uint32_t m, hipStream_t st) {
  constexpr uint32_t RPB = 256 / (D / 4);
  hipLaunchKernelGGL((kv8_pf_store_kernel<D, FMT>), dim3((m + RPB - 1) / RPB, n_kv, 2), dim3(256), 0, st, krows, vrows, src_rows, m, pos0, max_seq,
                     kv.k_bytes(), kv.v_bytes(), kv.kscale(), kv.vscale());
  return hipGetLastError();
}

// type: LGH_KV_INT8 / LGH_KV_FP8_E4M3 / LGH_KV_FP8_E5M2 (= FMT 1 / 2 / 3); head_dim 64 or 128; rows pos0 .. pos0+m-1 must lie in the cache
hipError_t kv8_pf_store_launch(uint32_t type, const float* krows, const float* vrows, uint32_t src_rows, const KvCache& kv, uint32_t n_kv,
                               uint32_t head_dim, uint32_t max_seq, uint32_t pos0, uint32_t m, hipStream_t st) {
  if (type < LGH_KV_INT8 || type > LGH_KV_FP8_E5M2 || (head_dim != 64 && head_dim != 128) || n_kv == 0 || m == 0 || m > src_rows ||
      (uint64_t)pos0 + m > max_seq)
    return hipErrorInvalidValue;
  auto go = [&](auto d) {
    constexpr int D = decltype(d)::value;
    return type == LGH_KV_INT8       ? kv8_pf_store_go<D, 1>(krows, vrows, src_rows, kv, n_kv, max_seq, pos0, m, st)
           : type == LGH_KV_FP8_E4M3 ? kv8_pf_store_go<D, 2>(krows, vrows, src_rows, kv, n_kv, max_seq, pos0, m, st)
                                     : kv8_pf_store_go<D, 3>(krows, vrows, src_rows, kv, n_kv, max_seq, pos0, m, st);
  };
  return head_dim == 128 ? go(std::integral_constant<int, 128>{}) : go(std::integral_constant<int, 64>{});
}

// out[h][dim] = the merge of head h's splits (attn_split.h: attn_combine_splits), and wo's input as XQ records
template <bool MULTI>
__global__ void __launch_bounds__(128) attn_combine_kernel(const float* __restrict__ part_ml, const float* __restrict__ part_acc,
                                                           uint32_t g_per_kv, uint32_t head_dim, uint32_t n_splits,
                                                           float* __restrict__ out, uint8_t* __restrict__ xq_out) {
  __shared__ float s_f[64];
  __shared__ float s_linv;
  LGH_TL_BEGIN(attn, lgh::TL_COMBINE, n_splits);
  if (MULTI) {   // blockIdx.y = sequence: its partials, its output vector and XQ image
    const uint32_t sq = blockIdx.y, n_heads = gridDim.x;
    part_ml += (size_t)sq * n_heads * n_splits * 2;
    part_acc += (size_t)sq * n_heads * n_splits * head_dim;
    out += (size_t)sq * n_heads * head_dim;
    if (xq_out) xq_out += (size_t)sq * xq_bytes((size_t)n_heads * head_dim);
  }
  const uint32_t h = blockIdx.x, kvh = h / g_per_kv, g = h % g_per_kv;
  const size_t p0 = (size_t)kvh * n_splits * g_per_kv + g;   // split s lives at p0 + s * g_per_kv
  const uint32_t dim = threadIdx.x;   // one dim per thread: blockDim >= head_dim
  const float o = attn_combine_splits(part_ml, part_acc, p0, g_per_kv, head_dim, n_splits, dim, dim < head_dim, s_f, &s_linv);
  if (dim < head_dim) {
    out[(size_t)h * head_dim + dim] = o;
    if (xq_out) xq_store_chunk(xq_out, (h * head_dim + dim) >> 4, o);   // wo's input as XQ records (head_dim % 16 == 0)
  }
  LGH_TL_END();
}

// n_seq 0: the single-sequence launch; else grid y = the sequences of a step over cache slots (engine_batch.hip).  The wave count
// follows the cache capacity alone, so a sequence's rows are dealt the same way in both and its partials are the same bits.
template <int D, int G, int NW>
static hipError_t attn_go(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  const dim3 grid(l.n_kv * a.n_splits, a.n_seq ? a.n_seq : 1);
  if (a.n_seq)
    hipLaunchKernelGGL((attn_partial_kernel<D, G, NW, false, false, true>), grid, dim3(NW * 64), 0, a.st, a.q, kv.k_f32(), kv.v_f32(), l.max_seq, a.scale,
                       a.pos, 0, a.n_splits, a.part_ml, a.part_acc, a.slot, l.stride_floats());
  else
    hipLaunchKernelGGL((attn_partial_kernel<D, G, NW>), grid, dim3(NW * 64), 0, a.st, a.q, kv.k_f32(), kv.v_f32(), l.max_seq, a.scale, a.pos,
                       a.kv_len_fixed, a.n_splits, a.part_ml, a.part_acc);
  return hipGetLastError();
}

static hipError_t attn_f32_dispatch(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  const bool long_ctx = (a.pos ? l.max_seq : (uint32_t)a.kv_len_fixed) >= 2048;
  return attn_dispatch(l.d, a.n_heads / l.n_kv, [&](auto d, auto gg) {
    constexpr int D = decltype(d)::value, G = decltype(gg)::value;
    return long_ctx ? attn_go<D, G, 8>(l, kv, a) : attn_go<D, G, 4>(l, kv, a);
  });
}

// What both launches of a split step ask of its description, whatever the format
static bool attn_decode_ok(const KvLayout& l, const AttnDecode& a) {
  return l.n_kv != 0 && a.n_heads % l.n_kv == 0 && a.n_splits >= 1 && a.n_splits <= 32 && (a.pos || (l.f32() && !a.n_seq && a.kv_len_fixed > 0)) &&
         (a.n_seq == 0 || a.slot) && (!l.tq() || a.signs);
}

hipError_t attn_tq_split_launch(const KvLayout& l, const KvCache& kv, const AttnDecode& a);   // attention_tq.hip
hipError_t attn_tq_merge_launch(const KvLayout& l, const AttnDecode& a);

hipError_t attn_split_launch(const KvLayout& l, const KvCache& kv, const AttnDecode& a) {
  if (!attn_decode_ok(l, a) || (l.staged() && !a.kv_new) || (l.has_scales() && (!kv.kscale() || !kv.vscale())) || (a.qjl_s != nullptr) != (kv.kx() != nullptr))
    return hipErrorInvalidValue;
  return l.tq() ? attn_tq_split_launch(l, kv, a) : l.staged() ? attn_q8_dispatch(l, kv, a) : attn_f32_dispatch(l, kv, a);
}

// single-launch decode attention for short contexts (engine.hip picks it by the host-side position)
hipError_t attn_direct_launch(const float* q, const float* kcache, const float* vcache, uint32_t n_heads, uint32_t n_kv, uint32_t head_dim,
                              uint32_t max_seq, float scale, const int* pos, float* out, uint8_t* xq_out, hipStream_t st) {
  if (n_kv == 0 || n_heads % n_kv || !pos) return hipErrorInvalidValue;
  return attn_dispatch(head_dim, n_heads / n_kv, [&](auto d, auto gg) {
    hipLaunchKernelGGL((attn_partial_kernel<decltype(d)::value, decltype(gg)::value, 16, false, true>), dim3(n_kv), dim3(1024), 0, st, q, kcache, vcache,
                       max_seq, scale, pos, 0, 1u, reinterpret_cast<float*>(xq_out), out);
    return hipGetLastError();
  });
}

template <int D, int G>
static hipError_t attn_head_go(const float* q, const float* kc, const float* vc, uint32_t n_kv, uint32_t max_seq, float scale, const int* pos,
                               uint32_t cap_rows, float* out, uint8_t* xq_out, hipStream_t st) {
  auto lds = [](uint32_t rows) { return (size_t)(2 * rows + 16 * D + 16) * 4; };
  static bool attr_set[64] = {};
  if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(&attn_head_kernel<D, G>), (int)lds(kAttnHeadMaxRows), attr_set); e != hipSuccess) return e;
  hipLaunchKernelGGL((attn_head_kernel<D, G>), dim3(n_kv, G), dim3(1024), lds(cap_rows), st, q, kc, vc, pos, out, xq_out, max_seq, scale, cap_rows);
  return hipGetLastError();
}

// single-launch decode attention, one workgroup per query head (engine.hip picks it by the host-side position).  The position word
// must not exceed min(max_seq, max_rows) - 1: the kernel keeps a head's scores in LDS and attends to no row past that capacity.
hipError_t attn_head_launch(const float* q, const float* kcache, const float* vcache, uint32_t n_heads, uint32_t n_kv, uint32_t head_dim,
                            uint32_t max_seq, float scale, const int* pos, uint32_t max_rows, float* out, uint8_t* xq_out, hipStream_t st) {
  if (n_kv == 0 || n_heads % n_kv || !pos || max_rows == 0 || max_seq == 0) return hipErrorInvalidValue;
  const uint32_t rows = max_rows < max_seq ? max_rows : max_seq;
  if (rows > kAttnHeadMaxRows) return hipErrorInvalidValue;
  const uint32_t cap_rows = (rows + 127) / 128 * 128;
  return attn_dispatch(head_dim, n_heads / n_kv, [&](auto d, auto gg) {
    return attn_head_go<decltype(d)::value, decltype(gg)::value>(q, kcache, vcache, n_kv, max_seq, scale, pos, cap_rows, out, xq_out, st);
  });
}

// ------------------------------------------------------------------------------------------------
// Causal attention of a block of prompt tokens on the matrix cores, in f32 (v_mfma_f32_16x16x4_f32: exact f32 products,
// f32 accumulation — no f16 rounding enters here).  A workgroup = one query head x 16 tokens; its 4 waves take the kv tiles
// (16 cached rows each) round-robin, each with its own online-softmax state, merged through LDS at the end.
// Per kv tile a wave computes S^T = K Q^T (M = kv row, N = token; the contraction runs over d, lane group c owning the
// D/4 contiguous dims [c D/4, (c+1) D/4) of both operands, so K and Q fragments are plain 16-byte loads) and then
// O^T += V^T P^T: the D layout of S^T gives lane (token n, group c) the four kv rows 4c..4c+3 of token n, which is exactly
// the B operand of four MFMAs whose contraction index c stands for kv row 4c+i — the probabilities never leave their
// registers.  The A operand of those is V^T with output row m standing for dims D/16 m .. D/16 m + D/16 - 1 (contiguous
// loads again).  The VALU kernel this replaces (still taken by other head sizes; LGH_PF_ATTN_VALU=1 forces it) spent 17 us per
// layer of a 128-token Llama-3-8B prompt, bound by vector issue (four workgroups of four waves per CU); this one 10.7 us
// (8 waves, the next tile's fragments in flight during a tile; 11.7 us with 4 waves), and the 512-token prompt 19.0 instead
// of 21.8 ms.
// TQ (the prompt pass over a TurboQuantMSE cache, attention_tq.hip tq_pf_rows_kernel): q holds rotated queries and kc / vc the rows'
// centroids in the rotated space, so the scores are the reference's and the merged accumulator is sum_p w_p c[V_p] in the rotated
// space; the epilogue inverts the rotation per (token, head) in f32 — attn_tq_combine_kernel's expression, with the V signs
// tq_signs [kv head][k, v][D] — and only then rounds to f16.
// ------------------------------------------------------------------------------------------------
struct PfTqEpi { const float* signs; float inv_scale, inv_d; };   // (unused without TQ)

// the f16 element (token t of the block, column col) of the XH matrix the wo GEMM reads
__device__ __forceinline__ void pf_xh_store(uint8_t* xh_out, uint32_t t, uint32_t col, float v) {
  *reinterpret_cast<_Float16*>(xh_out + xh_offset(t, col)) = (_Float16)v;
}

template <int D, int NW, bool TQ>
__global__ void __launch_bounds__(NW * 64) attn_pf_mfma_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ vc,
                                                               uint32_t n_heads, uint32_t g_per_kv, uint32_t max_seq, float scale, uint32_t pos0,
                                                               uint32_t m_tokens, uint8_t* __restrict__ xh_out, const PfTqEpi tq) {
  using Core = AttnBlockCore<D, NW>;
  constexpr int DJ = Core::DJ, DQ = Core::DQ;
  Core b(g_per_kv, pos0, m_tokens);
  const uint32_t n = b.n, c = b.c;
  float qf[DJ];
  b.load_q(qf, q, n_heads, m_tokens);
  const float* kbase = kc + (size_t)b.kvh * max_seq * D;
  const float* vbase = vc + (size_t)b.kvh * max_seq * D;
  float m_run = kNegBig, l_run = 0.0f;
  f32x4 acc[DQ];   // acc[x][i] = O^T[dim DQ (4c + i) + x][token n] of this wave's tiles
#pragma unroll
  for (int x = 0; x < DQ; x++) acc[x] = (f32x4)(0.0f);
  // a tile's K fragment (row kv0 + n, dims [c DJ, (c+1) DJ)) and V fragments (rows kv0 + 4c + i, dims [n DQ, (n+1) DQ))
  f32x4 kn[DJ / 4], vn[4][DQ / 4];
  auto load_tile = [&](uint32_t tile) {
    const uint32_t kv0 = tile * 16;
    const float* kp = kbase + (size_t)b.row(kv0 + n) * D + c * DJ;
#pragma unroll
    for (int j = 0; j < DJ / 4; j++) kn[j] = *reinterpret_cast<const f32x4*>(kp + 4 * j);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float* vp = vbase + (size_t)b.row(kv0 + 4 * c + i) * D + n * DQ;
#pragma unroll
      for (int x = 0; x < DQ / 4; x++) vn[i][x] = *reinterpret_cast<const f32x4*>(vp + 4 * x);
    }
  };
  if (b.wave < b.n_tiles) load_tile(b.wave);
  for (uint32_t tile = b.wave; tile < b.n_tiles; tile += NW) {
    f32x4 kf[DJ / 4], vf[4][DQ / 4];
#pragma unroll
    for (int j = 0; j < DJ / 4; j++) kf[j] = kn[j];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int x = 0; x < DQ / 4; x++) vf[i][x] = vn[i][x];
    if (tile + NW < b.n_tiles) load_tile(tile + NW);   // the next tile's fragments are in flight while this one is computed
    f32x4 st = (f32x4)(0.0f);
#pragma unroll
    for (int j = 0; j < DJ; j++) st = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j / 4][j % 4], qf[j], st, 0, 0, 0);
    float pv[4];
    b.update(st, tile * 16, pos0, scale, m_run, l_run, acc, pv);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int x = 0; x < DQ; x++) acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[i][x / 4][x % 4], pv[i], acc[x], 0, 0, 0);
  }
  b.stash(m_run, l_run, acc);
  if (!TQ) {
    b.merge(m_tokens, [&](uint32_t t, uint32_t dim, float o) { pf_xh_store(xh_out, b.tt * 16 + t, b.head * D + dim, o); });
  } else {
    // the merged value takes wave 0's place, x sqrt(d) as attn_tq_combine_kernel; then the inverse rotation (rotation.rs:80-96):
    // out = signs * (1 / d) * H (sqrt(d) * o), a wave per token, butterflies in registers
    b.merge(m_tokens, [&](uint32_t t, uint32_t dim, float o) { b.s_o[0][t][dim] = o * tq.inv_scale; });
    __syncthreads();
    const float* sv = tq.signs + (size_t)(b.kvh * 2 + 1) * D;
    const uint32_t lane = b.lane;
    for (uint32_t t = b.wave; t < 16u; t += NW) {
      if (b.tt * 16 + t >= m_tokens) continue;   // wave-uniform
      float x0 = b.s_o[0][t][lane], x1 = 0.0f;
      if (D == 128) x1 = b.s_o[0][t][lane + 64];
      tq_fwht_wave<D>(x0, x1, lane);
      pf_xh_store(xh_out, b.tt * 16 + t, b.head * D + lane, x0 * tq.inv_d * sv[lane]);
      if (D == 128) pf_xh_store(xh_out, b.tt * 16 + t, b.head * D + lane + 64, x1 * tq.inv_d * sv[lane + 64]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The block attention over a byte cache (int8 + scales, FP8 E4M3 / E5M2; FMT 1 / 2 / 3): the same core (attn_block.h) and f16
// store, with the cache's own bytes as the A operands.  Every token attends to the STORED rows, the block's own included
// (kv8_pf_store_kernel ran before), which is what the token-by-token engine and the reference attend to.  Lane (n, c) takes
// D/4 contiguous bytes of K row kv0 + n and D/16 contiguous bytes of each V row kv0 + 4c + i; the next tile travels as raw dwords
// (D = 128: 8 + 8, and 8 scales for int8) and is widened only once it is the current tile.  An int8 row's scale multiplies its score
// (K) and its probability (V), 8 multiplies per tile and lane, not its 64 elements.  FP8 bytes are widened by the hardware's OCP
// converters (v_cvt_pk_f32_fp8 / _bf8): they agree with fp8_decode on every code except that 0x80 reads as -0, which adds nothing
// to a dot product either way (tests/test_gpu_kv8_prefill.py runs every code through both operands).
// ------------------------------------------------------------------------------------------------
template <int FMT>
__device__ __forceinline__ f32x4 kv8_widen4(uint32_t w) {
  f32x4 r;
  if (FMT == 1) {
    r.x = (float)(int)(int8_t)(w & 0xFFu); r.y = (float)(int)(int8_t)((w >> 8) & 0xFFu);
    r.z = (float)(int)(int8_t)((w >> 16) & 0xFFu); r.w = (float)(int)(int8_t)(w >> 24);
  } else if (FMT == 2) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    r.x = lo[0]; r.y = lo[1]; r.z = hi[0]; r.w = hi[1];
  } else {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true);
    r.x = lo[0]; r.y = lo[1]; r.z = hi[0]; r.w = hi[1];
  }
  return r;
}

template <int D, int NW, int FMT>
__global__ void __launch_bounds__(NW * 64) attn_pf_kv8_kernel(const float* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                                              const float* __restrict__ ksc, const float* __restrict__ vsc, uint32_t n_heads,
                                                              uint32_t g_per_kv, uint32_t max_seq, float scale, uint32_t pos0, uint32_t m_tokens,
                                                              uint8_t* __restrict__ xh_out) {
  using Core = AttnBlockCore<D, NW>;
  constexpr int DJ = Core::DJ, DQ = Core::DQ;   // bytes of a K row, of a V row per lane
  constexpr int KW = DJ / 4, VW = DQ / 4;       // dwords of the K fragment, of one V row's fragment
  Core b(g_per_kv, pos0, m_tokens);
  const uint32_t n = b.n, c = b.c;
  float qf[DJ];
  b.load_q(qf, q, n_heads, m_tokens);
  const size_t hrow = (size_t)b.kvh * max_seq;   // first row of this kv head
  float m_run = kNegBig, l_run = 0.0f;
  f32x4 acc[DQ];   // acc[x][i] = O^T[dim DQ (4c + i) + x][token n] of this wave's tiles
#pragma unroll
  for (int x = 0; x < DQ; x++) acc[x] = (f32x4)(0.0f);
  // a tile's raw K fragment (row kv0 + n, bytes [c DJ, (c+1) DJ)), V fragments (rows kv0 + 4c + i, bytes [n DQ, (n+1) DQ)) and, int8,
  // the K and V scales of rows kv0 + 4c + i (the rows of this lane's scores)
  uint32_t kn[KW], vn[4][VW];
  float ksn[4], vsn[4];
  auto load_tile = [&](uint32_t tile) {
    const uint32_t kv0 = tile * 16;
    const uint8_t* kp = kc + (hrow + b.row(kv0 + n)) * D + c * DJ;
#pragma unroll
    for (int j = 0; j < KW; j += 4) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(kp + 4 * j);
      kn[j] = v.x; kn[j + 1] = v.y; kn[j + 2] = v.z; kn[j + 3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t vr = b.row(kv0 + 4 * c + i);
      const uint8_t* vp = vc + (hrow + vr) * D + n * DQ;
      if (VW == 2) {
        const u32x2 v = *reinterpret_cast<const u32x2*>(vp);
        vn[i][0] = v.x; vn[i][VW - 1] = v.y;
      } else {
        vn[i][0] = *reinterpret_cast<const uint32_t*>(vp);
      }
      if (FMT == 1) { ksn[i] = ksc[hrow + vr]; vsn[i] = vsc[hrow + vr]; }
    }
  };
  if (b.wave < b.n_tiles) load_tile(b.wave);
  for (uint32_t tile = b.wave; tile < b.n_tiles; tile += NW) {
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
    if (tile + NW < b.n_tiles) load_tile(tile + NW);   // the next tile's bytes are in flight while this one is computed
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
    b.update(st, tile * 16, pos0, scale, m_run, l_run, acc, pv);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float p = FMT == 1 ? pv[i] * vs[i] : pv[i];
#pragma unroll
      for (int x = 0; x < VW; x++) {
        const f32x4 v4 = kv8_widen4<FMT>(vf[i][x]);
#pragma unroll
        for (int e = 0; e < 4; e++) acc[4 * x + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(v4[e], p, acc[4 * x + e], 0, 0, 0);
      }
    }
  }
  b.stash(m_run, l_run, acc);
  b.merge(m_tokens, [&](uint32_t t, uint32_t dim, float o) { pf_xh_store(xh_out, b.tt * 16 + t, b.head * D + dim, o); });
}

// ---- host: the block attention's one launch (common.h: AttnBlock) ----
void tq_inverse_factors(uint32_t head_dim, float* inv_scale, float* inv_d);   // attention_tq.hip

// the LDS opt-in and the grid of whichever kernel was picked: n_heads x token tiles of NW waves
template <auto Kernel, int D, int NW, typename... Args>
static hipError_t attn_block_go(const AttnBlock& a, Args... args) {
  constexpr size_t lds = AttnBlockCore<D, NW>::kLdsBytes;
  static bool attr_set[64] = {};
  if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(Kernel), (int)lds, attr_set); e != hipSuccess) return e;
  hipLaunchKernelGGL(Kernel, dim3(a.n_heads, (a.m_tokens + 15) / 16), dim3(NW * 64), lds, a.st, args...);
  return hipGetLastError();
}

// (The formats in this order, f32's VALU fallback between f32 and TurboQuant, head_dim 128 before 64: kernels are emitted in the order
// of their first use, and the code object keeps the kernel order it was measured with — the launch-description note under profiles/)
hipError_t attn_block_launch(const KvLayout& l, const KvCache& kv, const AttnBlock& a) {
  if (l.type > LGH_KV_TQ3_QJL || l.n_kv == 0 || a.n_heads % l.n_kv || a.m_tokens == 0 || (uint64_t)a.pos0 + a.m_tokens > l.max_seq || l.qjl() ||
      (l.tq() && (!a.signs || !a.tq_kv)))
    return hipErrorInvalidValue;
  constexpr int NW = 8;   // (4 waves: 11.7 us per layer of a 128-token Llama-3-8B prompt, the last token tile's waves take two kv tiles each)
  const uint32_t g = a.n_heads / l.n_kv;
  const bool mfma_shape = l.d == 128 || l.d == 64;   // the matrix-core kernels' head sizes
  auto by_head_dim = [&](auto go) { return l.d == 128 ? go(std::integral_constant<int, 128>{}) : go(std::integral_constant<int, 64>{}); };
  if (l.f32()) {
    // (read once per process: tests/test_gpu_fresh_env.py::test_valu_prompt_attention holds the VALU kernel to test_prefill's bound)
    static const bool valu = [] { const char* e = std::getenv("LGH_PF_ATTN_VALU"); return e && std::atoi(e) != 0; }();   // (A/B switch: the VALU kernel)
    if (!valu && mfma_shape)
      return by_head_dim([&](auto d) {
        constexpr int D = decltype(d)::value;
        return attn_block_go<&attn_pf_mfma_kernel<D, NW, false>, D, NW>(a, a.q, kv.k_f32(), kv.v_f32(), a.n_heads, g, l.max_seq, a.scale, a.pos0, a.m_tokens,
                                                                        a.xh_out, PfTqEpi{});
      });
    // 4 waves per (kv head, token) workgroup: 8 and 16 waves measured slower on the 128-token Llama-3-8B prompt (4.79 / 5.07 vs
    // 4.74 ms per prompt pass) — the grid is already 1024 workgroups wide.
    return attn_dispatch(l.d, g, [&](auto d, auto gg) {
      hipLaunchKernelGGL((attn_partial_kernel<decltype(d)::value, decltype(gg)::value, 4, true>), dim3(l.n_kv, a.m_tokens), dim3(256), 0, a.st, a.q, kv.k_f32(),
                         kv.v_f32(), l.max_seq, a.scale, (const int*)nullptr, (int)(a.pos0 + 1), 1u, (float*)nullptr, reinterpret_cast<float*>(a.xh_out));
      return hipGetLastError();
    });
  }
  if (!mfma_shape) return hipErrorInvalidValue;
  if (l.tq())   // over the prompt pass's scratch (tq_pf_rows_launch filled it and rotated q)
    return by_head_dim([&](auto d) {
      constexpr int D = decltype(d)::value;
      PfTqEpi tq{a.signs, 0.0f, 0.0f};
      tq_inverse_factors(D, &tq.inv_scale, &tq.inv_d);
      return attn_block_go<&attn_pf_mfma_kernel<D, NW, true>, D, NW>(a, a.q, a.tq_kv, a.tq_kv + l.stride_floats(), a.n_heads, g, l.max_seq, a.scale, a.pos0,
                                                                     a.m_tokens, a.xh_out, tq);
    });
  return by_head_dim([&](auto d) {
    constexpr int D = decltype(d)::value;
    auto go = [&](auto fmt) {
      return attn_block_go<&attn_pf_kv8_kernel<D, NW, decltype(fmt)::value>, D, NW>(a, a.q, kv.k_bytes(), kv.v_bytes(), kv.kscale(), kv.vscale(), a.n_heads, g,
                                                                                    l.max_seq, a.scale, a.pos0, a.m_tokens, a.xh_out);
    };
    return l.type == LGH_KV_INT8       ? go(std::integral_constant<int, 1>{})
           : l.type == LGH_KV_FP8_E4M3 ? go(std::integral_constant<int, 2>{})
                                       : go(std::integral_constant<int, 3>{});
  });
}

// Attention of one query row for any head_dim (256 threads): scores of the `visible` rows in LDS (sc), the arithmetic of
// ops.rs:1353-1472 / 1479-1537 — sequential dot per score, max, exp, sum, weights times 1/sum, then V accumulated in position order.
__device__ __forceinline__ void attn_naive_row(const float* __restrict__ qv, const float* __restrict__ kb, const float* __restrict__ vb,
                                               float* __restrict__ out, uint32_t visible, uint32_t d, float scale, float* sc, float* s_red) {
  float m = -INFINITY;
  for (uint32_t p = threadIdx.x; p < visible; p += 256) {
    float dot = 0.0f;
    for (uint32_t i = 0; i < d; i++) dot += qv[i] * kb[(size_t)p * d + i];
    sc[p] = dot * scale;
    m = fmaxf(m, sc[p]);
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  __syncthreads();
  float sum = 0.0f;
  for (uint32_t p = threadIdx.x; p < visible; p += 256) {
    const float e = expf(sc[p] - m);
    sc[p] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = sum;
  __syncthreads();
  const float inv = 1.0f / ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
  for (uint32_t i = threadIdx.x; i < d; i += 256) {
    float o = 0.0f;
    for (uint32_t p = 0; p < visible; p++) o += (sc[p] * inv) * vb[(size_t)p * d + i];
    out[i] = o;
  }
}

// Backend::attention for any head_dim / group size (per-op surface only; the engine's shapes take the kernels above):
// one workgroup per (head, query position), causal
__global__ void __launch_bounds__(256) attn_generic_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                           float* __restrict__ out, uint32_t per_kv, uint32_t seq_len, uint32_t kv_len,
                                                           uint32_t kv_rows, uint32_t d, float scale) {
  extern __shared__ float sc[];
  __shared__ float s_red[4];
  const uint32_t head = blockIdx.x, s = blockIdx.y, kvh = head / per_kv;
  const uint32_t q_abs = (kv_len >= seq_len ? kv_len - seq_len : 0) + s;
  const uint32_t visible = q_abs + 1 < kv_len ? q_abs + 1 : kv_len;
  const size_t qrow = ((size_t)head * seq_len + s) * d;
  // kv_rows: rows per kv head in memory (a cache: max_seq_len)
  attn_naive_row(q + qrow, k + (size_t)kvh * kv_rows * d, v + (size_t)kvh * kv_rows * d, out + qrow, visible, d, scale, sc, s_red);
}

hipError_t attn_generic_launch(const float* q, const float* k, const float* v, float* out, uint32_t n_heads, uint32_t n_kv, uint32_t seq_len,
                               uint32_t kv_len, uint32_t kv_rows, uint32_t d, float scale, hipStream_t st) {
  if (n_kv == 0 || n_heads % n_kv || seq_len == 0 || kv_len == 0 || kv_len > 16000 || kv_rows < kv_len || seq_len > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_generic_kernel, dim3(n_heads, seq_len), dim3(256), (size_t)kv_len * 4, st, q, k, v, out, n_heads / n_kv, seq_len,
                     kv_len, kv_rows, d, scale);
  return hipGetLastError();
}

// Decode attention for ANY head_dim / query-heads-per-kv-head inside the engine (the templated kernels above cover
// head_dim 64 / 128 with 1, 2, 4, 8 heads per kv head): one workgroup per query head, kv_len = *pos + 1 from the device,
// scores in LDS (max_seq floats).  Slower than the split kernels, correct for every shape the reference's kernel takes
// (kernels.rs:1395-1458).
__global__ void __launch_bounds__(256) attn_decode_any_kernel(const float* __restrict__ q, const float* __restrict__ kc, const float* __restrict__ vc,
                                                              float* __restrict__ out, uint32_t per_kv, uint32_t max_seq, uint32_t d, float scale,
                                                              const int* __restrict__ pos_ptr) {
  extern __shared__ float sc[];
  __shared__ float s_red[4];
  const uint32_t head = blockIdx.x, kvh = head / per_kv, kv_len = (uint32_t)*pos_ptr + 1;
  attn_naive_row(q + (size_t)head * d, kc + (size_t)kvh * max_seq * d, vc + (size_t)kvh * max_seq * d, out + (size_t)head * d, kv_len, d, scale, sc,
                 s_red);
}

bool attn_shape_has_fast_kernel(uint32_t head_dim, uint32_t group) {
  return attn_dispatch(head_dim, group, [](auto, auto) { return hipSuccess; }) == hipSuccess;
}

hipError_t attn_decode_any_launch(const float* q, const float* kcache, const float* vcache, float* out, uint32_t n_heads, uint32_t n_kv,
                                  uint32_t head_dim, uint32_t max_seq, float scale, const int* pos, hipStream_t st) {
  if (n_kv == 0 || n_heads % n_kv || !pos || (size_t)max_seq * 4 > 150 * 1024) return hipErrorInvalidValue;
  static bool attr_set[64] = {};
  if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(&attn_decode_any_kernel), 152 * 1024, attr_set); e != hipSuccess) return e;
  hipLaunchKernelGGL(attn_decode_any_kernel, dim3(n_heads), dim3(256), (size_t)max_seq * 4, st, q, kcache, vcache, out, n_heads / n_kv, max_seq,
                     head_dim, scale, pos);
  return hipGetLastError();
}

// the merge of a split step's partials: the f32 and byte caches' here, the TurboQuant caches' with the inverse rotation (attention_tq.hip).
// (Last in the file, the single-sequence instantiation first: kernels are emitted in the order of their first use, and the code
// object keeps the kernel order it was measured with — the launch-description note under profiles/)
hipError_t attn_merge_launch(const KvLayout& l, const AttnDecode& a) {
  if (!attn_decode_ok(l, a)) return hipErrorInvalidValue;
  if (l.tq()) return attn_tq_merge_launch(l, a);
  if (l.d % 16 || l.d > 128) return hipErrorInvalidValue;
  const dim3 block(l.d > 64 ? 128 : 64);
  if (!a.n_seq)
    hipLaunchKernelGGL(attn_combine_kernel<false>, dim3(a.n_heads), block, 0, a.st, a.part_ml, a.part_acc, a.n_heads / l.n_kv, l.d, a.n_splits, a.out,
                       a.xq_out);
  else
    hipLaunchKernelGGL(attn_combine_kernel<true>, dim3(a.n_heads, a.n_seq), block, 0, a.st, a.part_ml, a.part_acc, a.n_heads / l.n_kv, l.d, a.n_splits, a.out,
                       a.xq_out);
  return hipGetLastError();
}

}  // namespace lgh
