// sample.hip — Sampler::sample and sample_mirostat (src/sampling/mod.rs:188-387) on the device, inside the per-token graph.
//
// Two launches per step, the sequence as the grid's second dimension (merge: first):
//   samp_partial  kSampParts workgroups per sequence.  Each applies the penalties and the temperature to a contiguous slice of
//                 the vocabulary and leaves the slice's max, its exp-sum relative to that max, and its kSampK best candidates
//                 by (value desc, index asc), sorted.
//   samp_merge    one workgroup per sequence.  Global max and sum (the sum as a fixed tree, not the reference's sequential
//                 loop; under Mirostat, where the sum's rounding reaches mu, that sequential loop), the kSampK best
//                 candidates of all slices, their probabilities sorted by (probability desc, index asc) — the reference's
//                 stable sort — and the truncation and draw scans as sequential f32 sums, as the reference does them.  Then
//                 the token is written, appended to the window and counted.
// The candidates are a prefix of the reference's sorted order as long as their probabilities stay above the smallest one
// among them.  When the top-k / top-p cut or the draw falls past that prefix — with top_k 0 or > kSampK that is every step
// that keeps everything (top_p 1, or a top token alone above top_p: cutoff 0) and every flat one — the merge workgroup
// walks the sorted order in bands instead: a radix select on the probability bits finds the next
// <= kBandCap values, they are sorted in LDS and scanned in order; the chosen position is mapped back to its index (ties:
// ascending index).  Exact, but not fast.
//
// min-p (mod.rs:248-258) cuts the sorted order at the first probability below p[order[0]] * min_p, before top-k; Mirostat
// (mod.rs:304-387) skips the temperature and every truncation but its own, draws against the unnormalized sum and keeps mu
// in the sequence's SampSeq.  Both are settled by the candidates as soon as one valid candidate lies past the cut (below the
// threshold / with a surprise above mu); a cut further out, and every Mirostat v1 step, takes the band walk.
#include "engine.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace lgh {
namespace {

constexpr int kBandCap = 4096;
constexpr int kSeqChunk = kBandCap / 2;   // terms per half of the band buffer in Mirostat's sequential softmax sum
typedef unsigned long long u64;

__device__ __forceinline__ uint32_t f2o(float f) {   // float -> unsigned key of the same order
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float o2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}
// half an ulp above s > 0: a positive p below it leaves fl(s + p) == s.  The sorted order is descending and the running sum
// never shrinks, so once one probability is below it the reference's sequential sum cannot change any more.
__device__ __forceinline__ float half_ulp(float s) { return s > 0.0f ? (__uint_as_float(__float_as_uint(s) + 1u) - s) * 0.5f : 0.0f; }
__device__ __forceinline__ u64 kmax(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ u64 kmin(u64 a, u64 b) { return a < b ? a : b; }

// one key per lane -> the wave's 64 keys sorted descending across lanes (bitonic network)
__device__ u64 sort64(u64 v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const u64 o = shfl_xor64(v, j);
      v = (((lane & j) == 0) == ((lane & k) == 0)) ? kmax(v, o) : kmin(v, o);
    }
  return v;
}
// two descending lists -> the 64 largest of both, descending
__device__ u64 merge64(u64 a, u64 b) {
  const int lane = threadIdx.x & 63;
  u64 v = kmax(a, shfl64(b, 63 - lane));
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const u64 o = shfl_xor64(v, j);
    v = ((lane & j) == 0) ? kmax(v, o) : kmin(v, o);
  }
  return v;
}

// repetition penalty once per occurrence in the window, frequency / presence penalties, temperature (mod.rs:200-221, 390-424)
__device__ __forceinline__ float penalize(float x, uint32_t i, const SampSeq& c, const int* wc, const int* sc) {
  if (c.rp != 1.0f)
    for (int n = wc[i]; n > 0; n--) x = x > 0.0f ? x / c.rp : x * c.rp;
  if (c.fp != 0.0f || c.pp != 0.0f) {
    const int n = sc[i];
    if (n > 0) {
      x -= c.fp * (float)n;
      x -= c.pp;
    }
  }
  if (c.miro == 0 && c.temp > 0.0f && c.temp != 1.0f) x *= c.inv_t;   // (sample_mirostat runs before the temperature)
  return x;
}

__global__ void __launch_bounds__(256) samp_partial(const float* __restrict__ logits, uint32_t vocab, const int* slots, SampBufs B) {
  __shared__ u64 lists[4][64];
  __shared__ float red[4];
  const uint32_t s = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t slot = slots ? (uint32_t)slots[s] : 0u;
  const SampSeq c = B.ctl[slot];
  const int* wc = B.wcnt + (size_t)slot * vocab;
  const int* sc = B.scnt + (size_t)slot * vocab;
  const float* x = logits + (size_t)s * vocab;
  const uint32_t chunk = (vocab + kSampParts - 1) / kSampParts;
  const uint32_t i0 = min(vocab, blk * chunk), i1 = min(vocab, i0 + chunk);
  float m = -INFINITY;
  u64 top = 0;   // 0 = no candidate (below every real key)
  for (uint32_t base = i0 + w * 64; base < i1; base += 256) {
    const uint32_t i = base + lane;
    u64 key = 0;
    if (i < i1) {
      const float v = penalize(x[i], i, c, wc, sc);
      m = fmaxf(m, v);
      key = ((u64)f2o(v) << 32) | (uint32_t)~i;
    }
    if (__any(key > shfl64(top, 63))) top = merge64(top, sort64(key));
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  lists[w][lane] = top;
  if (lane == 0) red[w] = m;
  __syncthreads();
  const float bm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  if (w == 0) {
    u64 t = lists[0][lane];
    for (int o = 1; o < 4; o++) t = merge64(t, lists[o][lane]);
    B.part_k[((size_t)s * kSampParts + blk) * kSampK + lane] = t;
  }
  float acc = 0.0f;
  if (bm != -INFINITY)
    for (uint32_t i = i0 + tid; i < i1; i += 256) acc += expf(penalize(x[i], i, c, wc, sc) - bm);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  __syncthreads();
  if (lane == 0) red[w] = acc;
  __syncthreads();
  if (tid == 0) {
    B.part_m[(size_t)s * kSampParts + blk] = bm;
    B.part_s[(size_t)s * kSampParts + blk] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

struct MergeLds {
  u64 lists[16][64];
  float cp[64];
  int ci[64];
  alignas(16) uint32_t band[kBandCap];
  int hist[256];
  int scan[1024];
  u64 last;
  float gmax, gsum, r, psel;
  int mode, tok, done, kind, count, fin, k, nsel, cnt;
  uint32_t lo, val, prefix, mask, res_val, res_rank;
};

// The next band of the sorted order below `L.last` (exclusive bound on the probability bits): kind 0 none left, 1 every
// value in [lo, last) (count <= kBandCap, gathered and sorted into L.band), 2 one value `val` repeated `count` times.
__device__ void next_band(const uint32_t* pbits, uint32_t vocab, MergeLds& L) {
  const uint32_t tid = threadIdx.x;
  const u64 last = L.last;
  if (tid == 0) { L.prefix = 0; L.mask = 0; L.k = kBandCap; L.fin = 0; }
  for (int pass = 0; pass < 4; pass++) {
    const int shift = 24 - 8 * pass;
    for (uint32_t j = tid; j < 256; j += blockDim.x) L.hist[j] = 0;
    __syncthreads();
    const uint32_t prefix = L.prefix, mask = L.mask;
    for (uint32_t i = tid; i < vocab; i += blockDim.x) {
      const uint32_t b = pbits[i];
      if (b < last && (b & mask) == prefix) atomicAdd(&L.hist[(b >> shift) & 255], 1);
    }
    __syncthreads();
    if (tid == 0) {
      if (pass == 0) {
        int total = 0;
        for (int d = 0; d < 256; d++) total += L.hist[d];
        if (total == 0) { L.kind = 0; L.fin = 1; }
        else if (total <= kBandCap) { L.kind = 1; L.lo = 0; L.count = total; L.fin = 1; }
      }
      if (!L.fin) {
        int acc = 0, d = 255;
        while (d > 0 && acc + L.hist[d] < L.k) { acc += L.hist[d]; d--; }
        L.k -= acc;
        L.prefix |= (uint32_t)d << shift;
        L.mask |= 0xFFu << shift;
        L.nsel = L.hist[d];
        if (pass == 3) {   // prefix = the kBandCap-th largest value; k = its rank within its ties
          const int above = kBandCap - L.k;
          if (above + L.nsel <= kBandCap) { L.kind = 1; L.lo = L.prefix; L.count = above + L.nsel; }
          else if (above > 0) { L.kind = 1; L.lo = L.prefix + 1; L.count = above; }
          else { L.kind = 2; L.val = L.prefix; L.count = L.nsel; }
        }
      }
    }
    __syncthreads();
    if (L.fin) break;
  }
  if (L.kind != 1) return;
  if (tid == 0) L.cnt = 0;
  __syncthreads();
  const uint32_t lo = L.lo;
  for (uint32_t i = tid; i < vocab; i += blockDim.x) {
    const uint32_t b = pbits[i];
    if (b < last && b >= lo) {
      const int q = atomicAdd(&L.cnt, 1);
      if (q < kBandCap) L.band[q] = b;
    }
  }
  __syncthreads();
  const uint32_t n = (uint32_t)min(L.cnt, kBandCap);
  uint32_t n2 = 2;
  while (n2 < n) n2 <<= 1;
  for (uint32_t j = n + tid; j < n2; j += blockDim.x) L.band[j] = 0;
  __syncthreads();
  for (uint32_t k = 2; k <= n2; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < n2; i += blockDim.x) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint32_t a = L.band[i], b = L.band[l];
          if (((i & k) == 0) ? a < b : a > b) { L.band[i] = b; L.band[l] = a; }
        }
      }
      __syncthreads();
    }
  if (tid == 0) L.count = (int)n;
  __syncthreads();
}

__global__ void __launch_bounds__(1024) samp_merge(const float* __restrict__ logits, uint32_t vocab, const int* slots, SampBufs B, int* state,
                                                   int* tok_log, int* tokens_out) {
  __shared__ MergeLds L;
  const uint32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t slot = slots ? (uint32_t)slots[s] : 0u;
  const SampSeq c = B.ctl[slot];
  const int* wc = B.wcnt + (size_t)slot * vocab;
  const int* sc = B.scnt + (size_t)slot * vocab;
  const float* x = logits + (size_t)s * vocab;
  // ---- global max and sum over the slices (kSampParts == one wave)
  if (w == 0) {
    const float bm = B.part_m[(size_t)s * kSampParts + lane], bs = B.part_s[(size_t)s * kSampParts + lane];
    float gm = bm;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) gm = fmaxf(gm, __shfl_xor(gm, off, 64));
    float t = bs > 0.0f ? bs * expf(bm - gm) : 0.0f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
    if (lane == 0) { L.gmax = gm; L.gsum = t; }
  }
  // ---- the kSampK best candidates of all slices
  {
    u64 top = 0;
    for (uint32_t b = w; b < (uint32_t)kSampParts; b += 16) top = merge64(top, B.part_k[((size_t)s * kSampParts + b) * kSampK + lane]);
    L.lists[w][lane] = top;
  }
  __syncthreads();
  // ---- Mirostat: the reference's own denominator.  The reference sums exp(x - max) in f32 in vocabulary order on every path
  // (mod.rs:225-229 as well as sample_mirostat's 311-316), which on spiked logits rounds a large vocabulary's tail away (1.5e-4
  // relative at 32 000 tokens).  The other configurations keep the accurate tree sum above: there the denominator only moves a
  // decision that already sits on a boundary.  Under Mirostat mu moves by eta * log2(p_selected) at every step, so the
  // probability's rounding is part of the sampler's state, and the tree sum would leave mu that far from the reference's.
  // Waves 1..15 fill one half of L.band (free until the band walk) with the next kSeqChunk terms while thread 0 adds the other
  // half in order; the padding past the vocabulary is +0, which changes no sum.
  if (c.miro) {
    float* buf = (float*)L.band;
    const float gmax = L.gmax;
    const uint32_t nch = (vocab + kSeqChunk - 1) / kSeqChunk;
    float acc = 0.0f;
    for (uint32_t ch = 0; ch <= nch; ch++) {
      if (w > 0) {
        if (ch < nch) {
          float* dst = buf + (ch & 1u) * kSeqChunk;
          for (uint32_t j = tid - 64; j < (uint32_t)kSeqChunk; j += blockDim.x - 64) {
            const uint32_t i = ch * kSeqChunk + j;
            dst[j] = i < vocab ? expf(penalize(x[i], i, c, wc, sc) - gmax) : 0.0f;
          }
        }
      } else if (tid == 0 && ch > 0) {
        const float4* src = (const float4*)(buf + ((ch - 1) & 1u) * kSeqChunk);
#pragma unroll 4
        for (int j = 0; j < kSeqChunk / 4; j++) {
          const float4 v = src[j];
          acc += v.x;
          acc += v.y;
          acc += v.z;
          acc += v.w;
        }
      }
      __syncthreads();
    }
    if (tid == 0) L.gsum = acc;
    __syncthreads();
  }
  if (w == 0) {
    u64 t = L.lists[0][lane];
    for (int o = 1; o < 16; o++) t = merge64(t, L.lists[o][lane]);
    u64 key = 0;
    if (t != 0) {
      const float p = expf(o2f((uint32_t)(t >> 32)) - L.gmax) / L.gsum;
      key = ((u64)__float_as_uint(p) << 32) | (uint32_t)t;   // low word: ~index (ties: ascending index)
    }
    key = sort64(key);
    L.cp[lane] = __uint_as_float((uint32_t)(key >> 32));
    L.ci[lane] = (int)~(uint32_t)key;
  }
  __syncthreads();
  // ---- the decision, when the candidates settle it
  const uint32_t nk0 = (c.top_k > 0 && c.top_k < vocab) ? c.top_k : vocab;   // top-k truncation (mod.rs:260-263)
  // min-p (mod.rs:248-258): the order ends before the first probability below this (0: never; cp[0] is the largest of all)
  const float thr = c.min_p > 0.0f && !c.greedy ? L.cp[0] * c.min_p : 0.0f;
  if (tid == 0) {
    const uint32_t ncand = min(vocab, (uint32_t)kSampK);
    L.r = c.greedy ? 0.0f : B.uni[(size_t)slot * B.uni_cap + min((uint32_t)c.step, B.uni_cap - 1)];
    // valid prefix: every candidate whose probability exceeds the smallest candidate's (no element outside can tie it)
    uint32_t V = ncand;
    if (vocab > (uint32_t)kSampK) {
      V = 0;
      while (V < (uint32_t)kSampK && L.cp[V] > L.cp[kSampK - 1]) V++;
    }
    int mode = 0, tok = 0;
    float psel = 0.0f;
    if (c.miro) {   // sample_mirostat (mod.rs:304-387)
      // v2: the first rank whose surprise exceeds mu, at least 1.  v1: n = clamp((2^mu * vocab) as usize, 1, vocab) with
      // mu in [0, 20] (it starts at 2 * tau with tau >= 0 and is clamped after every update), so 2^mu >= 1 and n == vocab:
      // no truncation.
      int trunc = -1;
      if (c.miro == 2)
        for (uint32_t j = 0; j < V; j++)
          if (-log2f(L.cp[j]) > c.mu) { trunc = (int)max(j, 1u); break; }
      if (trunc < 0 && vocab <= (uint32_t)kSampK) trunc = (int)vocab;   // (every candidate is valid: V == vocab)
      if (trunc < 0) mode = 1;
      else {   // the draw against the unnormalized sum; nobody above r: the TOP token (mod.rs:363-373)
        float fsum = 0.0f, cum2 = 0.0f;
        for (int j = 0; j < trunc; j++) fsum += L.cp[j];
        const float rf = L.r * fsum;
        int k = 0;
        for (int j = 0; j < trunc; j++) {
          cum2 += L.cp[j];
          if (cum2 > rf) { k = j; break; }
        }
        tok = L.ci[k];
        psel = L.cp[k];
      }
    } else if (c.greedy) {   // the LAST index of the maximal probability (max_by, mod.rs:235-243)
      if (vocab > (uint32_t)kSampK && L.cp[kSampK - 1] == L.cp[0]) mode = 2;
      else {
        tok = L.ci[0];
        for (uint32_t j = 1; j < ncand; j++)
          if (L.cp[j] == L.cp[0]) tok = max(tok, L.ci[j]);
      }
    } else {
      // min-p, settled when a valid candidate is below the threshold: the order is exactly the candidates before it, and top-k
      // compares against that length
      uint32_t nkc = nk0;
      if (thr > 0.0f)
        for (uint32_t j = 1; j < V; j++)
          if (L.cp[j] < thr) { nkc = min(nkc, j); break; }
      int nk = -1;
      float cum = 0.0f, sk = 0.0f;
      bool crossed = false;
      const uint32_t lim = min(nkc, V);
      for (uint32_t j = 0; j < lim; j++) {   // top-p (mod.rs:266-277): the first position whose cumulative sum exceeds top_p
        cum += L.cp[j];
        if (c.top_p < 1.0f && !crossed && cum > c.top_p) {
          crossed = true;
          if (j > 0) { nk = (int)j + 1; sk = cum; break; }   // cutoff 0 keeps everything (reference quirk)
        }
      }
      if (nk < 0 && nkc <= V) { nk = (int)nkc; sk = cum; }
      // nothing is truncated inside the prefix (a cutoff at 0, or top_p 1): the kept sum is the whole order's, which the prefix
      // already settles when every later probability (<= cp[V]) is below half an ulp of it; the draw must then land inside
      bool inside = nk >= 0;
      if (nk < 0 && L.cp[V] < half_ulp(cum)) { nk = (int)nkc; sk = cum; }
      if (nk < 0) mode = 1;
      else {   // renormalize and draw (mod.rs:279-303)
        tok = L.ci[min(nk, (int)V) - 1];
        float cum2 = 0.0f;
        bool hit = false;
        for (int j = 0; j < min(nk, (int)V); j++) {
          cum2 += L.cp[j] / sk;
          if (L.r < cum2) { tok = L.ci[j]; hit = true; break; }
        }
        if (!hit && !inside && nk > (int)V) mode = 1;   // (past the prefix: the general path finds the position)
      }
    }
    L.mode = mode;
    L.tok = tok;
    L.psel = psel;
  }
  __syncthreads();
  // ---- general path: the whole vocabulary's probabilities, walked in sorted order
  if (L.mode != 0) {
    float* pb = B.pb + (size_t)s * vocab;
    const uint32_t* pbits = (const uint32_t*)pb;
    const float gmax = L.gmax, gsum = L.gsum;
    for (uint32_t i = tid; i < vocab; i += blockDim.x) pb[i] = expf(penalize(x[i], i, c, wc, sc) - gmax) / gsum;
    __syncthreads();
    if (L.mode == 2) {
      if (tid == 0) L.tok = -1;
      __syncthreads();
      const uint32_t pmax = __float_as_uint(L.cp[0]);
      int best = -1;
      for (uint32_t i = tid; i < vocab; i += blockDim.x)
        if (pbits[i] == pmax) best = (int)i;
      if (best >= 0) atomicMax(&L.tok, best);
      __syncthreads();
    } else {
      // thread 0's scan state; phase 0 finds the kept count nk and their sum sk, phase 1 the drawn position
      uint32_t pos = 0, nk = 0, prev = 0, gstart = 0, last_val = 0, last_rank = 0;
      float cum = 0.0f, sk = 0.0f, hu = 0.0f, rf = 0.0f;
      const uint32_t top_val = __float_as_uint(L.cp[0]);   // the first of the order: the smallest index with the largest probability
      bool crossed = false;
      const bool cut = thr > 0.0f || c.miro == 2;   // a min-p or v2 cut to look for: chosen once, the other walks skip the tests
      for (int phase = 0; phase < 2; phase++) {
        if (tid == 0) { L.last = 1ull << 32; L.done = 0; pos = 0; cum = 0.0f; prev = 0xFFFFFFFFu; }
        __syncthreads();
        for (;;) {
          next_band(pbits, vocab, L);
          if (L.kind == 0) break;
          if (tid == 0) {
            const int n = L.count;
            for (int q = 0; q < n && !L.done; q++) {
              const uint32_t bits = L.kind == 1 ? L.band[q] : L.val;
              const float p = __uint_as_float(bits);
              if (phase == 0) {
                // the sum cannot change any more (hu: half an ulp of the sum as it was up to 64 elements ago, never above today's)
                if ((pos & 63) == 0) hu = half_ulp(cum);
                if (p < hu && thr == 0.0f) { nk = nk0; sk = cum; L.done = 1; break; }   // (under min-p the walk needs the cut itself: it ends the kept set)
                if (cut) {
                  if (p < thr) { nk = pos; sk = cum; L.done = 1; break; }   // min-p: the order ends here (pos > 0: thr <= cp[0])
                  if (c.miro == 2 && -log2f(p) > c.mu) {                    // Mirostat v2: truncate at max(rank, 1)
                    if (pos == 0) { cum = p; pos = 1; }
                    nk = pos; sk = cum; L.done = 1; break;
                  }
                }
                cum += p;
                if (c.top_p < 1.0f && !crossed && cum > c.top_p) {
                  crossed = true;
                  if (pos > 0) { nk = pos + 1; sk = cum; L.done = 1; }
                }
                pos++;
                if (!L.done && pos == nk0) { nk = nk0; sk = cum; L.done = 1; }
              } else {
                if (bits != prev) { prev = bits; gstart = pos; }
                last_val = bits;
                last_rank = pos - gstart;
                if (c.miro) {   // unnormalized, against r * fsum; nobody above it: the top token
                  cum += p;
                  if (cum > rf) { L.res_val = bits; L.res_rank = last_rank; L.done = 1; }
                } else {
                  cum += p / sk;
                  if (L.r < cum) { L.res_val = bits; L.res_rank = last_rank; L.done = 1; }
                }
                pos++;
                if (!L.done && pos == nk) {
                  L.res_val = c.miro ? top_val : last_val;
                  L.res_rank = c.miro ? 0u : last_rank;
                  L.done = 1;
                }
              }
            }
            L.last = L.kind == 1 ? L.lo : L.val;
          }
          __syncthreads();
          if (L.done) break;
        }
        if (tid == 0 && !L.done) {   // (the order ran out: only with non-finite values)
          if (phase == 0) { nk = pos; sk = cum; }
          else { L.res_val = c.miro ? top_val : last_val; L.res_rank = c.miro ? 0u : last_rank; }
        }
        if (tid == 0 && phase == 0) rf = L.r * sk;
        __syncthreads();
      }
      // position -> index: the res_rank-th smallest index whose probability has the bits res_val
      const uint32_t v = L.res_val, rank = L.res_rank;
      if (tid == 0) L.psel = __uint_as_float(v);
      const uint32_t per = (vocab + blockDim.x - 1) / blockDim.x;
      const uint32_t a0 = min(vocab, tid * per), a1 = min(vocab, a0 + per);
      int cnt = 0;
      for (uint32_t i = a0; i < a1; i++) cnt += pbits[i] == v;
      L.scan[tid] = cnt;
      if (tid == 0) L.tok = -1;
      __syncthreads();
      if (tid == 0) {
        int acc = 0;
        for (uint32_t t = 0; t < blockDim.x; t++) { const int n = L.scan[t]; L.scan[t] = acc; acc += n; }
      }
      __syncthreads();
      const int ex = L.scan[tid];
      if ((int)rank >= ex && (int)rank < ex + cnt) {
        int k = (int)rank - ex;
        for (uint32_t i = a0; i < a1; i++)
          if (pbits[i] == v && k-- == 0) { L.tok = (int)i; break; }
      }
      __syncthreads();
    }
  }
  // ---- the token: fed back, logged, counted, appended to the window
  if (tid == 0) {
    const int t = min(max(L.tok, 0), (int)vocab - 1);
    if (state) { state[ST_ARGMAX] = t; state[ST_TOKEN] = t; }
    if (tok_log) tok_log[state ? state[ST_POS] : 0] = t;
    if (tokens_out) tokens_out[s] = t;
    if (c.track) {
      SampSeq* cs = B.ctl + slot;
      int* wcw = B.wcnt + (size_t)slot * vocab;
      int* scw = B.scnt + (size_t)slot * vocab;
      int* tk = B.tk + (size_t)slot * B.tk_cap;
      if (!c.greedy && !c.eos_done) scw[t] += 1;   // greedy does not count (mod.rs:235-243 returns first)
      if (c.eos >= 0 && t == c.eos) cs->eos_done = 1;
      const int nxt = c.step + 1;
      const int fi = c.lv_h + nxt;
      if (fi >= 0 && fi < (int)B.tk_cap) tk[fi] = t;
      wcw[t] += 1;
      if (c.window > 0) {
        const int j = c.lv_a + nxt;
        if (j >= 0) {
          const int q = j < c.lv_h ? j : j - c.lv_g;
          if (q >= 0 && q < (int)B.tk_cap) {
            const int u = tk[q];
            if (u >= 0 && (uint32_t)u < vocab) wcw[u] -= 1;
          }
        }
      }
      cs->step = nxt;
    }
    if (c.miro && !c.eos_done) {   // mod.rs:377-383, from the selected token's probability; frozen after eos like the counts
      float mu = c.mu - c.eta * (-log2f(L.psel) - c.tau);
      mu = mu < 0.0f ? 0.0f : mu > 20.0f ? 20.0f : mu;
      B.ctl[slot].mu = mu;
    }
  }
}

__global__ void __launch_bounds__(256) samp_window_kernel(int* wcnt, const int* pairs, uint32_t n, uint32_t vocab) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) {
    const int t = pairs[2 * j];
    if (t >= 0 && (uint32_t)t < vocab) wcnt[t] = pairs[2 * j + 1];
  }
}

}  // namespace

hipError_t sample_launch(const SampBufs& B, const float* logits, uint32_t vocab, uint32_t n_seq, const int* slots, int* state,
                         int* tok_log, int* tokens_out, hipStream_t st) {
  if (n_seq == 0 || n_seq > B.n_rows || vocab != B.vocab || B.uni_cap == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(samp_partial, dim3(kSampParts, n_seq), dim3(256), 0, st, logits, vocab, slots, B);
  hipLaunchKernelGGL(samp_merge, dim3(n_seq), dim3(1024), 0, st, logits, vocab, slots, B, state, tok_log, tokens_out);
  return hipGetLastError();
}

hipError_t sample_window_launch(const SampBufs& B, uint32_t slot, uint32_t n_pairs, hipStream_t st) {
  if (slot >= B.n_slots || n_pairs > B.vocab) return hipErrorInvalidValue;
  int* wc = B.wcnt + (size_t)slot * B.vocab;
  hipError_t e = hipMemsetAsync(wc, 0, (size_t)B.vocab * 4, st);
  if (e != hipSuccess || n_pairs == 0) return e;
  hipLaunchKernelGGL(samp_window_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, st, wc, B.stage, n_pairs, B.vocab);
  return hipGetLastError();
}

}  // namespace lgh

using namespace lgh;

// ------------------------------------------------------------------------------------------------
// host side: buffers, config checks, the per-call window set-up
// ------------------------------------------------------------------------------------------------
int samp_alloc(lgh_ctx* c, SampBufs& B, uint32_t n_slots, uint32_t n_rows) {
  const lgh_model_desc& d = c->d;
  B.n_slots = n_slots;
  B.n_rows = n_rows;
  B.vocab = d.vocab_size;
  B.tk_cap = 2 * d.max_seq_len + 2;   // <= n_steps + 1 leaving history tokens, then n_steps + 1 fed tokens
  B.uni_cap = std::max(1u, d.max_seq_len);
  const size_t V = d.vocab_size;
  const AllocSpec bufs[] = {
      {(void**)&B.ctl, n_slots * sizeof(SampSeq)},          {(void**)&B.wcnt, n_slots * V * 4},
      {(void**)&B.scnt, n_slots * V * 4},                   {(void**)&B.tk, (size_t)n_slots * B.tk_cap * 4},
      {(void**)&B.uni, (size_t)n_slots * B.uni_cap * 4},    {(void**)&B.pb, n_rows * V * 4},
      {(void**)&B.part_m, (size_t)n_rows * kSampParts * 4}, {(void**)&B.part_s, (size_t)n_rows * kSampParts * 4},
      {(void**)&B.part_k, (size_t)n_rows * kSampParts * kSampK * 8}, {(void**)&B.stage, (2 * V + 2 * kMaxBatch) * 4},
  };
  return alloc_zeroed(c, bufs, sizeof(bufs) / sizeof(bufs[0]), c->stats.scratch_bytes);
}

int samp_check(lgh_ctx* c, const lgh_sampler_config* s) {
  if (!s) return fail(c, LGH_INVALID_ARGUMENT, "sampler config is NULL");
  if (!std::isfinite(s->temperature) || s->temperature < 0.0f) return fail(c, LGH_INVALID_ARGUMENT, "temperature must be finite and >= 0");
  if (!(s->top_p > 0.0f && s->top_p <= 1.0f)) return fail(c, LGH_INVALID_ARGUMENT, "top_p must be in (0, 1]");
  if (!(s->repeat_penalty > 0.0f) || !std::isfinite(s->repeat_penalty)) return fail(c, LGH_INVALID_ARGUMENT, "repeat_penalty must be finite and > 0");
  if (!std::isfinite(s->frequency_penalty) || !std::isfinite(s->presence_penalty)) return fail(c, LGH_INVALID_ARGUMENT, "penalties must be finite");
  return LGH_OK;
}

int samp_check_ex(lgh_ctx* c, const lgh_sampler_config_ex* s) {
  if (!s) return fail(c, LGH_INVALID_ARGUMENT, "sampler config is NULL");
  if (s->struct_size != sizeof(lgh_sampler_config_ex)) return fail(c, LGH_INVALID_ARGUMENT, "lgh_sampler_config_ex.struct_size mismatch");
  const int rc = samp_check(c, &s->base);
  if (rc) return rc;
  if (!(s->min_p >= 0.0f && s->min_p <= 1.0f)) return fail(c, LGH_INVALID_ARGUMENT, "min_p must be in [0, 1]");
  if (s->mirostat > 2) return fail(c, LGH_INVALID_ARGUMENT, "mirostat must be 0, 1 or 2");
  if (!std::isfinite(s->mirostat_tau) || !std::isfinite(s->mirostat_eta) || s->mirostat_tau < 0.0f)
    return fail(c, LGH_INVALID_ARGUMENT, "mirostat_tau must be finite and >= 0, mirostat_eta finite");
  return LGH_OK;
}

lgh_sampler_config_ex samp_plain(const lgh_sampler_config& s) {
  lgh_sampler_config_ex x{};
  x.struct_size = sizeof(x);
  x.base = s;
  return x;
}

bool samp_needs_uniforms(const lgh_sampler_config_ex& s) { return s.mirostat || !(s.base.temperature == 0.0f || s.base.top_k == 1); }

// Sampler::new's mirostat_mu (mod.rs:156-161)
static float mu_start(const lgh_sampler_config_ex& s) { return s.mirostat ? s.mirostat_tau * 2.0f : 10.0f; }

int samp_reset(lgh_ctx* c, SampBufs& B, uint32_t slot, const lgh_sampler_config_ex& cfg) {
  const float mu = mu_start(cfg);
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemsetAsync(B.scnt + (size_t)slot * B.vocab, 0, (size_t)B.vocab * 4, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(&B.ctl[slot].mu, &mu, 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

int samp_mu(lgh_ctx* c, SampBufs& B, uint32_t slot, float* mu) {
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpy(mu, &B.ctl[slot].mu, 4, hipMemcpyDeviceToHost));
  return LGH_OK;
}

static SampSeq seq_of(const lgh_sampler_config_ex& x) {
  lgh_sampler_config s = x.base;
  SampSeq q{};
  q.rp = s.repeat_penalty;
  q.fp = s.frequency_penalty;
  q.pp = s.presence_penalty;
  q.window = s.repeat_window;
  q.eos = s.eos_token;
  q.lv_a = INT_MIN / 2;
  q.mu = mu_start(x);
  if (x.mirostat) {   // sample_mirostat returns before the temperature, the greedy test, min-p, top-k and top-p (mod.rs:210-213)
    q.temp = q.inv_t = q.top_p = 1.0f;
    q.miro = (int32_t)x.mirostat;
    q.tau = x.mirostat_tau;
    q.eta = x.mirostat_eta;
    return q;
  }
  q.min_p = x.min_p;
  q.temp = s.temperature;
  q.inv_t = s.temperature > 0.0f ? 1.0f / s.temperature : 0.0f;
  q.top_p = s.top_p;
  q.top_k = s.top_k;
  q.greedy = s.temperature == 0.0f || s.top_k == 1;
  return q;
}

int samp_begin(lgh_ctx* c, SampBufs& B, uint32_t slot, const lgh_sampler_config_ex& cfg, const uint32_t* hist, size_t n_hist, uint32_t first,
               size_t n_steps, const float* uni, size_t uni_stride) {
  if (n_steps > B.uni_cap || n_steps + 1 > B.tk_cap / 2) return fail(c, LGH_INVALID_ARGUMENT, "too many steps");
  const size_t W = cfg.base.repeat_window;
  const size_t L0 = W ? std::min(n_hist, W) : n_hist;   // the window's history tokens
  const uint32_t* hw = hist + (n_hist - L0);
  SampSeq q = seq_of(cfg);
  q.track = 1;
  // step 0's window: the last W of hw ++ [first]
  std::vector<uint32_t> win(hw, hw + L0);
  win.push_back(first);
  if (W && win.size() > W) win.erase(win.begin(), win.begin() + (win.size() - W));
  std::sort(win.begin(), win.end());
  std::vector<int> pairs;
  for (size_t i = 0; i < win.size();) {
    size_t j = i;
    while (j < win.size() && win[j] == win[i]) j++;
    if (win[i] < B.vocab) { pairs.push_back((int)win[i]); pairs.push_back((int)(j - i)); }
    i = j;
  }
  // the tokens that leave the window during the call: S[lv_a + i] for steps i >= 1 (S = hw ++ fed tokens)
  std::vector<int> tk;
  if (W) {
    const long long a = (long long)L0 - (long long)W;   // <= 0
    const long long h = std::max(0LL, std::min((long long)L0, (long long)n_steps + 1 + a));
    q.lv_a = (int)std::max<long long>(a, INT_MIN / 2);
    q.lv_h = (int)h;
    q.lv_g = (int)((long long)L0 - h);
    tk.assign(hw, hw + h);
  }
  tk.push_back((int)first);   // fed token 0
  std::vector<float> u(std::max<size_t>(n_steps, 1), 0.0f);
  if (uni && !q.greedy)
    for (size_t i = 0; i < n_steps; i++) u[i] = uni[i * uni_stride];
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));   // the previous call's steps are done with these buffers
  // (everything but mu, which carries over from the previous call)
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(B.ctl + slot, &q, kSampSeqCallBytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(B.tk + (size_t)slot * B.tk_cap, tk.data(), tk.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(B.uni + (size_t)slot * B.uni_cap, u.data(), u.size() * 4, hipMemcpyHostToDevice, c->stream));
  if (!pairs.empty())
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(B.stage, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, sample_window_launch(B, slot, (uint32_t)(pairs.size() / 2), c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

// One eager launch of every sampling kernel with a greedy, non-tracking config on whatever the logits buffer holds (a kernel
// whose first launch happens inside a capture is not replayed: engine.hip warm_kernels).  The row outputs are scratch.
int samp_warm(lgh_ctx* c, SampBufs& B, const float* logits, uint32_t n_seq) {
  lgh_sampler_config g{};
  g.temperature = 0.0f; g.top_k = 1; g.top_p = 1.0f; g.repeat_penalty = 1.0f; g.eos_token = -1;
  const SampSeq q = seq_of(samp_plain(g));
  std::vector<SampSeq> qs(B.n_slots, q);
  std::vector<int> slots(n_seq);
  for (uint32_t i = 0; i < n_seq; i++) slots[i] = (int)(i % B.n_slots);
  int* d_slots = B.stage;   // (staging words, free outside a call)
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(B.ctl, qs.data(), qs.size() * sizeof(SampSeq), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(d_slots, slots.data(), n_seq * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, sample_window_launch(B, 0, 0, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, sample_launch(B, logits, B.vocab, n_seq, d_slots, nullptr, nullptr, d_slots + kMaxBatch, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemsetAsync(B.ctl, 0, B.n_slots * sizeof(SampSeq), c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

// One Sampler::sample call on device logits (lgh_op_sample): the window is the end of `recent`, counts[vocab] (or zero) the
// sampled counts, mu_in the sampler's mirostat_mu; nothing is tracked, *mu_out (when non-NULL) is mu after the step.
int samp_one(lgh_ctx* c, SampBufs& B, const lgh_sampler_config_ex& cfg, const uint32_t* recent, size_t n_recent, const uint32_t* counts,
             float uniform, float mu_in, const float* d_logits, uint32_t* token_out, float* mu_out) {
  SampSeq q = seq_of(cfg);
  q.mu = mu_in;
  const size_t W = cfg.base.repeat_window, n = W ? std::min(W, n_recent) : n_recent;
  std::vector<uint32_t> win(recent + (n_recent - n), recent + n_recent);
  std::sort(win.begin(), win.end());
  std::vector<int> pairs;
  for (size_t i = 0; i < win.size();) {
    size_t j = i;
    while (j < win.size() && win[j] == win[i]) j++;
    if (win[i] < B.vocab) { pairs.push_back((int)win[i]); pairs.push_back((int)(j - i)); }
    i = j;
  }
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(B.ctl, &q, sizeof(q), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(B.uni, &uniform, 4, hipMemcpyHostToDevice, c->stream));
  if (counts) HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(B.scnt, counts, (size_t)B.vocab * 4, hipMemcpyHostToDevice, c->stream));
  if (!pairs.empty())
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(B.stage, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, sample_window_launch(B, 0, (uint32_t)(pairs.size() / 2), c->stream));
  int* d_tok = B.stage + 2 * (size_t)B.vocab;
  HIP_TRY(c, LGH_OPERATION_FAILED, sample_launch(B, d_logits, B.vocab, 1, nullptr, nullptr, nullptr, d_tok, c->stream));
  int tok = 0;
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(&tok, d_tok, 4, hipMemcpyDeviceToHost, c->stream));
  if (mu_out) HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(mu_out, &B.ctl[0].mu, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  *token_out = (uint32_t)tok;
  return LGH_OK;
}
