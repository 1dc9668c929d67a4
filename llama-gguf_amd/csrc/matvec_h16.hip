// matvec_h16.hip — decode mat-vec over F16 / BF16 weights kept 16-bit in HBM (contexts with LGH_WEIGHTS_HALF_TILES), and the
// upload-time repack into their tile layout.
//
// The reference expands such a matrix to f32 at upload (src/backend/cuda/dequant_weights.rs:211-231) and so did this library:
// twice the bytes per token, and none of the fused prologues / epilogues.  A half is not a small integer, so the int8-limb
// matrix-core mat-vec (matvec_mfma.hip) cannot take it; and the step is HBM-bound (about 13 B per clock and CU against 64
// lanes of fma), so a matrix instruction — which would force the f32 activations through a rounding or a limb split — buys
// nothing.  This kernel is plain f32 fma over exactly converted weights: F16 is consumed in place by the mixed-precision fma
// (v_fma_mix_f32, no convert instruction), BF16 by a shift or a mask.  x stays f32, as in matvec.hip.
//
// Layout (kDevF16_T16 / kDevBF16_T16): tiles of 16 rows x 256 elements = 8192 B, rows padded to 16 with zeros, tile (rt, b) at
// (rt * nblk + b) * 8192.  Lane 16c + n of a wave owns, for step pp (64 elements), the 16 elements 64pp + 16c .. +15 of row n,
// as in every other tile16 layout: 8 pieces of 16 bytes per tile, piece j = 2pp + h (elements 64pp + 16c + 8h .. +7) at
// j * 1024 + lane * 16, so every load instruction of a wave is one contiguous 1 KiB.  Inside a piece the 8 halves are in the
// order 0,2,1,3,4,6,5,7 — the XH chunk's (prefill.hip): a loaded piece is the f16 GEMM's A operand as it stands.
//
// Work split: ONE workgroup per CU, as mv_plan; its waves are T k-slices x G groups of row tiles.  A wave walks the tiles of its
// slice for one row tile after the other (and pass after pass), the next tile's 8 loads in flight while this one is consumed;
// every item is a whole tile, so the load counts are static.  A lane keeps its (row n, chunk c) partial sums across all tiles of
// its slice: no reduction per row inside the stream.  At the end of a row tile the four lane groups are added with two
// cross-lane steps, and the T slices meet in LDS in the red[] layout mv_epilogue reads — 2 steps per 16 rows where mv_rows
// spends 6 per row.
// x is staged once per workgroup in LDS (x * norm_w with the RMSNorm prologue, each wave leaving its share of sum x^2); a lane
// reads the 16 consecutive floats of its chunk for a step with four ds_read_b128, the 16 lanes of a chunk reading one address.
// Passes with input vectors of their own (the two experts of a MoE down projection) get one staged vector each.
// Dynamic LDS: red[red_floats] | ssq[16] | x[nx * K].
#include "device_utils.h"
#include "mv_epilogue.h"

namespace lgh {

constexpr uint32_t kHTileBytes = 8192;
constexpr int kHXPT = 4;   // float4 x-loads a thread keeps in flight while staging x into LDS

// ------------------------------------------------------------------------------------------------
// upload: native row-major halves -> tiles.  One thread per piece, no atomics.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) repack_half_t16_kernel(const uint8_t* __restrict__ raw, uint8_t* __restrict__ dst, uint32_t n_rows,
                                                             uint32_t nblk, uint64_t total) {
  for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * 256) {
    const uint32_t lane = (uint32_t)(idx & 63), j = (uint32_t)(idx >> 6) & 7;
    const uint64_t tile = idx >> 9;
    const uint32_t rt = (uint32_t)(tile / nblk), b = (uint32_t)(tile % nblk);
    const uint32_t row = rt * 16 + (lane & 15), e0 = b * 256 + (j >> 1) * 64 + (lane >> 4) * 16 + (j & 1) * 8;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < n_rows) v = *reinterpret_cast<const u32x4*>(raw + ((size_t)row * nblk * 256 + e0) * 2);
    const u32x4 o = {(v.x & 0xFFFFu) | (v.y << 16), (v.x >> 16) | (v.y & 0xFFFF0000u), (v.z & 0xFFFFu) | (v.w << 16), (v.z >> 16) | (v.w & 0xFFFF0000u)};
    *reinterpret_cast<u32x4*>(dst + tile * kHTileBytes + j * 1024 + lane * 16) = o;
  }
}

hipError_t repack_half_t16_launch(const uint8_t* raw, uint8_t* dst, uint32_t n_rows, uint32_t nblk, hipStream_t st) {
  const uint64_t total = (uint64_t)((n_rows + 15) / 16) * nblk * 512;
  uint64_t blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(repack_half_t16_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, raw, dst, n_rows, nblk, total);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// the kernel
// ------------------------------------------------------------------------------------------------
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// acc + w * x with w the low / high half of `word`, converted exactly
template <bool BF16, int HI>
__device__ __forceinline__ float h16_fma(uint32_t word, float x, float acc) {
  if (BF16) return __builtin_fmaf(__builtin_bit_cast(float, HI ? word & 0xFFFF0000u : word << 16), x, acc);
  const f16x2 h = __builtin_bit_cast(f16x2, word);
  return __builtin_fmaf((float)(HI ? h.y : h.x), x, acc);   // v_fma_mix_f32: the half is read in place
}

struct HTile { u32x4 q[8]; };

__device__ __forceinline__ void h16_load(HTile& t, const uint8_t* p) {
#pragma unroll
  for (int j = 0; j < 8; j++) t.q[j] = ldg_nt128(p + j * 1024);
}

// one tile against the 256 staged floats at xb: 64 multiply-adds into 4 independent chains
template <bool BF16>
__device__ __forceinline__ void h16_tile(const HTile& t, const float* xb, float (&acc)[4]) {
#pragma unroll
  for (int pp = 0; pp < 4; pp++) {
    f32x4 xv[4];
#pragma unroll
    for (int i = 0; i < 4; i++) xv[i] = *reinterpret_cast<const f32x4*>(xb + pp * 64 + 4 * i);
#pragma unroll
    for (int h = 0; h < 2; h++) {   // piece 2pp + h: words (e0, e2) (e1, e3) (e4, e6) (e5, e7) of elements 8h .. 8h + 7
      const u32x4 w = t.q[2 * pp + h];
      const f32x4 a = xv[2 * h], b = xv[2 * h + 1];
      acc[0] = h16_fma<BF16, 0>(w.x, a.x, acc[0]);
      acc[1] = h16_fma<BF16, 0>(w.y, a.y, acc[1]);
      acc[2] = h16_fma<BF16, 1>(w.x, a.z, acc[2]);
      acc[3] = h16_fma<BF16, 1>(w.y, a.w, acc[3]);
      acc[0] = h16_fma<BF16, 0>(w.z, b.x, acc[0]);
      acc[1] = h16_fma<BF16, 0>(w.w, b.y, acc[1]);
      acc[2] = h16_fma<BF16, 1>(w.z, b.z, acc[2]);
      acc[3] = h16_fma<BF16, 1>(w.w, b.w, acc[3]);
    }
  }
}

// a segment's passes read input vectors of their own (MoE down: one activation per expert)
__device__ __forceinline__ bool h16_multi_x(const MvSeg& S) { return S.npass > 1 && S.pass[1].x != S.pass[0].x; }

template <bool BF16>
__device__ __forceinline__ void mvh_rows(const MvLaunch& L, const MvSeg& S, uint32_t wg, float* xs, float* red, float* ssq) {
  const uint32_t tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool active = wave < S.T * S.G;
  const uint32_t ks = active ? wave % S.T : 0, rg = active ? wave / S.T : 0;
  const uint32_t tiles_wg = S.rows_per_wg >> 4, tpg = tiles_wg / S.G, ntiles = (S.n_rows + 15) >> 4;
  const uint32_t t0 = wg * tiles_wg + rg * tpg;                       // this wave's first row tile ...
  const uint32_t nt = active && t0 < ntiles ? min(tpg, ntiles - t0) : 0;   // ... and how many of them exist
  const uint32_t bps = (S.nblk + S.T - 1) / S.T, b0 = ks * bps;       // its k-slice: blocks b0 .. b0 + nb - 1
  const uint32_t nb = b0 < S.nblk ? min(bps, S.nblk - b0) : 0;
  const bool nrm = L.do_norm != 0;
  const uint32_t nx = h16_multi_x(S) ? (uint32_t)S.npass : 1u;
  uint32_t remaining = nb ? (uint32_t)S.npass * nt * nb : 0;          // items (pass, row tile, block), walked in that order

  // Every pass's matrix (its expert selected) as a scalar base, before the stream: fetched inside it, the expert index is a vector
  // load whose wait drains the tile in flight, and the pass's pointers a dependent scalar round trip per tile.
  auto pass_base = [&](int p) -> const uint8_t* {
    if (p >= S.npass) return nullptr;
    const MvPass& P = S.pass[p];
    const uint64_t e = P.sel ? (uint64_t)sload_u32(P.sel) : 0;
    return P.plane[0] + e * P.sel_stride[0];
  };
  const uint8_t* const wb0 = pass_base(0);
  const uint8_t* const wb1 = pass_base(1);
  const uint8_t* const wb2 = pass_base(2);
  const uint8_t* const wb3 = pass_base(3);
  // the next item to issue: its pass, row tile and block
  uint32_t ip = 0, it = 0, ib = 0;
  auto issue = [&](HTile& buf) {
    const uint8_t* wb = ip == 0 ? wb0 : ip == 1 ? wb1 : ip == 2 ? wb2 : wb3;
    h16_load(buf, wb + ((size_t)(t0 + it) * S.nblk + b0 + ib) * kHTileBytes + lane * 16);
    if (++ib == nb) { ib = 0; if (++it == nt) { it = 0; ++ip; } }
  };

  HTile A, Bq;
  // ---- prologue: x -> (x * w, sum x^2) -> LDS, with the first tile already in flight
  float ss = 0.0f;
  const uint32_t k4 = L.k >> 2;
  for (uint32_t v = 0; v < nx; v++) {
    const float* xg = S.pass[v].x;
    f32x4* xd = reinterpret_cast<f32x4*>(xs + (size_t)v * L.k);
    for (uint32_t base = 0; base < k4; base += kHXPT * nthr) {
      f32x4 xv[kHXPT], wv[kHXPT];
#pragma unroll
      for (int j = 0; j < kHXPT; j++) {
        const uint32_t i = base + tid + j * nthr;
        if (i < k4) xv[j] = reinterpret_cast<const f32x4*>(xg)[i];
      }
      if (nrm) {
#pragma unroll
        for (int j = 0; j < kHXPT; j++) {
          const uint32_t i = base + tid + j * nthr;
          if (i < k4) wv[j] = reinterpret_cast<const f32x4*>(L.norm_w)[i];
        }
      }
      if (v == 0 && base == 0 && remaining) issue(A);
#pragma unroll
      for (int j = 0; j < kHXPT; j++) {
        const uint32_t i = base + tid + j * nthr;
        if (i < k4) {
          f32x4 x4 = xv[j];
          if (nrm) {
            ss = __builtin_fmaf(x4.x, x4.x, ss);
            ss = __builtin_fmaf(x4.y, x4.y, ss);
            ss = __builtin_fmaf(x4.z, x4.z, ss);
            ss = __builtin_fmaf(x4.w, x4.w, ss);
            x4 = x4 * wv[j];
          }
          xd[i] = x4;
        }
      }
    }
  }
  if (nrm) {  // this wave's share of sum(x^2); the epilogue adds the shares of all waves
    ss = wave_sum_to_lane63(ss);
    if (lane == 63) ssq[wave] = ss;
  }
  // publish x: wait for the LDS writes only — the weight loads stay in flight across the barrier
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (!nt) return;

  const uint32_t n = lane & 15, c = lane >> 4;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t cp = 0, ct = 0, cb = 0;   // the item being consumed
  // the end of a row tile's slice: the four chunk groups meet (lanes n, n + 16, n + 32, n + 48), lanes 0..15 leave the 16 rows
  auto finish = [&]() {
    float v = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lane < 16) red[(size_t)(cp * S.T + ks) * S.rows_per_wg + (rg * tpg + ct) * 16 + n] = v;
    acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
  };
  auto consume = [&](const HTile& buf) {
    h16_tile<BF16>(buf, xs + (size_t)(nx > 1 ? cp : 0) * L.k + (b0 + cb) * 256 + c * 16, acc);
    if (++cb == nb) {
      finish();
      cb = 0;
      if (++ct == nt) { ct = 0; ++cp; }
    }
  };
  if (!remaining) {   // (a slice without blocks: the planner leaves none, the epilogue would read its slots)
    for (cp = 0; cp < (uint32_t)S.npass; cp++)
      for (ct = 0; ct < nt; ct++) finish();
    return;
  }
  while (remaining > 2) {   // steady state: every issue / consume is unconditional
    issue(Bq);
    consume(A);
    issue(A);
    consume(Bq);
    remaining -= 2;
  }
  if (remaining == 2) {
    issue(Bq);
    consume(A);
    consume(Bq);
  } else {
    consume(A);
  }
}

// BF16: the launch's matrices are kDevBF16_T16 (else kDevF16_T16).  16 waves at <= 128 VGPRs: 4 waves per SIMD.
template <bool BF16>
__global__ void __launch_bounds__(1024) LGH_NO_PK_F32 mvh_kernel(const MvLaunch L) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* red = smem;
  float* ssq = red + L.red_floats;
  float* xs = ssq + 16;
  int s = 0;
  const uint32_t bid = blockIdx.x;
  if (L.nseg > 1 && bid >= L.seg[1].wg_begin) s = 1;
  if (L.nseg > 2 && bid >= L.seg[2].wg_begin) s = 2;
  const MvSeg& S = L.seg[s];
  const uint32_t wg = bid - S.wg_begin;
  mvh_rows<BF16>(L, S, wg, xs, red, ssq);
  __syncthreads();
  mv_epilogue(L, S, wg, red, ssq, S.T);
  if (L.amax_v) {
    // greedy decode (a single EPI_STORE segment, host-checked): this workgroup's (maximum, last index of the maximum) over its
    // own rows — the logits its threads just wrote, thread t row t; the staged x is dead by now
    const uint32_t t = threadIdx.x, row = wg * S.rows_per_wg + t;
    const bool has = t < S.rows_per_wg && row < S.n_rows;
    float bv = has ? S.out[row] : -INFINITY;
    int bi = has ? (int)row : -1;
    amax_block_reduce(bv, bi, xs, reinterpret_cast<int*>(xs + 16));
    if (t == 0) { L.amax_v[bid] = bv; L.amax_i[bid] = bi; }
  }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// Geometry for one weight shape: one workgroup per CU owning `tiles` consecutive row tiles of the launch's rows / 16 / 256; G = the
// largest divisor of that up to 16 (every group walks the same number of tiles), T = the k-slices the remaining waves allow.
hipError_t mvh_plan(uint32_t k, uint32_t n_rows, int npass, MvPlan* plan, uint32_t launch_rows) {
  if (k == 0 || k % 256 || n_rows == 0 || npass < 1 || npass > 4) return hipErrorInvalidValue;
  const uint32_t nblk = k / 256;
  if (launch_rows < n_rows) launch_rows = n_rows;
  const uint32_t tiles = std::max(1u, ((launch_rows + 15) / 16 + kNumCU - 1) / kNumCU);
  uint32_t G = 1;
  for (uint32_t g = 2; g <= 16 && g <= tiles; g++)
    if (tiles % g == 0) G = g;
  uint32_t T = std::min(16u / G, nblk);
  const uint32_t bps = (nblk + T - 1) / T;
  T = (nblk + bps - 1) / bps;                       // no slice without blocks
  const uint32_t tpg = std::min(tiles / G, 4 * T);  // the epilogue runs one thread per row: rows_per_wg <= threads
  plan->units = nblk;
  plan->T = T;
  plan->G = G;
  plan->rows_per_wg = 16 * G * tpg;
  plan->n_wg = (n_rows + plan->rows_per_wg - 1) / plan->rows_per_wg;
  plan->threads = T * G * 64;
  plan->red_floats = (uint32_t)npass * T * plan->rows_per_wg;
  return hipSuccess;
}

static size_t mvh_lds_bytes(const MvLaunch& L) {
  uint32_t nx = 1;
  for (int s = 0; s < L.nseg; s++)
    if (L.seg[s].npass > 1 && L.seg[s].pass[1].x != L.seg[s].pass[0].x) nx = std::max(nx, (uint32_t)L.seg[s].npass);
  return ((size_t)nx * L.k + L.red_floats + 16) * sizeof(float);
}

template <bool BF16>
static hipError_t mvh_go(const MvLaunch& L, uint32_t n_wg, uint32_t threads, size_t lds, hipStream_t st) {
  static bool attr_set[64] = {};  // > 64 KB of dynamic LDS needs the opt-in once per kernel and device
  if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(&mvh_kernel<BF16>), 160 * 1024, attr_set); e != hipSuccess) return e;
  hipLaunchKernelGGL((mvh_kernel<BF16>), dim3(n_wg), dim3(threads), lds, st, L);
  return hipGetLastError();
}

// *amax_done: the launch left the arg-max parts L.amax_v asks for (one EPI_STORE segment, at most kAmaxPartsMax workgroups)
hipError_t mvh_launch(const MvLaunch& L0, uint32_t n_wg, uint32_t threads, hipStream_t st, bool* amax_done) {
  MvLaunch L = L0;
  if (amax_done) *amax_done = false;
  if (L.nseg < 1 || L.nseg > 3 || n_wg == 0 || threads == 0 || threads > 1024 || L.k % 256) return hipErrorInvalidValue;
  for (int s = 0; s < L.nseg; s++) {
    const MvSeg& S = L.seg[s];
    if (!half_type(S.type) || S.type != L.seg[0].type || S.rows_per_wg % (16 * S.G) || S.rows_per_wg > threads || S.T * S.G * 64 > threads ||
        S.nblk != L.k / 256)
      return hipErrorInvalidValue;
  }
  // (the prologue's sum of squares is one vector's: no norm over passes with input vectors of their own — no caller asks for one)
  if (L.do_norm && mvh_lds_bytes(L) != ((size_t)L.k + L.red_floats + 16) * sizeof(float)) return hipErrorInvalidValue;
  const bool want_amax = L.amax_v && L.amax_i && L.nseg == 1 && L.seg[0].epi == EPI_STORE && n_wg <= kAmaxPartsMax;
  if (!want_amax) L.amax_v = nullptr;
  const size_t lds = mvh_lds_bytes(L);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  const hipError_t e = L.seg[0].type == kDevBF16_T16 ? mvh_go<true>(L, n_wg, threads, lds, st) : mvh_go<false>(L, n_wg, threads, lds, st);
  if (amax_done) *amax_done = want_amax && e == hipSuccess;
  return e;
}

}  // namespace lgh
