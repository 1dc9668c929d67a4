// matvec_batch_f32.hip — the multi-sequence mat-vec on the f32 matrix cores (v_mfma_f32_16x16x4_f32): mvqf_kernel, the first launch
// of an op on contexts that asked for it (lgh_set_batch_policy: LGH_BATCH_F32_MATRIX) from the policy's minimum sequence count on.
//
// Why.  mvqb2 (matvec_batch.hip) keeps every sequence bit-identical to the single-sequence engine: per (tile, sequence) four int8
// MFMAs whose A operand is 3/4 zeros plus ~42 vector instructions of limb recombination, so a step's cost grows with its sequences
// and the vector port is full.  Here the sequences are the N dimension of the matrix instruction: one 16-row x 256-element tile is
// dequantized ONCE to f32 and multiplied with all 16 sequences in 64 MFMAs, whatever the sequence count; nothing is done per
// sequence.  f32 x f32 -> f32: no narrower than the reference's arithmetic, but not the single-sequence engine's bits.
//
// Work split: mvqb2's, so that its second launch (mvqb2_epilogue_kernel) runs behind this kernel as it stands.  A workgroup = 8 waves
// = 8 units (a unit = one row tile of one pass) over one range of k blocks; on the SEQ grid a workgroup walks every block of its
// units (nslots = 1), otherwise blockIdx.y is the k-slice (nslots = T).  MvBatch::part is written in mvqb2's layout,
// [slot][sequence][unit * 16 + row].
//
// Operands.  M = the tile's 16 weight rows, N = 16 sequences, K = 4.  In the tile16 layouts lane 16c + n owns the 16 quants of
// k-chunk c of step pp of row n, so the K index c of MFMA t (0..15) of step pp is element 64pp + 16c + t: a lane's A operand is its
// own t-th weight (no cross-lane movement), its B operand x[sequence = lane & 15][64pp + 16c + t].  64 MFMAs per tile accumulate in
// a lane's 4 D registers (rows 4 * (lane >> 4) + r, sequence lane & 15) across all blocks of the workgroup's range; there is no
// per-tile vector finish and no cross-lane reduction.
//
// Weights.  mvq_issue_tile / mvq_unpack_tile unchanged (same loads, same non-temporal hint, next tile in flight while this one is
// used).  Per (row, sub-block) factors once per tile, then per weight one v_cvt_f32_ubyte and one fma:
//   Q4_K, Q5_K  w = fma(q, d * sc, -(dmin * mn))      Q6_K  w = fma(q', d * sc, -32 * d * sc) = round(d * sc * (q' - 32))
//   Q4_0        w = fma(q, d, -8 * d)                 Q8_0  w = fma(q ^ 0x80, d, -128 * d)    = round(d * q)
//   Q2_K        as Q4_K, one (sc, mn) per chunk       Q3_K  w = fma(q, d * sc, -4 * d * sc)   = round(d * sc * (q - 4))
//   Q4_1, Q5_1  w = fma(q, d, m)                      Q5_0  w = fma(q, d, -16 * d)            = round(d * (q - 16))
//   IQ4_NL, IQ4_XS  as Q8_0 over the decoded codebook bytes, d resp. d * (ls - 32) for d: w = round(d * kv[q])
//
// Activations.  Plain f32: x[s][.] * norm_w[.] (the product the XQ producers round; x alone without a norm) staged per chunk of
// kXfCb blocks for all sequences in LDS, double-buffered with one barrier per chunk; rows of sequences >= n_seq are zero.  A
// sequence's row is kXfCb * 1024 + 16 bytes long: the 16 sequences of a ds_read_b128 fall into 16 different 16-byte bank groups (a
// stride of 1024 B would put them all in one).  A lane reads its 16 consecutive floats of a step with four 16-byte reads.
//
// Not taken (mvqb_launch): one sequence, fewer sequences than the policy's minimum, launches whose segments do not share their
// input, indirect (MoE expert) launches and launches that fall back for a short partial buffer keep mvqb / mvqb2.
#include "device_utils.h"
#include "mvq_core.h"

namespace lgh {

constexpr int kFWaves = 8;
constexpr uint32_t kXfCb = 2;                          // blocks staged per chunk
constexpr uint32_t kXfRow = kXfCb * 256 + 4;           // floats per sequence row in LDS (+16 B: the bank spread)
constexpr uint32_t kXfBuf = 16 * kXfRow;               // floats per half of the two-deep buffer
constexpr uint32_t kXfPieces = kXfCb * 64 * 16 / (kFWaves * 64);   // 16-byte pieces per thread and chunk

template <uint32_t MASK, bool SEQ>
__global__ void __launch_bounds__(kFWaves * 64) __attribute__((amdgpu_waves_per_eu(4, 4)))
mvqf_kernel(const Mvqb2Geom Gm, const MvLaunch L, const MvBatch B, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float xsm[];   // [2][16][kXfRow]
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t n_seq = B.n_seq;
  const uint32_t u = blockIdx.x * kFWaves + wave;                 // this wave's unit
  const bool active = u < Gm.n_units;
  const int sg = (int)(u >= Gm.ub1) + (int)(u >= Gm.ub2);
  const MvSeg& S = L.seg[active ? sg : 0];
  constexpr bool kSingle = (MASK & (MASK - 1)) == 0;
  const int fmt = kSingle ? __builtin_ctz(MASK) : fmt_of_dev_type(S.type);
  auto is = [&](int f) { return mvq_is<MASK>(fmt, f); };
  const uint32_t tb = mvq_tile_stride<MASK>(fmt);
  const uint32_t ntiles = (S.n_rows + 15) >> 4;
  const uint32_t ul = u - (sg == 0 ? 0u : sg == 1 ? Gm.ub1 : Gm.ub2);
  const uint32_t pass = active ? ul / ntiles : 0, tl = active ? ul - pass * ntiles : 0;
  const uint8_t* wbase = (pass == 0 ? S.pass[0].plane[0] : S.pass[1].plane[0]) + (size_t)tl * Gm.nblk * tb;
  const float* xg = L.seg[0].pass[0].x;                           // sequence 0's vector (all segments and passes share the input)
  const float* nw = L.do_norm ? L.norm_w : nullptr;
  const uint32_t sq = lane & 15, c = lane >> 4;

  // this workgroup's blocks: all of them (SEQ), or k-slice blockIdx.y's (possibly none: its partial sums are zeros)
  const uint32_t b_begin = SEQ ? 0u : min(blockIdx.y * Gm.nbw, Gm.nblk);
  const uint32_t b_end = SEQ ? Gm.nblk : min(b_begin + Gm.nbw, Gm.nblk);

  // rows of sequences the launch does not have: zero in both halves, once
  for (uint32_t i = tid; i < (16 - n_seq) * (kXfRow / 4) * 2; i += kFWaves * 64) {
    const uint32_t h = i / ((16 - n_seq) * (kXfRow / 4)), j = i - h * (16 - n_seq) * (kXfRow / 4);
    *reinterpret_cast<f32x4*>(xsm + h * kXfBuf + n_seq * kXfRow + j * 4) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  RawT16 nxt;
  if (active && b_begin < b_end) mvq_issue_tile<MASK>(fmt, wbase + (size_t)b_begin * tb, lane, nxt);

  // ---- staging: chunk i + 1 is fetched into registers while chunk i is computed, and stored (times the norm weights) into the
  // other half at the next barrier.  Piece i of a chunk of cn blocks = 4 floats at offset (i % P) * 4 of sequence i / P, P = cn * 64;
  // a thread's pieces lie 512 apart, i.e. at the same offset of different sequences: one norm-weight piece serves them all
  f32x4 stg[kXfPieces], nwv = {1.0f, 1.0f, 1.0f, 1.0f};
  auto fetch = [&](uint32_t b0, uint32_t cn) {
    const uint32_t P = cn * 64, off = tid & (P - 1);
#pragma unroll
    for (uint32_t j = 0; j < kXfPieces; j++) {
      const uint32_t s = (tid + j * kFWaves * 64) / P;
      if (s < n_seq) stg[j] = *reinterpret_cast<const f32x4*>(xg + (size_t)s * B.x_stride + (size_t)b0 * 256 + off * 4);
    }
    if (nw) nwv = *reinterpret_cast<const f32x4*>(nw + (size_t)b0 * 256 + off * 4);
  };
  auto stash = [&](uint32_t cn, uint32_t buf) {
    const uint32_t P = cn * 64, off = tid & (P - 1);
#pragma unroll
    for (uint32_t j = 0; j < kXfPieces; j++) {
      const uint32_t s = (tid + j * kFWaves * 64) / P;
      if (s < n_seq) *reinterpret_cast<f32x4*>(xsm + buf * kXfBuf + s * kXfRow + off * 4) = stg[j] * nwv;
    }
  };

  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t b0 = b_begin, buf = 0;
  if (b0 < b_end) fetch(b0, min(kXfCb, b_end - b0));
  while (b0 < b_end) {
    const uint32_t cn = min(kXfCb, b_end - b0);
    stash(cn, buf);
    __syncthreads();
    const uint32_t nb0 = b0 + cn;
    if (nb0 < b_end) fetch(nb0, min(kXfCb, b_end - nb0));
    if (active) {
      for (uint32_t bi = 0; bi < cn; bi++) {
        const RawT16 cur = nxt;
        const uint32_t bn = b0 + bi + 1;                          // the unit's next tile
        if (bn < b_end) mvq_issue_tile<MASK>(fmt, wbase + (size_t)bn * tb, lane, nxt);
        TileOps t;
        mvq_unpack_tile<MASK>(fmt, cur, lane, t);
        // w = fma(q, sa, sb) per step: the (row, sub-block) factors
        float sa[4], sb[4];
#pragma unroll
        for (int pp = 0; pp < 4; pp++) {
          if (is(F_Q6K)) { sa[pp] = t.dd * t.f[pp]; sb[pp] = -32.0f * sa[pp]; }
          else if (is(F_Q80) || is(F_IQ4NL)) { sa[pp] = t.f[pp]; sb[pp] = -128.0f * sa[pp]; }
          else if (is(F_IQ4XS)) { sa[pp] = t.dd * t.f[pp]; sb[pp] = -128.0f * sa[pp]; }
          else if (is(F_Q40)) { sa[pp] = t.f[pp]; sb[pp] = -8.0f * sa[pp]; }
          else if (is(F_Q3K)) { sa[pp] = t.dd * t.f[pp]; sb[pp] = -4.0f * sa[pp]; }
          else if (is(F_Q50)) { sa[pp] = t.f[pp]; sb[pp] = -16.0f * sa[pp]; }
          else if (is(F_Q41) || is(F_Q51)) { sa[pp] = t.f[pp]; sb[pp] = t.g[pp]; }
          else { sa[pp] = t.dd * t.f[pp]; sb[pp] = -(t.dmin * t.g[pp]); }
        }
        const float* xrow = xsm + buf * kXfBuf + sq * kXfRow + bi * 256 + c * 16;
#pragma unroll
        for (int pp = 0; pp < 4; pp++) {
          f32x4 xv[4];
#pragma unroll
          for (int j = 0; j < 4; j++) xv[j] = *reinterpret_cast<const f32x4*>(xrow + pp * 64 + j * 4);
#pragma unroll
          for (int j = 0; j < 4; j++) {
            uint32_t qw = (uint32_t)t.bw[pp][j];
            if (is(F_Q80) || is(F_IQ4NL) || is(F_IQ4XS)) qw ^= 0x80808080u;   // int8 quants as bytes biased by 128
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_fmaf(ub0(qw), sa[pp], sb[pp]), xv[j].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_fmaf(ub1(qw), sa[pp], sb[pp]), xv[j].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_fmaf(ub2(qw), sa[pp], sb[pp]), xv[j].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_fmaf(ub3(qw), sa[pp], sb[pp]), xv[j].w, acc, 0, 0, 0);
          }
        }
      }
    }
    b0 = nb0; buf ^= 1u;
  }
  if (active && sq < n_seq) {   // D: rows 4c .. 4c + 3 of the unit, sequence sq
    const uint32_t slot = SEQ ? 0u : blockIdx.y;
    const size_t rows16 = (size_t)Gm.n_units * 16;
    *reinterpret_cast<f32x4*>(part + ((size_t)slot * n_seq + sq) * rows16 + (size_t)u * 16 + c * 4) = acc;
  }
}

size_t mvqf_lds_bytes() { return (size_t)2 * kXfBuf * 4; }

template <uint32_t MASK>
static hipError_t mvqf_go(const Mvqb2Geom& Gm, const MvLaunch& L, const MvBatch& B, bool seq, uint32_t groups, hipStream_t st) {
  static bool attr_set[2][64] = {};
  const size_t lds = mvqf_lds_bytes();
  if (seq) {
    if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(&mvqf_kernel<MASK, true>), 160 * 1024, attr_set[0]); e != hipSuccess) return e;
    hipLaunchKernelGGL((mvqf_kernel<MASK, true>), dim3(groups), dim3(kFWaves * 64), lds, st, Gm, L, B, B.part);
  } else {
    if (hipError_t e = lds_opt_in(reinterpret_cast<const void*>(&mvqf_kernel<MASK, false>), 160 * 1024, attr_set[1]); e != hipSuccess) return e;
    hipLaunchKernelGGL((mvqf_kernel<MASK, false>), dim3(groups, Gm.T), dim3(kFWaves * 64), lds, st, Gm, L, B, B.part);
  }
  return hipGetLastError();
}

// the first launch of an op of `mask`'s formats; mvqb_launch (matvec_batch.hip) puts mvqb2's epilogue launch behind it
hipError_t mvqf_launch(uint32_t mask, const Mvqb2Geom& Gm, const MvLaunch& L, const MvBatch& B, bool seq, uint32_t groups, hipStream_t st) {
  if (B.ind_cnt || !B.part || !L.seg[0].pass[0].x || B.n_seq == 0 || B.n_seq > 16u || B.x_stride < L.k || L.k != Gm.nblk * 256u)
    return hipErrorInvalidValue;
#define LGH_MVQF_CASE(M) case M: return mvqf_go<M>(Gm, L, B, seq, groups, st)
  switch (mask) {
    LGH_MVQF_CASE(1u << F_Q4K); LGH_MVQF_CASE(1u << F_Q6K); LGH_MVQF_CASE(1u << F_Q5K); LGH_MVQF_CASE(1u << F_Q80); LGH_MVQF_CASE(1u << F_Q40);
    LGH_MVQF_CASE(1u << F_Q3K); LGH_MVQF_CASE(1u << F_Q2K);
    LGH_MVQF_CASE(1u << F_Q41); LGH_MVQF_CASE(1u << F_Q50); LGH_MVQF_CASE(1u << F_Q51);
    LGH_MVQF_CASE(1u << F_IQ4NL); LGH_MVQF_CASE(1u << F_IQ4XS);
    LGH_MVQF_CASE((1u << F_Q4K) | (1u << F_Q6K)); LGH_MVQF_CASE((1u << F_Q5K) | (1u << F_Q6K));
    default: return hipErrorInvalidValue;
  }
#undef LGH_MVQF_CASE
}

}  // namespace lgh
