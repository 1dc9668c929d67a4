// mvq_core.h — the tile-level core of the int8 matrix-core mat-vec (internal, device side): how one 16-row x 256-element
// weight tile is requested from HBM and how it is multiplied with the XQ record of its 256 input elements.  Shared by
// the launch-per-op kernel (matvec_mfma.hip: mvq_kernel) and the persistent token kernel (decode_persistent.hip), so both
// produce the same bits for the same tile.  Formats, tile layouts and the arithmetic are described in matvec_mfma.hip.
#pragma once

#include "device_utils.h"
#include "xq.h"

namespace lgh {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kTileBytes = 2304;      // Q4_K tile16
constexpr int kTileBytesQ6 = 3392;    // Q6_K tile16
// formats of the matrix-core mat-vec; a kernel instantiation handles the formats in its MASK (bit = 1 << format)
enum : int { F_Q4K = 0, F_Q6K = 1, F_Q5K = 2, F_Q80 = 3, F_Q40 = 4, F_Q3K = 5, F_Q2K = 6, F_Q41 = 7, F_Q50 = 8, F_Q51 = 9, F_IQ4NL = 10,
              F_IQ4XS = 11, F_COUNT = 12 };
constexpr uint32_t kLowbitMask = (1u << F_Q3K) | (1u << F_Q2K);   // instantiations that hold one of these are the *_lowbit_kernel twins
constexpr uint32_t kLegacyMask = (1u << F_Q41) | (1u << F_Q50) | (1u << F_Q51);   // ... and of these the *_legacy_kernel ones
constexpr uint32_t kIq4Mask = (1u << F_IQ4NL) | (1u << F_IQ4XS);                 // ... and of these the *_iq4_kernel ones
__host__ __device__ constexpr uint32_t fmt_tile_bytes(int f) {   // = 16 rows x the GGUF bytes of 256 elements (Q6_K: +32 pad; Q3_K: 114 per row)
  return f == F_Q4K ? 2304u : f == F_Q6K ? 3392u : f == F_Q5K ? 2816u : f == F_Q80 ? 4352u : f == F_Q3K ? 1824u : f == F_Q2K ? 1344u
         : f == F_Q41 ? 2560u : f == F_Q50 ? 2816u : f == F_Q51 ? 3072u : f == F_IQ4XS ? 2176u : 2304u;   // (Q4_0, IQ4_NL: 2304)
}
__host__ __device__ constexpr int fmt_loads_per_tile(int f) {
  return f == F_Q4K ? 3 : f == F_Q6K ? 5 : f == F_Q5K ? 4 : f == F_Q80 ? 5 : f == F_Q3K ? 4 : f == F_Q41 ? 4 : f == F_Q50 ? 4 : f == F_Q51 ? 5 : 3;   // (IQ4_NL, IQ4_XS: 3)
}
__host__ __device__ constexpr int fmt_of_dev_type(int t) {
  return t == kDevQ4K_T16 ? F_Q4K : t == kDevQ6K_T16 ? F_Q6K : t == kDevQ5K_T16 ? F_Q5K : t == kDevQ80_T16 ? F_Q80 : t == kDevQ40_T16 ? F_Q40
         : t == kDevQ3K_T16 ? F_Q3K : t == kDevQ2K_T16 ? F_Q2K : t == kDevQ41_T16 ? F_Q41 : t == kDevQ50_T16 ? F_Q50 : t == kDevQ51_T16 ? F_Q51
         : t == kDevIQ4NL_T16 ? F_IQ4NL : t == kDevIQ4XS_T16 ? F_IQ4XS : -1;
}


struct RawT16 { u32x4 hd; u32x4 q[4]; };   // one tile in flight: header / scales + up to four 16-byte payload loads per lane

// `fmt` is only read when MASK holds more than one format (otherwise the format is a compile-time constant)
template <uint32_t MASK>
__device__ __forceinline__ bool mvq_is(int fmt, int f) {
  constexpr bool kSingle = (MASK & (MASK - 1)) == 0;
  return ((MASK >> f) & 1u) != 0 && (kSingle || fmt == f);
}

// bytes of one tile of the segment's format (a constant in a single-format instantiation)
template <uint32_t MASK>
__device__ __forceinline__ uint32_t mvq_tile_stride(int fmt) {
  auto is = [&](int f) { return mvq_is<MASK>(fmt, f); };
  return is(F_Q4K) ? fmt_tile_bytes(F_Q4K) : is(F_Q6K) ? fmt_tile_bytes(F_Q6K) : is(F_Q5K) ? fmt_tile_bytes(F_Q5K) : is(F_Q80) ? fmt_tile_bytes(F_Q80)
         : is(F_Q3K) ? fmt_tile_bytes(F_Q3K) : is(F_Q2K) ? fmt_tile_bytes(F_Q2K) : is(F_Q41) ? fmt_tile_bytes(F_Q41)
         : is(F_Q50) ? fmt_tile_bytes(F_Q50) : is(F_Q51) ? fmt_tile_bytes(F_Q51) : is(F_IQ4XS) ? fmt_tile_bytes(F_IQ4XS) : fmt_tile_bytes(F_Q40);
}

// The two low-bit K-quants (tile layouts: matvec_mfma.hip).  r.q[0] dword pp: the lane's 16 two-bit quants of step pp, byte t = q[t] |
// q[t+4] << 2 | q[t+8] << 4 | q[t+12] << 6, so B-operand dword j (elements 4j .. 4j+3) is one shift and one mask; Q3_K's third bits
// (r.q[1].x / .y: a dword per step pair, low nibbles = even step, high nibbles = odd step, byte t = f[t] | f[t+4] << 1 | f[t+8] << 2 |
// f[t+12] << 3) complete it to q = lo2 | hi1 << 2 (0..7; the reference's "- 4" goes through the chunk's sum of x).
template <bool Q3>
__device__ __forceinline__ i32x4 mvq_lowbit_operand(const RawT16& r, int pp) {
  const uint32_t w = pp == 0 ? r.q[0].x : pp == 1 ? r.q[0].y : pp == 2 ? r.q[0].z : r.q[0].w;
  i32x4 bw;
  bw.x = (int)(w & 0x03030303u);
  bw.y = (int)((w >> 2) & 0x03030303u);
  bw.z = (int)((w >> 4) & 0x03030303u);
  bw.w = (int)((w >> 6) & 0x03030303u);
  if (Q3) {
    const uint32_t H = ((pp >> 1) ? r.q[1].y : r.q[1].x) >> (4 * (pp & 1));
    bw.x |= (int)((H & 0x01010101u) << 2);
    bw.y |= (int)(((H >> 1) & 0x01010101u) << 2);
    bw.z |= (int)(((H >> 2) & 0x01010101u) << 2);
    bw.w |= (int)(((H >> 3) & 0x01010101u) << 2);
  }
  return bw;
}

// The three 32-element-block formats with an additive minimum and / or a fifth bit: Q4_1, Q5_0, Q5_1 (tile layouts: matvec_mfma.hip).
// Nibble words r.q[0] / r.q[1] as Q4_0's; with FIFTH the fifth bits (r.q[2].x / .y, stored as Q5_K's: a dword per step pair, low nibbles =
// even step, high nibbles = odd step, byte t = f[t] | f[t+4] << 1 | f[t+8] << 2 | f[t+12] << 3) complete B-operand dword j to q = nibble |
// fifth << 4 (0..31).  Q5_0's "- 16" and the minima of Q4_1 / Q5_1 go through the chunk's sum of x.
template <bool FIFTH>
__device__ __forceinline__ i32x4 mvq_legacy_operand(const RawT16& r, int pp) {
  const uint32_t N0 = (pp & 1) ? r.q[pp >> 1].z : r.q[pp >> 1].x, N1 = (pp & 1) ? r.q[pp >> 1].w : r.q[pp >> 1].y;
  i32x4 bw;
  bw.x = (int)(N0 & 0x0F0F0F0Fu);
  bw.y = (int)((N0 >> 4) & 0x0F0F0F0Fu);
  bw.z = (int)(N1 & 0x0F0F0F0Fu);
  bw.w = (int)((N1 >> 4) & 0x0F0F0F0Fu);
  if (FIFTH) {
    const uint32_t H = ((pp >> 1) ? r.q[2].y : r.q[2].x) >> (4 * (pp & 1));
    bw.x |= (int)((H & 0x01010101u) << 4);
    bw.y |= (int)(((H >> 1) & 0x01010101u) << 4);
    bw.z |= (int)(((H >> 2) & 0x01010101u) << 4);
    bw.w |= (int)(((H >> 3) & 0x01010101u) << 4);
  }
  return bw;
}
// the f16 of block 2pp + (c >> 1) out of a row's eight (one dword per step: blocks 2pp, 2pp + 1)
__device__ __forceinline__ float mvq_block_f16(const u32x4& h, int pp, uint32_t c) {
  const uint32_t w = pp == 0 ? h.x : pp == 1 ? h.y : pp == 2 ? h.z : h.w;
  return h2f((c >> 1) ? w >> 16 : w & 0xFFFFu);
}

// The two non-linear 4-bit formats, IQ4_NL and IQ4_XS (tile layouts: matvec_mfma.hip).  Nibble words r.q[0] / r.q[1] as Q4_0's; a nibble
// is an index into the 16-entry codebook kv = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113}, whose entries
// are signed int8: the decoded byte IS the B-operand byte, as Q8_0's quants are — no offset, no minimum.  The lookup is done in registers
// (iq4_decode4, device_utils.h): about 6 vector operations per operand dword against Q4_0's 2.
__device__ __forceinline__ i32x4 mvq_iq4_operand(const RawT16& r, int pp) {
  const uint32_t N0 = (pp & 1) ? r.q[pp >> 1].z : r.q[pp >> 1].x, N1 = (pp & 1) ? r.q[pp >> 1].w : r.q[pp >> 1].y;
  i32x4 bw;
  bw.x = (int)iq4_decode4(N0 & 0x0F0F0F0Fu);
  bw.y = (int)iq4_decode4((N0 >> 4) & 0x0F0F0F0Fu);
  bw.z = (int)iq4_decode4(N1 & 0x0F0F0F0Fu);
  bw.w = (int)iq4_decode4((N1 >> 4) & 0x0F0F0F0Fu);
  return bw;
}
// IQ4_XS: ls - 32 of sub-block ib = 2pp + (c >> 1), the sub-block of chunk 4pp + c; hd.x = d | scales_h << 16, hd.y = scales_l[0..3]
// (ls = (scales_l[ib / 2] >> 4 (ib % 2) & 15) | (scales_h >> 2 ib & 3) << 4, iq_quants.rs:86-89)
__device__ __forceinline__ float mvq_iq4xs_scale(const u32x4& hd, int pp, uint32_t c) {
  const uint32_t h = c >> 1;
  const uint32_t ls = ((hd.y >> (8 * pp + 4 * h)) & 15u) | (((hd.x >> (16 + 4 * pp + 2 * h)) & 3u) << 4);
  return (float)((int)ls - 32);
}

// fmt_loads_per_tile(format) non-temporal loads of this lane's share of the tile at `tile` (lane roles: row n = lane & 15)
template <uint32_t MASK>
__device__ __forceinline__ void mvq_issue_tile(int fmt, const uint8_t* tile, uint32_t lane, RawT16& r) {
  const uint32_t n = lane & 15;
  auto is = [&](int f) { return mvq_is<MASK>(fmt, f); };
    if (is(F_Q6K)) {
      r.hd = ldg_nt128(tile + 3072 + n * 16);
#pragma unroll
      for (int i = 0; i < 3; i++) r.q[i] = ldg_nt128(tile + i * 1024 + lane * 16);
      r.q[3].x = ldg_nt32(tile + 3328 + (n >> 1) * 4);
    } else if (is(F_Q80)) {
      r.hd = ldg_nt128(tile + 4096 + n * 16);
#pragma unroll
      for (int i = 0; i < 4; i++) r.q[i] = ldg_nt128(tile + i * 1024 + lane * 16);
    } else if (is(F_Q3K)) {   // two-bit words, third bits, the lane's four int8 scales, the row pair's d
      r.q[0] = ldg_nt128(tile + lane * 16);
      const u32x2 h = ldg_nt64(tile + 1024 + lane * 8);
      r.q[1].x = h.x;
      r.q[1].y = h.y;
      r.hd.x = ldg_nt32(tile + 1536 + lane * 4);
      r.hd.y = ldg_nt32(tile + 1792 + (n >> 1) * 4);
    } else if (is(F_Q2K)) {   // two-bit words, the lane's four scale | min << 4 bytes, the row's d | dmin
      r.q[0] = ldg_nt128(tile + lane * 16);
      r.hd.x = ldg_nt32(tile + 1024 + lane * 4);
      r.hd.y = ldg_nt32(tile + 1280 + n * 4);
    } else if (is(F_Q41) || is(F_Q50) || is(F_Q51)) {   // the row's eight d, two nibble loads, then the row's eight m and / or the fifth bits
      r.hd = ldg_nt128(tile + 2048 + n * 16);
      r.q[0] = ldg_nt128(tile + lane * 16);
      r.q[1] = ldg_nt128(tile + 1024 + lane * 16);
      if (!is(F_Q50)) r.q[3] = ldg_nt128(tile + 2304 + n * 16);
      if (!is(F_Q41)) {
        const u32x2 h = ldg_nt64(tile + (is(F_Q50) ? 2304 : 2560) + lane * 8);
        r.q[2].x = h.x;
        r.q[2].y = h.y;
      }
    } else if (is(F_IQ4XS)) {   // the row's native 8-byte header {d, scales_h, scales_l[4]}, two nibble loads
      const u32x2 h = ldg_nt64(tile + 2048 + n * 8);
      r.hd.x = h.x;
      r.hd.y = h.y;
      r.q[0] = ldg_nt128(tile + lane * 16);
      r.q[1] = ldg_nt128(tile + 1024 + lane * 16);
    } else {   // Q4_K, Q5_K, Q4_0, IQ4_NL: header + two nibble loads (+ the fifth bits)
      r.hd = ldg_nt128(tile + 2048 + n * 16);
      r.q[0] = ldg_nt128(tile + lane * 16);
      r.q[1] = ldg_nt128(tile + 1024 + lane * 16);
      if (is(F_Q5K)) {
        const u32x2 h = ldg_nt64(tile + 2304 + lane * 8);
        r.q[2].x = h.x;
        r.q[2].y = h.y;
      }
    }
}

// acc += (weight rows n of the tile) . (the 256 elements of XQ record `rec`, in LDS), this lane's k-chunk c = lane >> 4 only:
// four MFMAs (one per 64 elements); lane group c then holds, for weight row n, the four limb sums of chunk 4pp + c,
// recombined to V = sum_k q_k * I_k (exact int, rounded once to f32).
template <uint32_t MASK>
__device__ __forceinline__ void mvq_consume_tile(int fmt, const RawT16& r, const uint8_t* rec, uint32_t lane, float& acc) {
  const uint32_t n = lane & 15, c = lane >> 4;
  const bool a_valid = (n >> 2) == c;
  const uint32_t a_off = (c >> 1) * 128 + (n & 3) * 32 + (c & 1) * 16;   // + 2p * 128
  auto is = [&](int f) { return mvq_is<MASK>(fmt, f); };
    i32x4 areg[4];
#pragma unroll
    for (int pp = 0; pp < 4; pp++) {
      i32x4 t = {0, 0, 0, 0};
      if (a_valid) t = *reinterpret_cast<const i32x4*>(rec + pp * 256 + a_off);
      areg[pp] = t;
    }
    const f32x4 xs = *reinterpret_cast<const f32x4*>(rec + kXqXs16 + c * 16);   // sum of x over chunk 4pp + c
    const f32x4 sx = *reinterpret_cast<const f32x4*>(rec + kXqSx16 + c * 16);   // its scale * 2^-30
    if (is(F_Q6K)) {
      const uint32_t s8 = c * 8;
      const uint32_t hdw[4] = {r.hd.x, r.hd.y, r.hd.z, r.hd.w};   // int8 scales 4pp .. 4pp+3 of row n (dequant.rs:343-350)
      float s1 = 0.0f;
#pragma unroll
      for (int pp = 0; pp < 4; pp++) {
        const uint32_t N0 = (pp & 1) ? r.q[pp >> 1].z : r.q[pp >> 1].x, N1 = (pp & 1) ? r.q[pp >> 1].w : r.q[pp >> 1].y;
        const uint32_t H = pp == 0 ? r.q[2].x : pp == 1 ? r.q[2].y : pp == 2 ? r.q[2].z : r.q[2].w;
        i32x4 bw;   // q' = ql | qh << 4, 0..63; the reference's "- 32" is applied through the chunk's sum of x below
        bw.x = (int)((N0 & 0x0F0F0F0Fu) | ((H & 0x03030303u) << 4));
        bw.y = (int)(((N0 >> 4) & 0x0F0F0F0Fu) | (((H >> 2) & 0x03030303u) << 4));
        bw.z = (int)((N1 & 0x0F0F0F0Fu) | (((H >> 4) & 0x03030303u) << 4));
        bw.w = (int)(((N1 >> 4) & 0x0F0F0F0Fu) | (((H >> 6) & 0x03030303u) << 4));
        const i32x4 zero = {0, 0, 0, 0};
        const i32x4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(areg[pp], bw, zero, 0, 0, 0);
        // |D0| <= 64*63*16, so the high half is exact in f32; the low half may round at 2^-24 of a term that is 2^-16 of the sum
        const float hi = (float)((d.x << 8) + d.y), lo = (float)((d.z << 8) + d.w);
        const float V = __builtin_fmaf(hi, 65536.0f, lo);
        const float scf = (float)(int)__builtin_amdgcn_sbfe((int)hdw[pp], s8, 8);
        s1 = __builtin_fmaf(scf, __builtin_fmaf(sx[pp], V, -32.0f * xs[pp]), s1);
      }
      const uint32_t dh = (n & 1) ? r.q[3].x >> 16 : r.q[3].x & 0xFFFFu;
      acc = __builtin_fmaf(h2f(dh), s1, acc);
    } else if (is(F_Q80) || is(F_Q40)) {
      // 32-element blocks with one f16 scale: chunk 4pp + c lies in block 2pp + (c >> 1) of the row's eight
      const uint32_t hdw[4] = {r.hd.x, r.hd.y, r.hd.z, r.hd.w};
      float s1 = 0.0f;
#pragma unroll
      for (int pp = 0; pp < 4; pp++) {
        i32x4 bw;
        if (is(F_Q80)) {
          bw.x = (int)r.q[pp].x; bw.y = (int)r.q[pp].y; bw.z = (int)r.q[pp].z; bw.w = (int)r.q[pp].w;   // int8 quants as they are
        } else {
          const uint32_t N0 = (pp & 1) ? r.q[pp >> 1].z : r.q[pp >> 1].x, N1 = (pp & 1) ? r.q[pp >> 1].w : r.q[pp >> 1].y;
          bw.x = (int)(N0 & 0x0F0F0F0Fu);
          bw.y = (int)((N0 >> 4) & 0x0F0F0F0Fu);
          bw.z = (int)(N1 & 0x0F0F0F0Fu);
          bw.w = (int)((N1 >> 4) & 0x0F0F0F0Fu);
        }
        const i32x4 zero = {0, 0, 0, 0};
        const i32x4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(areg[pp], bw, zero, 0, 0, 0);
        const float hi = (float)((d.x << 8) + d.y), lo = (float)((d.z << 8) + d.w);
        const float V = __builtin_fmaf(hi, 65536.0f, lo);
        const float dd = h2f((c >> 1) ? hdw[pp] >> 16 : hdw[pp] & 0xFFFFu);
        // Q4_0: y = d * (q - 8) (dequant.rs:16-30); the offset goes through the chunk's sum of x
        s1 = __builtin_fmaf(dd, is(F_Q40) ? __builtin_fmaf(sx[pp], V, -8.0f * xs[pp]) : sx[pp] * V, s1);
      }
      acc += s1;
    } else if (is(F_Q3K)) {
      // y = d * (s6 - 32) * (q - 4), one scale per 16 elements = per chunk (dequant.rs:161-200): the Q6_K shape
      float s1 = 0.0f;
#pragma unroll
      for (int pp = 0; pp < 4; pp++) {
        const i32x4 zero = {0, 0, 0, 0};
        const i32x4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(areg[pp], mvq_lowbit_operand<true>(r, pp), zero, 0, 0, 0);
        // both halves exact in f32: every limb sum is at most 16 * 7 * 128
        const float hi = (float)((d.x << 8) + d.y), lo = (float)((d.z << 8) + d.w);
        const float V = __builtin_fmaf(hi, 65536.0f, lo);
        const float scf = (float)(int)__builtin_amdgcn_sbfe((int)r.hd.x, 8 * pp, 8);
        s1 = __builtin_fmaf(scf, __builtin_fmaf(sx[pp], V, -4.0f * xs[pp]), s1);
      }
      const uint32_t dh = (n & 1) ? r.hd.y >> 16 : r.hd.y & 0xFFFFu;
      acc = __builtin_fmaf(h2f(dh), s1, acc);
    } else if (is(F_Q2K)) {
      // y = d * sc * q - dmin * mn, a 4-bit (sc, mn) per chunk (dequant.rs:129-156): the Q4_K shape
      float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int pp = 0; pp < 4; pp++) {
        const i32x4 zero = {0, 0, 0, 0};
        const i32x4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(areg[pp], mvq_lowbit_operand<false>(r, pp), zero, 0, 0, 0);
        const float hi = (float)((d.x << 8) + d.y), lo = (float)((d.z << 8) + d.w);
        const float V = __builtin_fmaf(hi, 65536.0f, lo);
        const uint32_t sm = (r.hd.x >> (8 * pp)) & 0xFFu;
        s1 = __builtin_fmaf((float)(sm & 15u) * sx[pp], V, s1);
        s2 = __builtin_fmaf((float)(sm >> 4), xs[pp], s2);
      }
      const float dd = h2f(r.hd.y & 0xFFFFu), dmin = h2f(r.hd.y >> 16);
      acc += dd * s1 - dmin * s2;
    } else if (is(F_Q41) || is(F_Q50) || is(F_Q51)) {
      // 32-element blocks: chunk 4pp + c lies in block 2pp + (c >> 1) of the row's eight, whose f16 d (and m) it takes.
      // Q5_0: y = d * (q - 16) (dequant.rs:54-76), the Q4_0 shape; Q4_1 / Q5_1: y = d * q + m (dequant.rs:36-48, 81-101), the Q4_K shape
      // with a plus sign.  q <= 31: |D0| <= 64*31*16, |D1..3| <= 128*31*16 as for Q5_K, so both halves of V are exact in f32.
      float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int pp = 0; pp < 4; pp++) {
        const i32x4 bw = is(F_Q41) ? mvq_legacy_operand<false>(r, pp) : mvq_legacy_operand<true>(r, pp);
        const i32x4 zero = {0, 0, 0, 0};
        const i32x4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(areg[pp], bw, zero, 0, 0, 0);
        const float hi = (float)((d.x << 8) + d.y), lo = (float)((d.z << 8) + d.w);
        const float V = __builtin_fmaf(hi, 65536.0f, lo);
        const float dd = mvq_block_f16(r.hd, pp, c);
        if (is(F_Q50)) {
          s1 = __builtin_fmaf(dd, __builtin_fmaf(sx[pp], V, -16.0f * xs[pp]), s1);
        } else {
          s1 = __builtin_fmaf(dd * sx[pp], V, s1);
          s2 = __builtin_fmaf(mvq_block_f16(r.q[3], pp, c), xs[pp], s2);
        }
      }
      if (is(F_Q50)) acc += s1;
      else acc += s1 + s2;
    } else if (is(F_IQ4NL) || is(F_IQ4XS)) {
      // y = d * kv[q] (IQ4_NL, 32-element blocks: the Q8_0 shape) / d * (ls - 32) * kv[q] (IQ4_XS, a 6-bit scale per 32 elements: the
      // Q6_K shape without an offset), iq_quants.rs:66-99.  |kv| <= 127: the limb sums stay within Q8_0's.
      float s1 = 0.0f;
#pragma unroll
      for (int pp = 0; pp < 4; pp++) {
        const i32x4 zero = {0, 0, 0, 0};
        const i32x4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(areg[pp], mvq_iq4_operand(r, pp), zero, 0, 0, 0);
        const float hi = (float)((d.x << 8) + d.y), lo = (float)((d.z << 8) + d.w);
        const float V = __builtin_fmaf(hi, 65536.0f, lo);
        s1 = __builtin_fmaf(is(F_IQ4NL) ? mvq_block_f16(r.hd, pp, c) : mvq_iq4xs_scale(r.hd, pp, c), sx[pp] * V, s1);
      }
      if (is(F_IQ4NL)) acc += s1;
      else acc = __builtin_fmaf(h2f(r.hd.x & 0xFFFFu), s1, acc);
    } else {
      // Q4_K / Q5_K: 6-bit scales / mins of sub-blocks h, h+2, h+4, h+6 of row n, h = c >> 1 (packing: dequant.rs:210-223);
      // chunk 4pp + c lies in sub-block 2pp + h
      const uint32_t s8 = (c >> 1) * 8;
      const uint32_t a = (r.hd.y >> s8) & 0x00FF00FFu, bq = (r.hd.z >> s8) & 0x00FF00FFu, cq = (r.hd.w >> s8) & 0x00FF00FFu;
      const uint32_t sc01 = a & 0x003F003Fu, mn01 = bq & 0x003F003Fu;
      const uint32_t sc23 = (cq & 0x000F000Fu) | ((a >> 2) & 0x00300030u);
      const uint32_t mn23 = ((cq >> 4) & 0x000F000Fu) | ((bq >> 2) & 0x00300030u);
      const float scf[4] = {ub0(sc01), ub2(sc01), ub0(sc23), ub2(sc23)};
      const float mnf[4] = {ub0(mn01), ub2(mn01), ub0(mn23), ub2(mn23)};
      float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int pp = 0; pp < 4; pp++) {
        const uint32_t N0 = (pp & 1) ? r.q[pp >> 1].z : r.q[pp >> 1].x, N1 = (pp & 1) ? r.q[pp >> 1].w : r.q[pp >> 1].y;
        i32x4 bw;
        bw.x = (int)(N0 & 0x0F0F0F0Fu);
        bw.y = (int)((N0 >> 4) & 0x0F0F0F0Fu);
        bw.z = (int)(N1 & 0x0F0F0F0Fu);
        bw.w = (int)((N1 >> 4) & 0x0F0F0F0Fu);
        if (is(F_Q5K)) {   // the fifth bit: dword of the step pair, low nibbles = even step, high nibbles = odd step
          const uint32_t H = ((pp >> 1) ? r.q[2].y : r.q[2].x) >> (4 * (pp & 1));
          bw.x |= (int)((H & 0x01010101u) << 4);
          bw.y |= (int)(((H >> 1) & 0x01010101u) << 4);
          bw.z |= (int)(((H >> 2) & 0x01010101u) << 4);
          bw.w |= (int)(((H >> 3) & 0x01010101u) << 4);
        }
        const i32x4 zero = {0, 0, 0, 0};
        const i32x4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(areg[pp], bw, zero, 0, 0, 0);
        // both halves exact in f32: |D0| <= 64*31*16, |D1..3| <= 128*31*16
        const float hi = (float)((d.x << 8) + d.y), lo = (float)((d.z << 8) + d.w);
        const float V = __builtin_fmaf(hi, 65536.0f, lo);
        s1 = __builtin_fmaf(scf[pp] * sx[pp], V, s1);
        s2 = __builtin_fmaf(mnf[pp], xs[pp], s2);   // the reference's x_acc per sub-block (simd.rs:1002-1008), split per chunk
      }
      const float dd = h2f(r.hd.x & 0xFFFFu), dmin = h2f(r.hd.x >> 16);
      acc += dd * s1 - dmin * s2;
    }
}


// ------------------------------------------------------------------------------------------------
// The same arithmetic in two halves, for the multi-sequence mat-vec (matvec_batch.hip): a weight tile is unpacked ONCE
// (mvq_unpack_tile: the B operands of its four MFMAs + its scales) and then multiplied with the XQ operands of every
// sequence (mvq_mac_tile).  mvq_mac_tile(unpack(r), load(rec)) performs, per format, exactly the floating-point
// operations of mvq_consume_tile(r, rec) in the same order — that is what makes a batched step bit-identical to the
// single-sequence engine (tests/test_gpu_batch.py).
// ------------------------------------------------------------------------------------------------
struct XqOps { i32x4 a[4]; f32x4 xs, sx; };   // the A operands of a block's four MFMAs (zero outside the lane's own chunk), x sums, x scales

// this lane's operands out of one XQ record (LDS or global memory)
__device__ __forceinline__ void xq_load_ops(const uint8_t* rec, uint32_t lane, XqOps& o) {
  const uint32_t n = lane & 15, c = lane >> 4;
  const bool a_valid = (n >> 2) == c;
  const uint32_t a_off = (c >> 1) * 128 + (n & 3) * 32 + (c & 1) * 16;
#pragma unroll
  for (int pp = 0; pp < 4; pp++) {
    i32x4 t = {0, 0, 0, 0};
    if (a_valid) t = *reinterpret_cast<const i32x4*>(rec + pp * 256 + a_off);
    o.a[pp] = t;
  }
  o.xs = *reinterpret_cast<const f32x4*>(rec + kXqXs16 + c * 16);
  o.sx = *reinterpret_cast<const f32x4*>(rec + kXqSx16 + c * 16);
}

struct TileOps {
  i32x4 bw[4];      // B operand of step pp
  float f[4];       // per step: Q4_K/Q5_K sub-block scale, Q6_K / Q3_K int8 scale, Q8_0/Q4_0/Q4_1/Q5_0/Q5_1/IQ4_NL block d, Q2_K chunk scale,
                    // IQ4_XS sub-block ls - 32
  float g[4];       // Q4_K/Q5_K: sub-block min; Q2_K: chunk min; Q4_1/Q5_1: block m
  float dd, dmin;   // Q4_K/Q5_K/Q2_K: d, dmin; Q6_K/Q3_K/IQ4_XS: d
};

template <uint32_t MASK>
__device__ __forceinline__ void mvq_unpack_tile(int fmt, const RawT16& r, uint32_t lane, TileOps& t) {
  const uint32_t n = lane & 15, c = lane >> 4;
  auto is = [&](int f) { return mvq_is<MASK>(fmt, f); };
  if (is(F_Q6K)) {
    const uint32_t s8 = c * 8;
    const uint32_t hdw[4] = {r.hd.x, r.hd.y, r.hd.z, r.hd.w};
#pragma unroll
    for (int pp = 0; pp < 4; pp++) {
      const uint32_t N0 = (pp & 1) ? r.q[pp >> 1].z : r.q[pp >> 1].x, N1 = (pp & 1) ? r.q[pp >> 1].w : r.q[pp >> 1].y;
      const uint32_t H = pp == 0 ? r.q[2].x : pp == 1 ? r.q[2].y : pp == 2 ? r.q[2].z : r.q[2].w;
      t.bw[pp].x = (int)((N0 & 0x0F0F0F0Fu) | ((H & 0x03030303u) << 4));
      t.bw[pp].y = (int)(((N0 >> 4) & 0x0F0F0F0Fu) | (((H >> 2) & 0x03030303u) << 4));
      t.bw[pp].z = (int)((N1 & 0x0F0F0F0Fu) | (((H >> 4) & 0x03030303u) << 4));
      t.bw[pp].w = (int)(((N1 >> 4) & 0x0F0F0F0Fu) | (((H >> 6) & 0x03030303u) << 4));
      t.f[pp] = (float)(int)__builtin_amdgcn_sbfe((int)hdw[pp], s8, 8);
      t.g[pp] = 0.0f;
    }
    const uint32_t dh = (n & 1) ? r.q[3].x >> 16 : r.q[3].x & 0xFFFFu;
    t.dd = h2f(dh);
    t.dmin = 0.0f;
  } else if (is(F_Q80) || is(F_Q40)) {
    const uint32_t hdw[4] = {r.hd.x, r.hd.y, r.hd.z, r.hd.w};
#pragma unroll
    for (int pp = 0; pp < 4; pp++) {
      if (is(F_Q80)) {
        t.bw[pp].x = (int)r.q[pp].x; t.bw[pp].y = (int)r.q[pp].y; t.bw[pp].z = (int)r.q[pp].z; t.bw[pp].w = (int)r.q[pp].w;
      } else {
        const uint32_t N0 = (pp & 1) ? r.q[pp >> 1].z : r.q[pp >> 1].x, N1 = (pp & 1) ? r.q[pp >> 1].w : r.q[pp >> 1].y;
        t.bw[pp].x = (int)(N0 & 0x0F0F0F0Fu);
        t.bw[pp].y = (int)((N0 >> 4) & 0x0F0F0F0Fu);
        t.bw[pp].z = (int)(N1 & 0x0F0F0F0Fu);
        t.bw[pp].w = (int)((N1 >> 4) & 0x0F0F0F0Fu);
      }
      t.f[pp] = h2f((c >> 1) ? hdw[pp] >> 16 : hdw[pp] & 0xFFFFu);
      t.g[pp] = 0.0f;
    }
    t.dd = t.dmin = 0.0f;
  } else if (is(F_Q3K)) {
#pragma unroll
    for (int pp = 0; pp < 4; pp++) {
      t.bw[pp] = mvq_lowbit_operand<true>(r, pp);
      t.f[pp] = (float)(int)__builtin_amdgcn_sbfe((int)r.hd.x, 8 * pp, 8);
      t.g[pp] = 0.0f;
    }
    t.dd = h2f((n & 1) ? r.hd.y >> 16 : r.hd.y & 0xFFFFu);
    t.dmin = 0.0f;
  } else if (is(F_Q2K)) {
#pragma unroll
    for (int pp = 0; pp < 4; pp++) {
      t.bw[pp] = mvq_lowbit_operand<false>(r, pp);
      const uint32_t sm = (r.hd.x >> (8 * pp)) & 0xFFu;
      t.f[pp] = (float)(sm & 15u);
      t.g[pp] = (float)(sm >> 4);
    }
    t.dd = h2f(r.hd.y & 0xFFFFu);
    t.dmin = h2f(r.hd.y >> 16);
  } else if (is(F_Q41) || is(F_Q50) || is(F_Q51)) {
#pragma unroll
    for (int pp = 0; pp < 4; pp++) {
      t.bw[pp] = is(F_Q41) ? mvq_legacy_operand<false>(r, pp) : mvq_legacy_operand<true>(r, pp);
      t.f[pp] = mvq_block_f16(r.hd, pp, c);
      t.g[pp] = is(F_Q50) ? 0.0f : mvq_block_f16(r.q[3], pp, c);
    }
    t.dd = t.dmin = 0.0f;
  } else if (is(F_IQ4NL) || is(F_IQ4XS)) {
#pragma unroll
    for (int pp = 0; pp < 4; pp++) {
      t.bw[pp] = mvq_iq4_operand(r, pp);
      t.f[pp] = is(F_IQ4NL) ? mvq_block_f16(r.hd, pp, c) : mvq_iq4xs_scale(r.hd, pp, c);
      t.g[pp] = 0.0f;
    }
    t.dd = is(F_IQ4NL) ? 0.0f : h2f(r.hd.x & 0xFFFFu);
    t.dmin = 0.0f;
  } else {
    const uint32_t s8 = (c >> 1) * 8;
    const uint32_t a = (r.hd.y >> s8) & 0x00FF00FFu, bq = (r.hd.z >> s8) & 0x00FF00FFu, cq = (r.hd.w >> s8) & 0x00FF00FFu;
    const uint32_t sc01 = a & 0x003F003Fu, mn01 = bq & 0x003F003Fu;
    const uint32_t sc23 = (cq & 0x000F000Fu) | ((a >> 2) & 0x00300030u);
    const uint32_t mn23 = ((cq >> 4) & 0x000F000Fu) | ((bq >> 2) & 0x00300030u);
    t.f[0] = ub0(sc01); t.f[1] = ub2(sc01); t.f[2] = ub0(sc23); t.f[3] = ub2(sc23);
    t.g[0] = ub0(mn01); t.g[1] = ub2(mn01); t.g[2] = ub0(mn23); t.g[3] = ub2(mn23);
#pragma unroll
    for (int pp = 0; pp < 4; pp++) {
      const uint32_t N0 = (pp & 1) ? r.q[pp >> 1].z : r.q[pp >> 1].x, N1 = (pp & 1) ? r.q[pp >> 1].w : r.q[pp >> 1].y;
      t.bw[pp].x = (int)(N0 & 0x0F0F0F0Fu);
      t.bw[pp].y = (int)((N0 >> 4) & 0x0F0F0F0Fu);
      t.bw[pp].z = (int)(N1 & 0x0F0F0F0Fu);
      t.bw[pp].w = (int)((N1 >> 4) & 0x0F0F0F0Fu);
      if (is(F_Q5K)) {
        const uint32_t H = ((pp >> 1) ? r.q[2].y : r.q[2].x) >> (4 * (pp & 1));
        t.bw[pp].x |= (int)((H & 0x01010101u) << 4);
        t.bw[pp].y |= (int)(((H >> 1) & 0x01010101u) << 4);
        t.bw[pp].z |= (int)(((H >> 2) & 0x01010101u) << 4);
        t.bw[pp].w |= (int)(((H >> 3) & 0x01010101u) << 4);
      }
    }
    t.dd = h2f(r.hd.x & 0xFFFFu);
    t.dmin = h2f(r.hd.x >> 16);
  }
}

// mvq_mac_tile in its two phases — the four matrix-core products, then everything the vector ALU does with them — so that a caller
// can put other sequences' products between a sequence's two phases (matvec_batch.hip, mvqb2).  Same operations, same order.
struct MacD { i32x4 d[4]; };

__device__ __forceinline__ void mvq_mac_mfma(const TileOps& t, const i32x4 (&a)[4], MacD& m) {
  const i32x4 zero = {0, 0, 0, 0};
#pragma unroll
  for (int pp = 0; pp < 4; pp++) m.d[pp] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[pp], t.bw[pp], zero, 0, 0, 0);
}

template <uint32_t MASK>
__device__ __forceinline__ void mvq_mac_finish(int fmt, const TileOps& t, const MacD& m, const f32x4 xs, const f32x4 sx, float& acc);

template <uint32_t MASK>
__device__ __forceinline__ void mvq_mac_tile(int fmt, const TileOps& t, const XqOps& o, float& acc) {
  MacD m;
  mvq_mac_mfma(t, o.a, m);
  mvq_mac_finish<MASK>(fmt, t, m, o.xs, o.sx, acc);
}

template <uint32_t MASK>
__device__ __forceinline__ void mvq_mac_finish(int fmt, const TileOps& t, const MacD& m, const f32x4 xs, const f32x4 sx, float& acc) {
  auto is = [&](int f) { return mvq_is<MASK>(fmt, f); };
  struct { f32x4 xs, sx; } o{xs, sx};
  float V[4];
#pragma unroll
  for (int pp = 0; pp < 4; pp++) {
    const i32x4 d = m.d[pp];
    const float hi = (float)((d.x << 8) + d.y), lo = (float)((d.z << 8) + d.w);
    V[pp] = __builtin_fmaf(hi, 65536.0f, lo);
  }
  if (is(F_Q6K)) {
    float s1 = 0.0f;
#pragma unroll
    for (int pp = 0; pp < 4; pp++) s1 = __builtin_fmaf(t.f[pp], __builtin_fmaf(o.sx[pp], V[pp], -32.0f * o.xs[pp]), s1);
    acc = __builtin_fmaf(t.dd, s1, acc);
  } else if (is(F_Q3K)) {
    float s1 = 0.0f;
#pragma unroll
    for (int pp = 0; pp < 4; pp++) s1 = __builtin_fmaf(t.f[pp], __builtin_fmaf(o.sx[pp], V[pp], -4.0f * o.xs[pp]), s1);
    acc = __builtin_fmaf(t.dd, s1, acc);
  } else if (is(F_Q80) || is(F_Q40)) {
    float s1 = 0.0f;
#pragma unroll
    for (int pp = 0; pp < 4; pp++)
      s1 = __builtin_fmaf(t.f[pp], is(F_Q40) ? __builtin_fmaf(o.sx[pp], V[pp], -8.0f * o.xs[pp]) : o.sx[pp] * V[pp], s1);
    acc += s1;
  } else if (is(F_Q50)) {
    float s1 = 0.0f;
#pragma unroll
    for (int pp = 0; pp < 4; pp++) s1 = __builtin_fmaf(t.f[pp], __builtin_fmaf(o.sx[pp], V[pp], -16.0f * o.xs[pp]), s1);
    acc += s1;
  } else if (is(F_Q41) || is(F_Q51)) {
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int pp = 0; pp < 4; pp++) {
      s1 = __builtin_fmaf(t.f[pp] * o.sx[pp], V[pp], s1);
      s2 = __builtin_fmaf(t.g[pp], o.xs[pp], s2);
    }
    acc += s1 + s2;
  } else if (is(F_IQ4NL) || is(F_IQ4XS)) {
    float s1 = 0.0f;
#pragma unroll
    for (int pp = 0; pp < 4; pp++) s1 = __builtin_fmaf(t.f[pp], o.sx[pp] * V[pp], s1);
    if (is(F_IQ4NL)) acc += s1;
    else acc = __builtin_fmaf(t.dd, s1, acc);
  } else {   // Q4_K, Q5_K, Q2_K
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int pp = 0; pp < 4; pp++) {
      s1 = __builtin_fmaf(t.f[pp] * o.sx[pp], V[pp], s1);
      s2 = __builtin_fmaf(t.g[pp], o.xs[pp], s2);
    }
    acc += t.dd * s1 - t.dmin * s2;
  }
}

}  // namespace lgh
