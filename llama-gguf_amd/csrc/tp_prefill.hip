// tp_prefill.hip — the two synchronisation points of a layer for a BLOCK of up to 128 prompt tokens over tensor-parallel ranks: the
// block siblings of tp_reduce_kernel (tensor_parallel.hip) and pf_resid_kernel (prefill.hip).
//
// A rank's wo / down GEMM over its k-shard leaves split-K partial sums [S][128][ncols] of the WHOLE hidden width.  tp_pf_partial_kernel
// collapses them, on the rank's own data only, into one compact block a_r[128][H] f32 — exactly the accumulation pf_resid_kernel runs
// into a0 / a1, zero start and bias included — so that a peer reads H floats per token from this rank and never the S split buffers.
// tp_pf_reduce_kernel<N> then leaves on every rank  hidden = hidden + (((a_0 + a_1) + a_2) ...)  in rank order (tp_reduce_kernel's
// order: all ranks hold the same bits), the XH image of hidden * nw for the next GEMM and the per-chunk sums of squares, with
// pf_resid_kernel's grid, row mapping and summation order.  With N = 1 the two launches give the bits of pf_row_epi_launch.
#include "device_utils.h"
#include "tp_prefill.h"
#include "xh_store.h"

#include <utility>
#include <vector>

namespace lgh {

// (2048-column chunks) x (tokens) workgroups, a thread owns 8 consecutive columns of one token
__global__ void __launch_bounds__(256) tp_pf_partial_kernel(const float* __restrict__ part, uint32_t S, uint32_t ncols, uint32_t col0,
                                                            const float* __restrict__ bias, float* __restrict__ a_out, uint32_t H, uint32_t m) {
  const uint32_t t = blockIdx.y, ch = blockIdx.x * 256 + threadIdx.x, i = ch * 8;
  if (i >= H || t >= m) return;
  f32x4 a0 = (f32x4)(0.0f), a1 = (f32x4)(0.0f);
  for (uint32_t s = 0; s < S; s++) {
    const float* row = part + ((size_t)s * kPfTokens + t) * ncols + col0 + i;
    a0 += *reinterpret_cast<const f32x4*>(row);
    a1 += *reinterpret_cast<const f32x4*>(row + 4);
  }
  if (bias) { a0 += *reinterpret_cast<const f32x4*>(bias + i); a1 += *reinterpret_cast<const f32x4*>(bias + i + 4); }
  *reinterpret_cast<f32x4*>(a_out + (size_t)t * H + i) = a0;
  *reinterpret_cast<f32x4*>(a_out + (size_t)t * H + i + 4) = a1;
}

// Same grid.  Every 16-byte load of a thread — the N partial blocks, the residual, the norm weights — is requested before the first
// is used: the address is clamped (column 0 of the token's row for a thread past H), the loads are unconditional, the stores guarded.
template <int N>
__global__ void __launch_bounds__(256) tp_pf_reduce_kernel(const float* __restrict__ a0p, float* __restrict__ hidden, const float* __restrict__ nw,
                                                           uint8_t* __restrict__ xh, float* __restrict__ ssq, uint32_t H, uint32_t m,
                                                           TpPfPeers peers) {
  __shared__ float s_ss[4];
  const uint32_t t = blockIdx.y, ch = blockIdx.x * 256 + threadIdx.x, i = ch * 8;
  const bool ok = i < H && t < m;
  const size_t at = (size_t)(t < m ? t : 0) * H + (i < H ? i : 0);
  f32x4 a[N][2];
  a[0][0] = *reinterpret_cast<const f32x4*>(a0p + at);
  a[0][1] = *reinterpret_cast<const f32x4*>(a0p + at + 4);
#pragma unroll
  for (int r = 1; r < N; r++) {
    a[r][0] = *reinterpret_cast<const f32x4*>(peers.p[r - 1] + at);
    a[r][1] = *reinterpret_cast<const f32x4*>(peers.p[r - 1] + at + 4);
  }
  f32x4 v0 = *reinterpret_cast<const f32x4*>(hidden + at), v1 = *reinterpret_cast<const f32x4*>(hidden + at + 4);
  f32x4 w0 = (f32x4)(1.0f), w1 = (f32x4)(1.0f);
  if (nw) {   // (a uniform branch, as in tp_reduce_kernel: the loads above are out before these two)
    w0 = *reinterpret_cast<const f32x4*>(nw + (i < H ? i : 0));
    w1 = *reinterpret_cast<const f32x4*>(nw + (i < H ? i : 0) + 4);
  }
  f32x4 s0 = a[0][0], s1 = a[0][1];
#pragma unroll
  for (int r = 1; r < N; r++) { s0 += a[r][0]; s1 += a[r][1]; }   // rank order, one rounding per add
  v0 += s0;   // the residual last
  v1 += s1;
  float ss = 0.0f;
  if (ok) {
    *reinterpret_cast<f32x4*>(hidden + at) = v0;
    *reinterpret_cast<f32x4*>(hidden + at + 4) = v1;
    const f32x4 q = v0 * v0 + v1 * v1;
    ss = (q.x + q.y) + (q.z + q.w);
    if (nw) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 4; j++) { v[j] = v0[j] * w0[j]; v[4 + j] = v1[j] * w1[j]; }
      xh_store_chunk(xh, t, ch, v);
    }
  }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) s_ss[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0 && ssq && t < m) ssq[t * kPfSsqChunks + blockIdx.x] = (s_ss[0] + s_ss[1]) + (s_ss[2] + s_ss[3]);
}

static uint32_t tp_pf_chunks(uint32_t H) { return (H + 2047) / 2048; }

hipError_t tp_pf_partial_launch(const float* part, uint32_t S, uint32_t ncols, uint32_t col0, const float* bias, float* a_out, uint32_t H,
                                uint32_t m_tokens, hipStream_t st) {
  if (!part || !a_out || S == 0 || H == 0 || H % 8 || ncols % 4 || col0 % 4 || (uint64_t)col0 + H > ncols || m_tokens == 0 ||
      m_tokens > (uint32_t)kPfTokens)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(tp_pf_partial_kernel, dim3(tp_pf_chunks(H), m_tokens), dim3(256), 0, st, part, S, ncols, col0, bias, a_out, H, m_tokens);
  return hipGetLastError();
}

hipError_t tp_pf_reduce_launch(const float* const* blocks, uint32_t n, float* hidden, uint32_t H, const float* nw, uint8_t* xh, float* ssq,
                               uint32_t m_tokens, hipStream_t st) {
  if (!blocks || !hidden || n < 1 || n > (uint32_t)kTpPfMaxRanks || H == 0 || H % 8 || m_tokens == 0 || m_tokens > (uint32_t)kPfTokens)
    return hipErrorInvalidValue;
  // (an XH needs the norm weights and a place for the sums of squares its consumer divides by; those are kept for kPfSsqChunks chunks)
  if ((nw && (!xh || !ssq)) || (ssq && tp_pf_chunks(H) > (uint32_t)kPfSsqChunks)) return hipErrorInvalidValue;
  TpPfPeers peers{};
  for (uint32_t r = 1; r < n; r++) peers.p[r - 1] = blocks[r];
  const dim3 g(tp_pf_chunks(H), m_tokens), b(256);
#define TP_PF_GO(NR) hipLaunchKernelGGL(tp_pf_reduce_kernel<NR>, g, b, 0, st, blocks[0], hidden, nw, xh, ssq, H, m_tokens, peers)
  switch (n) {
    case 1: TP_PF_GO(1); break;
    case 2: TP_PF_GO(2); break;
    case 3: TP_PF_GO(3); break;
    case 4: TP_PF_GO(4); break;
    case 5: TP_PF_GO(5); break;
    case 6: TP_PF_GO(6); break;
    case 7: TP_PF_GO(7); break;
    default: TP_PF_GO(8); break;
  }
#undef TP_PF_GO
  return hipGetLastError();
}

}  // namespace lgh

using namespace lgh;

extern "C" {

// The two launches on their own, or (path 1) pf_row_epi_launch on rank 0's split partials: the yardstick a one-rank block has to equal
// bit for bit.  hidden_io, xh_image and ssq_io are in / out: the device buffers start from the host's bytes, so that a caller sees which
// bytes the kernels wrote; every device buffer also sits between two guard bands, and a changed guard byte is OperationFailed.
int lgh_op_tp_pf_reduce(int device, int path, const float* partials, uint32_t n, uint32_t S, size_t ncols, size_t col0, const float* bias,
                        const float* resid, const float* norm_w, size_t H, size_t m, float* hidden_io, uint8_t* xh_image, float* ssq_io) {
  if (!partials || !resid || !hidden_io || !xh_image || !ssq_io) return LGH_INVALID_ARGUMENT;
  if (n < 1 || n > (uint32_t)kTpPfMaxRanks || m < 1 || m > (size_t)kPfTokens || H == 0 || H % 8 || H > 2048u * kPfSsqChunks) return LGH_INVALID_ARGUMENT;
  if (ncols % 4 || col0 % 4 || col0 + H > ncols || ncols > (1u << 24) || S < 1 || S > 256) return LGH_INVALID_ARGUMENT;
  if ((path != 0 && path != 1) || (path == 1 && n != 1)) return LGH_INVALID_ARGUMENT;
  const int nd = lgh_device_count();
  if (nd <= 0 || device < 0 || device >= nd) return LGH_NOT_AVAILABLE;
  if (hipSetDevice(device) != hipSuccess) return LGH_NOT_AVAILABLE;
  constexpr size_t kGuard = 256;
  constexpr uint8_t kPattern = 0xA5;
  std::vector<void*> allocs;
  std::vector<std::pair<uint8_t*, size_t>> guarded;   // (base, payload bytes)
  hipStream_t st = nullptr;
  auto cleanup = [&](int rc) {
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (void* p : allocs) (void)hipFree(p);
    return rc;
  };
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return LGH_INITIALIZATION_FAILED;
  auto up = [&](const void* host, size_t bytes) -> uint8_t* {   // payload rounded up to 256 bytes so that the next guard stays aligned
    const size_t padded = (bytes + 255) / 256 * 256;
    uint8_t* base = nullptr;
    if (hipMalloc((void**)&base, padded + 2 * kGuard) != hipSuccess) return nullptr;
    allocs.push_back(base);
    if (hipMemsetAsync(base, kPattern, padded + 2 * kGuard, st) != hipSuccess) return nullptr;
    if (host && hipMemcpyAsync(base + kGuard, host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return nullptr;
    guarded.push_back({base, bytes});
    return base + kGuard;
  };
  const size_t rank_floats = (size_t)S * kPfTokens * ncols, hid_bytes = (size_t)kPfTokens * H * 4;
  const size_t xh_len = (H + 255) / 256 * (size_t)kPfSlabBytes, ssq_bytes = (size_t)kPfTokens * kPfSsqChunks * 4;
  const float* d_part[kTpPfMaxRanks] = {};
  const float* d_blk[kTpPfMaxRanks] = {};
  for (uint32_t r = 0; r < n; r++) {
    d_part[r] = (const float*)up(partials + r * rank_floats, rank_floats * 4);
    if (path == 0) d_blk[r] = (const float*)up(nullptr, hid_bytes);   // (the compact block starts as the guard pattern: rows t >= m are never read)
    if (!d_part[r] || (path == 0 && !d_blk[r])) return cleanup(LGH_ALLOCATION_FAILED);
  }
  const float* d_bias = bias ? (const float*)up(bias, H * 4) : nullptr;
  const float* d_nw = norm_w ? (const float*)up(norm_w, H * 4) : nullptr;
  float* d_hid = (float*)up(hidden_io, hid_bytes);
  uint8_t* d_xh = up(xh_image, xh_len);
  float* d_ssq = (float*)up(ssq_io, ssq_bytes);
  if ((bias && !d_bias) || (norm_w && !d_nw) || !d_hid || !d_xh || !d_ssq) return cleanup(LGH_ALLOCATION_FAILED);
  if (hipMemcpyAsync(d_hid, resid, m * H * 4, hipMemcpyHostToDevice, st) != hipSuccess) return cleanup(LGH_OPERATION_FAILED);
  bool ok = true;
  if (path == 1) {
    ok = pf_row_epi_launch(d_part[0], S, (uint32_t)ncols, (uint32_t)col0, d_bias, d_hid, (uint32_t)H, d_nw, d_nw ? d_xh : nullptr, d_ssq, (uint32_t)m, st) ==
         hipSuccess;
  } else {
    for (uint32_t r = 0; r < n && ok; r++)   // (lgh_tp_upload_tensor gives attn_output.bias to rank 0 alone)
      ok = tp_pf_partial_launch(d_part[r], S, (uint32_t)ncols, (uint32_t)col0, r == 0 ? d_bias : nullptr, (float*)d_blk[r], (uint32_t)H, (uint32_t)m, st) ==
           hipSuccess;
    ok = ok && tp_pf_reduce_launch(d_blk, n, d_hid, (uint32_t)H, d_nw, d_xh, d_ssq, (uint32_t)m, st) == hipSuccess;
  }
  if (!ok) return cleanup(LGH_OPERATION_FAILED);
  ok = hipMemcpyAsync(hidden_io, d_hid, hid_bytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
       hipMemcpyAsync(xh_image, d_xh, xh_len, hipMemcpyDeviceToHost, st) == hipSuccess &&
       hipMemcpyAsync(ssq_io, d_ssq, ssq_bytes, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
  std::vector<uint8_t> g;
  for (size_t i = 0; i < guarded.size() && ok; i++) {   // the bands in front of and behind every buffer (the payload's rounding included)
    const size_t bytes = guarded[i].second, tail = (bytes + 255) / 256 * 256 - bytes + kGuard;
    g.resize(kGuard + tail);
    ok = hipMemcpy(g.data(), guarded[i].first, kGuard, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(g.data() + kGuard, guarded[i].first + kGuard + bytes, tail, hipMemcpyDeviceToHost) == hipSuccess;
    for (size_t j = 0; j < g.size() && ok; j++)
      if (g[j] != kPattern) ok = false;
  }
  return cleanup(ok ? LGH_OK : LGH_OPERATION_FAILED);
}

}  // extern "C"
