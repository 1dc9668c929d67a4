// tp_prefill.h — the two row-wise launches of a tensor-parallel prompt block (tp_prefill.hip; internal).
#pragma once

#include "prefill.h"

namespace lgh {

constexpr int kTpPfMaxRanks = 8;
// the compact partial blocks [128][H] f32 of ranks 1 .. N - 1 (rank 0's is an argument of its own), by value as TpPeers
struct TpPfPeers { const float* p[kTpPfMaxRanks - 1]; };

// a_out[t][i] = ((0 + part[0][t][col0 + i]) + part[1][t][col0 + i]) + ... (+ bias[i]) for the m_tokens tokens of one rank's split-K
// partial sums [S][128][ncols]: pf_resid_kernel's accumulation, stored instead of added to the residual.  H % 8 == 0, S >= 1,
// ncols % 4 == 0, col0 % 4 == 0, col0 + H <= ncols.
hipError_t tp_pf_partial_launch(const float* part, uint32_t S, uint32_t ncols, uint32_t col0, const float* bias, float* a_out, uint32_t H,
                                uint32_t m_tokens, hipStream_t st);
// hidden[t][i] += (((a_0 + a_1) + a_2) ...) over blocks[0 .. n), rank order; with nw also XH[t][i] = f16(f32(hidden * nw)) (xh and ssq
// required then); with ssq the per-chunk sums of hidden^2 in pf_resid_kernel's order.  n in 1 .. 8, H % 8 == 0.
hipError_t tp_pf_reduce_launch(const float* const* blocks, uint32_t n, float* hidden, uint32_t H, const float* nw, uint8_t* xh, float* ssq,
                               uint32_t m_tokens, hipStream_t st);

}  // namespace lgh
