"""A float64 restatement of a block of prompt tokens over a TurboQuantProd cache (tq2-qjl / tq3-qjl): token t of the block is the
reference's decode step at kv_len = pos0 + t + 1 (kv_turboquant.rs:127-201 with the QJL score correction, quant.rs:133-168), which is
`attention_ref.tq_decode` with the K rows' QJL words and the projection matrices.  Shared by tests/test_tq_qjl_prefill_ref.py (against
the oracle, on the CPU) and tests/test_gpu_tq_qjl_prefill.py (the arbiter of the batched path's kernels)."""
from __future__ import annotations

import numpy as np

import attention_ref as ar


def block(orc, q, k_codes, v_codes, k_qjl, bits: int, signs, S, scale: float, pos0: int):
    """q [m, n_heads, d]; codes [n_kv, rows, row bytes]; k_qjl [n_kv, rows, d / 32 + 1] uint32; signs [n_kv, 2, d]; S [n_kv, d, d].
    -> (out [m, n_heads, d] float64, S_mag, vmax): the bound's magnitudes are the maxima over the block's tokens."""
    q = np.asarray(q, np.float64)
    out = np.zeros_like(q)
    s_mag = vmax = 0.0
    for t in range(q.shape[0]):
        out[t], s, v = ar.tq_decode(orc, q[t], k_codes, v_codes, bits, signs, scale, pos0 + t + 1, k_qjl, S)
        s_mag, vmax = max(s_mag, s), max(vmax, v)
    return out, s_mag, vmax
