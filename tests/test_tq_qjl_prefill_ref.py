"""The float64 block reference of the TurboQuantProd prompt pass (tests/tq_qjl_prefill_ref.py) against the oracle's f32 restatement of
the reference's decode step (oracle/turboquant.cpp tq_attention_head_qjl), one head, every token of a block, to float32 rounding: the
bound the GPU tests apply, without its f16 term."""
import numpy as np
import pytest

import attention_ref as ar
import tq_prefill_ref as tr
import tq_qjl_prefill_ref as qr


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("bits", [2, 3])
@pytest.mark.parametrize("pos0,m", [(0, 17), (5, 16)])
def test_block_reference_matches_oracle_token_by_token(orc, d, bits, pos0, m):
    rng = np.random.default_rng([d, bits, pos0, m, 11])
    n = pos0 + m
    signs = tr.make_signs(rng, 1, d)
    S = rng.standard_normal((1, d, d)).astype(np.float32)
    rows = [orc.tq_compress_qjl(x, bits, signs[0, 0], S[0]) for x in rng.standard_normal((n, d)).astype(np.float32)]
    kc = np.stack([c for c, _, _ in rows])[None]
    kx = np.stack([np.concatenate([b.view(np.uint32), np.float32([r]).view(np.uint32)]) for _, b, r in rows])[None]
    vc = tr.compress_rows(orc, rng.standard_normal((1, n, d)).astype(np.float32), bits, signs[:, 1])
    q = rng.standard_normal((m, 1, d)).astype(np.float32)
    scale = 1.0 / np.sqrt(d)
    ref, _, _ = qr.block(orc, q, kc, vc, kx, bits, signs, S, scale, pos0)
    assert np.isfinite(ref).all()
    worst = 0.0
    for t in range(m):
        kv_len = pos0 + t + 1
        _, s_mag, vmax = ar.tq_decode(orc, q[t], kc, vc, bits, signs, scale, kv_len, kx, S)
        allow = ar.bound(s_mag, vmax, kv_len) + kv_len * 1e-8 * vmax          # (the oracle skips weights < 1e-8, as the reference does)
        want = orc.tq_attention_head_qjl(q[t, 0], kc[0, :kv_len], kx[0, :kv_len, :d // 32].copy().view(np.uint64), kx[0, :kv_len, d // 32].copy().view(np.float32),
                                         vc[0, :kv_len], kv_len, bits, signs[0, 0], signs[0, 1], S[0], scale)
        worst = max(worst, float(np.abs(want - ref[t, 0]).max()) / allow)
    print(f"tq-qjl block d={d} bits={bits} pos0={pos0} m={m}: oracle err / bound = {worst:.3f}")
    assert worst <= 1.0
