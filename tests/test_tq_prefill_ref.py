"""The float64 block reference of the TurboQuant prompt pass (tests/tq_prefill_ref.py) against the oracle's f32 restatement of the
reference, TurboQuantKVCache::attention_layer (oracle/turboquant.cpp tq_attention_head), row by row for every token of a block, within
the bound the GPU tests apply — and three planted mistakes, each of which must exceed that bound."""
import numpy as np
import pytest

import attention_ref as ar
import tq_prefill_ref as tr

N_KV, G = 2, 2


def _case(orc, d, bits, pos0, m):
    rng = np.random.default_rng([d, bits, pos0, m])
    n = pos0 + m
    signs = tr.make_signs(rng, N_KV, d)
    kc = tr.compress_rows(orc, rng.standard_normal((N_KV, n, d)).astype(np.float32), bits, signs[:, 0])
    vc = tr.compress_rows(orc, rng.standard_normal((N_KV, n, d)).astype(np.float32), bits, signs[:, 1])
    q = rng.standard_normal((m, N_KV * G, d)).astype(np.float32)
    return q, kc, vc, signs, 1.0 / np.sqrt(d)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("bits", [2, 3])
@pytest.mark.parametrize("pos0,m", [(0, 17), (5, 16)])
def test_block_reference_matches_oracle_row_by_row(orc, d, bits, pos0, m):
    q, kc, vc, signs, scale = _case(orc, d, bits, pos0, m)
    ref = tr.block(orc, q, kc, vc, bits, signs, scale, pos0, m)
    assert np.isfinite(ref).all()
    K, V = tr.values(orc, kc, vc, bits, d, signs, pos0 + m)
    np.testing.assert_array_equal(tr.attend(q, K, V, scale, tr.visibility(pos0, m)), ref)   # `attend` is prefill under the plain mask
    worst = 0.0
    for t in range(m):
        kv_len = pos0 + t + 1
        s_mag, vmax = tr.magnitudes(orc, q[t:t + 1], kc, vc, bits, signs, scale, kv_len)
        allow = ar.bound(s_mag, vmax, kv_len) + kv_len * 1e-8 * vmax          # (the oracle skips weights < 1e-8, as the reference does)
        for h in range(N_KV * G):
            kvh = h // G
            want = orc.tq_attention_head(q[t, h], kc[kvh], vc[kvh], kv_len, bits, signs[kvh, 0], signs[kvh, 1], scale)
            worst = max(worst, float(np.abs(want - ref[t, h]).max()) / allow)
    print(f"tq block d={d} bits={bits} pos0={pos0} m={m}: oracle err / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("bits", [2, 3])
@pytest.mark.parametrize("pos0,m", [(0, 17), (5, 16)])
def test_bound_sees_planted_mistakes(orc, d, bits, pos0, m):
    """A dropped last row, V's rotation inverted with K's signs and a mask that is off by one each exceed the bound of the GPU test
    (f16 term included)."""
    q, kc, vc, signs, scale = _case(orc, d, bits, pos0, m)
    n = pos0 + m
    ref = tr.block(orc, q, kc, vc, bits, signs, scale, pos0, m)
    s_mag, vmax = tr.magnitudes(orc, q, kc, vc, bits, signs, scale, n)
    K, V = tr.values(orc, kc, vc, bits, d, signs, n)
    assert ar.worst_ratio(ref.astype(np.float32), ref, s_mag, vmax, n, f16=True) <= 1.0
    dropped = tr.attend(q, K, V, scale, tr.visibility(pos0, m, drop_last=True))
    assert ar.worst_ratio(dropped, ref, s_mag, vmax, n, f16=True) > 1.0
    off_by_one = tr.attend(q, K, V, scale, tr.visibility(pos0, m, shift=1))
    assert ar.worst_ratio(off_by_one, ref, s_mag, vmax, n, f16=True) > 1.0
    _, V_k = tr.values(orc, kc, vc, bits, d, signs, n, v_sign_index=0)
    assert ar.worst_ratio(tr.attend(q, K, V_k, scale, tr.visibility(pos0, m)), ref, s_mag, vmax, n, f16=True) > 1.0
