"""The float64 reference of the batched prompt pass over a byte KV cache (tests/kv8_prefill_ref.py), checked on the CPU against what
it is built from: causal visibility, rows past the block, and the oracle's own round trip of a row."""
import numpy as np
import pytest

import attention_ref as ar
import kv8_prefill_ref as kr


def _case(orc, kv_type, d=64, n_kv=2, g=2, rows=40, seed=0):
    rng = np.random.default_rng([kv_type, d, seed])
    kb, ks = kr.encode_rows(orc, kv_type, rng.standard_normal((n_kv, rows, d)))
    vb, vs = kr.encode_rows(orc, kv_type, 2.0 * rng.standard_normal((n_kv, rows, d)))
    if kv_type != kr.KV_INT8:
        ks = vs = None
    return rng, kb, vb, ks, vs


@pytest.mark.parametrize("kv_type", kr.FORMATS)
def test_token_t_is_a_decode_step_over_its_visible_rows(orc, kv_type):
    """Causal visibility: token t of the block equals attention_ref.decode of its query over rows 0..pos0 + t."""
    rng, kb, vb, ks, vs = _case(orc, kv_type)
    pos0, m, scale = 7, 19, 0.125
    q = rng.standard_normal((m, 4, 64)).astype(np.float32)
    out = kr.block(orc, kv_type, q, kb, vb, ks, vs, scale, pos0, m)
    K, V = kr.values(orc, kv_type, kb, ks, pos0 + m), kr.values(orc, kv_type, vb, vs, pos0 + m)
    for t in (0, 1, m - 1):
        np.testing.assert_allclose(out[t], ar.decode(q[t], K, V, scale, pos0 + t + 1), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("kv_type", kr.FORMATS)
def test_rows_past_the_block_change_nothing(orc, kv_type):
    rng, kb, vb, ks, vs = _case(orc, kv_type)
    pos0, m = 3, 12
    q = rng.standard_normal((m, 4, 64)).astype(np.float32)
    want = kr.block(orc, kv_type, q, kb, vb, ks, vs, 0.125, pos0, m)
    kb2, vb2 = kb.copy(), vb.copy()
    kb2[:, pos0 + m:] = 0x7F
    vb2[:, pos0 + m:] = 0x7F
    ks2 = vs2 = None
    if kv_type == kr.KV_INT8:
        ks2, vs2 = ks.copy(), vs.copy()
        ks2[:, pos0 + m:] = np.nan
        vs2[:, pos0 + m:] = np.nan
    got = kr.block(orc, kv_type, q, kb2, vb2, ks2, vs2, 0.125, pos0, m)
    assert np.array_equal(got, want) and np.isfinite(got).all()
    # ... and a later row of the block changes the later tokens only
    vb3 = vb.copy()
    vb3[:, pos0 + 5] ^= 0x11
    other = kr.block(orc, kv_type, q, kb, vb3, ks, vs, 0.125, pos0, m)
    assert np.array_equal(other[:5], want[:5]) and not np.array_equal(other[5:], want[5:])


@pytest.mark.parametrize("kv_type", kr.FORMATS)
def test_encode_then_values_is_the_oracles_round_trip(orc, kv_type):
    rng = np.random.default_rng(kv_type)
    rows = rng.standard_normal((1, 6, 64)).astype(np.float32)
    rows[0, 1] = 0.0                               # an all-zero row: int8 scale 1
    rows[0, 2] = -np.abs(rows[0, 2]) - 0.5         # the largest element is negative
    b, sc = kr.encode_rows(orc, kv_type, rows)
    got = kr.values(orc, kv_type, b, sc if kv_type == kr.KV_INT8 else None, 6)
    for r in range(6):
        if kv_type == kr.KV_INT8:
            q8, s = orc.kv_quantize_int8(rows[0, r])
            want = orc.kv_dequantize_int8(q8, s).astype(np.float64)
        else:
            fmt = {kr.KV_FP8_E4M3: orc.FP8_E4M3, kr.KV_FP8_E5M2: orc.FP8_E5M2}[kv_type]
            want = np.array([orc.kv_dequantize_fp8(fmt, orc.kv_quantize_fp8(fmt, float(x))) for x in rows[0, r]], np.float64)
        # int8: scale * q in float64 against the oracle's f32 product — one f32 rounding apart
        np.testing.assert_allclose(got[0, r], want, rtol=2.0 ** -23 if kv_type == kr.KV_INT8 else 0, atol=0)
    assert sc[0, 1] == 1.0 or kv_type != kr.KV_INT8
