"""The float64 attention restatement (tests/attention_ref.py) — the arbiter of the kernel-level attention tests — against the
oracle's f32 restatements of the reference (oracle/ops.cpp, oracle/turboquant.cpp), at the shapes the GPU tests use, within
the bound the GPU tests apply.  The oracle skips softmax weights below 1e-8 as the reference's CPU path does; the skipped
mass times max|V| is added to the bound for these comparisons."""
import numpy as np
import pytest

import attention_ref as ar

SHAPES = [(64, 1), (64, 8), (128, 2), (128, 4), (96, 7), (80, 3)]


def _skipped(w, vmax):
    return float(w[w < 2e-8].sum()) * vmax if w.size else 0.0


def _cache(rng, n_kv, rows, d, kv_len):
    k = rng.standard_normal((n_kv, rows, d)).astype(np.float32)
    v = rng.standard_normal((n_kv, rows, d)).astype(np.float32)
    k[:, kv_len:] = np.nan   # never visible: the restatement must not read them
    v[:, kv_len:] = np.nan
    return k, v


@pytest.mark.parametrize("d,g", SHAPES)
@pytest.mark.parametrize("kv_len", [1, 2, 64, 65, 1000])
def test_decode_matches_oracle_attention_cached(orc, d, g, kv_len):
    rng = np.random.default_rng(d * 1000 + g * 10 + kv_len)
    n_kv, rows = 2, 1024
    q = rng.standard_normal((n_kv * g, d)).astype(np.float32)
    k, v = _cache(rng, n_kv, rows, d, kv_len)
    scale = 1.0 / np.sqrt(d)
    ref = ar.decode(q, k, v, scale, kv_len)
    assert np.isfinite(ref).all()
    want = orc.attention_cached(q, k, v, scale, kv_len)
    S, vmax = ar.magnitude(q, k, scale, kv_len), float(np.abs(v[:, :kv_len]).max())
    allow = ar.bound(S, vmax, kv_len) + _skipped(ar.weights(q, k, scale, kv_len), vmax)
    err = float(np.abs(want - ref).max())
    print(f"decode d={d} g={g} kv={kv_len}: oracle err / bound = {err / allow:.3f}")
    assert err <= allow


def test_decode_one_row_is_that_row(orc):
    rng = np.random.default_rng(1)
    k, v = _cache(rng, 2, 8, 64, 1)
    q = rng.standard_normal((4, 64))
    np.testing.assert_array_equal(ar.decode(q, k, v, 0.125, 1), np.repeat(v[:, 0].astype(np.float64), 2, axis=0))


@pytest.mark.parametrize("d,g", SHAPES)
@pytest.mark.parametrize("pos0,m", [(0, 1), (0, 17), (5, 16), (16, 15), (40, 100)])
def test_prefill_matches_oracle_attention(orc, d, g, pos0, m):
    rng = np.random.default_rng(d + g + pos0 + m)
    n_kv = 2
    n = pos0 + m
    q = rng.standard_normal((m, n_kv * g, d)).astype(np.float32)
    k = rng.standard_normal((n_kv, n, d)).astype(np.float32)
    v = rng.standard_normal((n_kv, n, d)).astype(np.float32)
    scale = 1.0 / np.sqrt(d)
    ref = ar.prefill(q, k, v, scale, pos0, m)
    want = orc.attention(q.transpose(1, 0, 2), k, v, scale).transpose(1, 0, 2)   # Backend::attention: [heads, seq, d]
    S, vmax = ar.magnitude(q, k, scale, n), float(np.abs(v).max())
    worst = 0.0
    for t in range(m):
        w = ar.weights(q[t], k, scale, pos0 + t + 1)
        allow = ar.bound(S, vmax, pos0 + t + 1) + _skipped(w, vmax)
        worst = max(worst, float(np.abs(want[t] - ref[t]).max()) / allow)
    print(f"prefill d={d} g={g} pos0={pos0} m={m}: oracle err / bound = {worst:.3f}")
    assert worst <= 1.0


def test_prefill_is_causal():
    """Token t of a block equals a decode step at position pos0 + t over the same cache."""
    rng = np.random.default_rng(7)
    q = rng.standard_normal((5, 4, 64))
    k, v = _cache(rng, 2, 12, 64, 12)
    out = ar.prefill(q, k, v, 0.125, 7, 5)
    for t in range(5):
        np.testing.assert_allclose(out[t], ar.decode(q[t], k, v, 0.125, 7 + t + 1), rtol=1e-12, atol=1e-14)


# ---- readers
def test_int8_reader_matches_oracle(orc):
    rng = np.random.default_rng(3)
    x = rng.standard_normal(128).astype(np.float32)
    qb, sc = orc.kv_quantize_int8(x)
    np.testing.assert_array_equal(ar.int8_values(qb[None], np.float32([sc]))[0].astype(np.float32), orc.kv_dequantize_int8(qb, sc))


@pytest.mark.parametrize("kv_type", [2, 3])
def test_fp8_table(orc, kv_type):
    t = ar.fp8_table(orc, kv_type)
    assert np.isnan(t[0x7F]) and np.isnan(t[0xFF])   # the NaN sentinel the GPU tests put past the visible rows
    assert t[0] == 0.0 and t[0x80] == 0.0
    fmt = {2: orc.FP8_E4M3, 3: orc.FP8_E5M2}[kv_type]
    for x in (0.5, -1.25, 3.0, 0.0078125):
        assert t[orc.kv_quantize_fp8(fmt, x)] == x


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("bits", [2, 3])
def test_tq_readers_match_oracle(orc, d, bits):
    rng = np.random.default_rng(d + bits)
    signs = np.where(rng.random(d) < 0.5, -1.0, 1.0).astype(np.float32)
    x = rng.standard_normal(d).astype(np.float32)
    rot = ar.tq_rotate(x, signs)
    np.testing.assert_allclose(rot, orc.tq_rotate(x, signs), rtol=0, atol=16 * ar.U * np.abs(x).sum() / np.sqrt(d))
    np.testing.assert_allclose(ar.tq_rotate_inverse(rot, signs), x, rtol=0, atol=1e-12 * np.abs(x).max())
    codes = orc.tq_compress(x, bits, signs)
    np.testing.assert_array_equal(ar.tq_indices(codes, bits, d), [orc.tq_quantize(d, bits, r) for r in orc.tq_rotate(x, signs)])
    deq = orc.tq_dequantize_vector(d, bits, codes, d)
    np.testing.assert_array_equal(ar.tq_centroids(orc, codes, bits, d), deq)
    want = orc.tq_rotate_inverse(deq, d, signs)
    np.testing.assert_allclose(ar.tq_values(orc, codes, bits, d, signs), want, rtol=0, atol=16 * ar.U * np.abs(deq).sum())


def _tq_rows(orc, rng, n, d, bits, signs, S=None):
    xs = rng.standard_normal((n, d)).astype(np.float32)
    if S is None:
        return np.stack([orc.tq_compress(x, bits, signs) for x in xs]), None, None
    out = [orc.tq_compress_qjl(x, bits, signs, S) for x in xs]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.float32([o[2] for o in out])


@pytest.mark.parametrize("d,g", [(64, 1), (64, 8), (128, 2), (128, 4)])
@pytest.mark.parametrize("bits", [2, 3])
@pytest.mark.parametrize("qjl", [False, True])
@pytest.mark.parametrize("kv_len", [1, 65, 300])
def test_tq_decode_matches_oracle_head(orc, d, g, bits, qjl, kv_len):
    rng = np.random.default_rng(d * 7 + g + bits * 3 + kv_len + qjl)
    n_kv = 2
    signs = np.where(rng.random((n_kv, 2, d)) < 0.5, -1.0, 1.0).astype(np.float32)
    S = rng.standard_normal((n_kv, d, d)).astype(np.float32) if qjl else None
    q = rng.standard_normal((n_kv * g, d)).astype(np.float32)
    kc, vc, kx = [], [], []
    for h in range(n_kv):
        c, qb, nrm = _tq_rows(orc, rng, kv_len, d, bits, signs[h, 0], S[h] if qjl else None)
        kc.append(c)
        vc.append(_tq_rows(orc, rng, kv_len, d, bits, signs[h, 1])[0])
        if qjl:
            kx.append(np.concatenate([qb.view(np.uint32), nrm.view(np.uint32)[:, None]], axis=1))
    kc, vc = np.stack(kc), np.stack(vc)
    kx = np.stack(kx) if qjl else None
    scale = 1.0 / np.sqrt(d)
    ref, s_mag, vmax = ar.tq_decode(orc, q, kc, vc, bits, signs, scale, kv_len, kx, S)
    worst = 0.0
    for h in range(n_kv * g):
        kvh = h // g
        if qjl:
            want = orc.tq_attention_head_qjl(q[h], kc[kvh], kx[kvh, :, : d // 32].copy().view(np.uint64), ar.qjl_norms(kx[kvh], d),
                                             vc[kvh], kv_len, bits, signs[kvh, 0], signs[kvh, 1], S[kvh], scale)
        else:
            want = orc.tq_attention_head(q[h], kc[kvh], vc[kvh], kv_len, bits, signs[kvh, 0], signs[kvh, 1], scale)
        allow = ar.bound(s_mag, vmax, kv_len) + kv_len * 1e-8 * vmax
        worst = max(worst, float(np.abs(want - ref[h]).max()) / allow)
    print(f"tq d={d} g={g} bits={bits} qjl={qjl} kv={kv_len}: oracle err / bound = {worst:.3f}")
    assert worst <= 1.0


def test_bound_sees_a_dropped_row(orc):
    """The bound is tight enough that losing the last visible row of a 1000-row context shows (the masks the GPU tests guard)."""
    rng = np.random.default_rng(11)
    k, v = _cache(rng, 2, 1024, 128, 1000)
    q = rng.standard_normal((4, 128))
    scale = 1.0 / np.sqrt(128)
    ref = ar.decode(q, k, v, scale, 1000)
    short = ar.decode(q, k, v, scale, 999)
    S, vmax = ar.magnitude(q, k, scale, 1000), float(np.abs(v[:, :1000]).max())
    assert ar.worst_ratio(short, ref, S, vmax, 1000) > 2.0
