"""CPU checks of tests/matvec_ref.py, the float64 judge of tests/test_gpu_matvec.py: its decoders against the oracle's
dequantization for every weight generator, the oracle's f32 mat-vec inside the derived bound at the GPU test shapes, and the
bound's power: each planted mistake must exceed it at least twice on some row at the largest k the GPU tests use."""
import numpy as np
import pytest

import matvec_ref as mr

K_GPU_MAX = 28672


def _raw(pkg, orc, tname, kind, k, n, seed):
    return mr.weights(tname, kind, k, n, seed, orc=orc, synth_fill=pkg.synth.fill_tensor)


@pytest.mark.parametrize("kind", mr.WEIGHT_KINDS)
@pytest.mark.parametrize("tname", mr.FUSED)
def test_decoders_match_oracle(pkg, orc, tname, kind):
    k, n = 512, 24
    raw = _raw(pkg, orc, tname, kind, k, n, 3)
    a, o = mr.decode(tname, raw, k, n)
    w = a - o
    got = orc.dequantize(mr.TYPE[tname], raw, k * n).reshape(n, k).astype(np.float64)
    assert np.all(np.isfinite(w))
    exact = w.astype(np.float32).astype(np.float64) == w           # the f32 value is the exact one: bit for bit
    assert np.array_equal(got[exact], w[exact])
    assert np.all(np.abs(got - w) <= mr.U * np.abs(w))             # elsewhere: one f32 rounding
    assert np.abs(w).max() <= 2.0 or kind in ("synth", "quantized")   # |w| about 1 or less


def test_generators_cover_the_header_ranges(pkg, orc):
    k, n = 1024, 16
    a, o = mr.decode("Q4_0", _raw(pkg, orc, "Q4_0", "full", k, n, 1), k, n)
    assert (o < 0).any() and (o > 0).any()                          # d of both signs
    raw = _raw(pkg, orc, "Q6_K", "full", k, n, 1).reshape(n, k // 256, 210)
    sc = raw[..., 192:208].view(np.int8)
    assert sc.min() == -128 and sc.max() == 127
    d = raw[..., 208:210].copy().view(np.float16)
    assert (d < 0).any() and (d > 0).any() and (np.abs(d) < np.float16(6.1e-5)).any()   # signs and subnormals
    raw = _raw(pkg, orc, "Q4_K", "full", k, n, 1).reshape(n, k // 256, 144)
    s, m = mr._k4_scales(raw[..., 4:16])
    assert s.min() == 0 and s.max() == 63 and m.min() == 0 and m.max() == 63
    raw = _raw(pkg, orc, "Q8_0", "full", k, n, 1).reshape(n, k // 32, 34)
    assert raw[..., 2:].view(np.int8).min() == -128


@pytest.mark.parametrize("act", mr.ACT_KINDS)
def test_activation_kinds(act):
    x = mr.activation(act, 4096, 7)
    assert x.dtype == np.float32 and np.all(np.isfinite(x))
    if act == "pow2":
        m = np.abs(x.reshape(-1, 16)).max(axis=1)
        assert np.all(np.log2(m[0::2]) == np.round(np.log2(m[0::2])))
        assert np.all(np.nextafter(m[1::2], np.float32(np.inf)) == 2.0 ** np.round(np.log2(m[1::2])))
    if act == "zeros":
        assert np.signbit(x[16:32]).all() and (x[16:32] == 0).all()


@pytest.mark.parametrize("k", [256, 5632, K_GPU_MAX])
@pytest.mark.parametrize("tname", mr.FUSED)
def test_oracle_fits_bound(pkg, orc, tname, k):
    """The oracle's sequential f32 sum is the widest chain (C_orc = k + 32); with that C it must fit for every generator."""
    n = 16
    worst = 0.0
    for wi, kind in enumerate(mr.WEIGHT_KINDS):
        raw = _raw(pkg, orc, tname, kind, k, n, 11 + wi)
        a, o = mr.decode(tname, raw, k, n)
        for ai, act in enumerate(mr.ACT_KINDS):
            x = mr.activation(act, k, 100 + ai)
            y, err = mr.matvec(a, o, x, family="orc")
            got = orc.vec_mat_q(mr.TYPE[tname], raw, x, n).astype(np.float64)
            worst = max(worst, float((np.abs(got - y) / err).max()))
            row = 5
            rb = raw.size // n
            assert abs(orc.dot_q(mr.TYPE[tname], raw[row * rb:(row + 1) * rb], x) - y[row]) <= err[row]
    assert worst <= 1.0, worst


# ---- the bound's power: planted mistakes at the largest k
def _outlier_x(k, seed=5, at=5):
    x = np.random.default_rng(seed).standard_normal(k)
    x[at] = 1e3 * np.abs(x[:16]).max()
    return x.astype(np.float32)


def _ratio(y_bad, y, err):
    r = float((np.abs(y_bad - y) / err).max())
    print("MUTATION ratio %.3g" % r)
    return r


@pytest.fixture(scope="module")
def q4k_case(pkg, orc):
    k, n = K_GPU_MAX, 16
    raw = mr.weights("Q4_K", "full", k, n, 21)
    a, o = mr.decode("Q4_K", raw, k, n)
    x = _outlier_x(k)
    y, err = mr.matvec(a, o, x, family="mfma")
    return k, n, raw, a, o, x, y, err


def test_mutation_dropped_chunk(q4k_case):
    k, n, raw, a, o, x, y, err = q4k_case
    a2, o2 = a.copy(), o.copy()
    a2[:, 0:16] = 0.0
    o2[:, 0:16] = 0.0
    assert _ratio(mr.matvec(a2, o2, x)[0], y, err) >= 2.0


def test_mutation_neighbour_scale(q4k_case):
    k, n, raw, a, o, x, y, err = q4k_case
    b = raw.reshape(n, k // 256, 144).copy()
    b[:, 0, 4] = (b[:, 0, 4] & 0xC0) | (b[:, 0, 5] & 0x3F)          # sub-block 0 takes sub-block 1's scale
    a2, o2 = mr.decode("Q4_K", b.reshape(-1), k, n)
    assert _ratio(mr.matvec(a2, o2, x)[0], y, err) >= 2.0


def test_mutation_min_sign(q4k_case):
    k, n, raw, a, o, x, y, err = q4k_case
    o2 = o.copy()
    o2[:, 32:64] = -o2[:, 32:64]                                      # sub-block 1 (its min is 63 in block 0)
    assert _ratio(mr.matvec(a, o2, x)[0], y, err) >= 2.0


def test_mutation_quant_off_by_one(q4k_case):
    k, n, raw, a, o, x, y, err = q4k_case
    b = raw.reshape(n, k // 256, 144).copy()
    q = b[:, 0, 16 + 5] & 0x0F                                        # element 5: low nibble of qs[5]
    b[:, 0, 16 + 5] = (b[:, 0, 16 + 5] & 0xF0) | np.where(q < 15, q + 1, q - 1)
    a2, o2 = mr.decode("Q4_K", b.reshape(-1), k, n)
    assert _ratio(mr.matvec(a2, o2, x)[0], y, err) >= 2.0


def test_mutation_xq_neighbour_scale(pkg, orc):
    k, n = K_GPU_MAX, 16
    a, o = mr.decode("Q6_K", mr.weights("Q6_K", "full", k, n, 22), k, n)
    x = mr.activation("scales", k, 9).astype(np.float64)
    y, err = mr.matvec(a, o, x)
    sx = 2.0 ** np.ceil(np.log2(np.abs(x.reshape(-1, 16)).max(axis=1)))
    x2 = x.copy()
    x2[16:32] *= sx[2] / sx[1]                                        # chunk 1 read with chunk 2's scale
    assert _ratio(mr.matvec(a, o, x2)[0], y, err) >= 2.0


def test_mutation_rope_position(orc):
    k, hd, n = 4096, 128, 512
    rng = np.random.default_rng(3)
    a, o = mr.decode("Q4_K", mr.weights("Q4_K", "full", k, n, 23), k, n)
    x, nw = rng.standard_normal(k).astype(np.float32), (1 + 0.1 * rng.standard_normal(k)).astype(np.float32)
    y, err = mr.matvec(a, o, x, nw=nw)
    pos = 700
    c, s = mr.rope_cs(orc, pos, hd, 500000.0, 1.0)
    r, rerr = mr.rope(y, err, c, s, hd)
    for p2 in (pos - 1, pos + 1):
        c2, s2 = mr.rope_cs(orc, p2, hd, 500000.0, 1.0)
        assert _ratio(mr.rope(y, err, c2, s2, hd)[0], r, rerr) >= 2.0


def test_rope_table_recovery_matches_oracle_rotation(orc):
    hd, pos = 64, 37
    c, s = mr.rope_cs(orc, pos, hd, 10000.0, 1.0)
    q = np.random.default_rng(1).standard_normal((2, 1, hd)).astype(np.float32)
    rq, _ = orc.rope(q, q.copy(), pos, 10000.0, 1.0, False)
    mine, _ = mr.rope(q.reshape(-1).astype(np.float64), np.zeros(2 * hd), c, s, hd)
    assert np.all(np.abs(rq.reshape(-1) - mine) <= 4 * mr.U * np.abs(q.reshape(-1)).max())


def test_mutation_moe_weights_swapped(pkg, orc):
    k, n = K_GPU_MAX, 16
    x = _outlier_x(k)
    ys, errs = [], []
    for e in range(2):
        a, o = mr.decode("Q4_K", mr.weights("Q4_K", "full", k, n, 30 + e), k, n)
        y, err = mr.matvec(a, o, x)
        ys.append(y)
        errs.append(err)
    r = np.random.default_rng(2).standard_normal(n)
    ref, bound = mr.moe_down(ys, errs, [0.7, 0.3], r)
    bad, _ = mr.moe_down(ys, errs, [0.3, 0.7], r)
    assert _ratio(bad, ref, bound) >= 2.0


def test_router_ties_keep_lower_index():
    x = np.ones(64, np.float32)
    wr = np.zeros((8, 64), np.float32)
    wr[[1, 3, 6]] = 1.0
    sel, w, _, _ = mr.router(x, np.ones(64), 1e-5, wr, 2)
    assert list(sel) == [1, 3] and np.allclose(w, 0.5)
