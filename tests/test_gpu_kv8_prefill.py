"""The batched prompt pass over the byte KV caches (kv_cache_type int8 / FP8 E4M3 / FP8 E5M2), opted into per context with
lgh_set_prefill_policy(LGH_PREFILL_BATCH_BYTE_KV), layer by layer:

  store    kv8_pf_store_kernel<D,FMT> through lgh_op_pf_kv8_store: the block's rows quantized bit for bit as the oracle and
           lgh_op_kv_roundtrip (the decode attention's quantizers) quantize them
  block    attn_pf_kv8_kernel<D,8,FMT> through lgh_op_attention_prefill_kv8, against the float64 reference (tests/kv8_prefill_ref.py)
           within the bound of tests/attention_ref.py plus one f16 rounding
  codes    every finite FP8 code through the V operand (exact) and the K operand (within the bound)
  switch   which contexts take the path
  engine   what holds after it; slots of the multi-sequence engine; stage contexts
  model    logits after forward_batch against the oracle with the same cache format, within K x the batched path's tolerance

K_KV8 (test_model_parity) is a measurement, not a guess — tools/kv8_prefill_calibrate.py, profiles/README.md "Byte-cache prompt pass: the
tolerance factor K", the method of tests/test_gpu_tq_prefill.py's K_TQ:
  (a) the f32 batched path against the oracle, max|dlogit| / tol (tol = 1e-2 max|logit| + 1e-2), prompts 70 and 300 + 4 tokens:
      test-dense Q4_K_M 0.1478, test-dense-d128 Q4_K_M 0.1735, test-moe Q5_K_M 0.2141
  (b) the oracle alone with attn_norm / ffn_norm weights times (1 + eps u), eps scaled so that its f32-cache logits move by (a):
      eps = 2^-10.41 / 2^-10.33 / 2^-10.50; at that eps the byte-cache oracle's logits move by, in units of tol, worst of the two
      prompts, perturbation seeds 0..4:
        test-dense       int8 0.671 0.748 0.709 0.553 0.661   e4m3 1.453 0.943 1.137 1.126 1.467    e5m2 1.834 1.832 1.425 2.265 2.607
        test-dense-d128  int8 0.839 0.765 0.933 1.115 1.081   e4m3 1.493 1.602 1.587 1.407 1.361    e5m2 2.443 1.789 1.865 2.396 2.103
        test-moe         int8 21.643 0.777 0.850 2.069 1.979  e4m3 1.866 50.060 1.120 1.390 29.347  e5m2 3.019 3.710 2.437 2.096 3.507
      (test-moe's outliers are expert selections that flip: the router's top-k is as discrete as a byte, and a changed expert moves the
      logits by tens of tol in the oracle itself)
  (c) K = 2 x the largest of those = 2 x 50.060 = 100.12 (the factor 2: byte flips are discrete and five seeds do not see the tail).  That
      is the MoE model's number; the dense models are held to their own rows' K, which is smaller: 2 x 2.607 = 5.214 and
      2 x 2.443 = 4.886.
"""
import ctypes as C

import numpy as np
import pytest

import attention_ref as ar
import kv8_prefill_ref as kr
import tq_prefill_ref as tr

pytestmark = pytest.mark.gpu

K_BY_MODEL = {"test-dense": 2 * 2.607, "test-dense-d128": 2 * 2.443, "test-moe": 2 * 50.060}   # (c) above
K_KV8 = K_BY_MODEL["test-dense"]   # the engine tests run test-dense
FMT_IDS = [kr.NAMES[f] for f in kr.FORMATS]


# ---- store
STORE_CASES = [(0, 1), (0, 17), (5, 16), (19, 128)]
_store_rows = {}


def _store_inputs(orc, gpu, kvt, d):
    """128 K rows and 128 V rows per kv head, their oracle encoding and the decode quantizers' (lgh_op_kv_roundtrip), once per shape.  Row
    0 of head 0 is all zero (int8 scale 1), row 0 of head 1 has its largest element negative."""
    key = (kvt, d)
    if key not in _store_rows:
        rng = np.random.default_rng([kvt, d, 1])
        k_rows = rng.standard_normal((2, 128, d)).astype(np.float32)
        v_rows = (3.0 * rng.standard_normal((2, 128, d))).astype(np.float32)
        for rows in (k_rows, v_rows):
            rows[0, 0] = 0.0
            rows[1, 0] = -np.abs(rows[1, 0])
            rows[1, 0, 5] = -9.0
        enc = [kr.encode_rows(orc, kvt, rows) for rows in (k_rows, v_rows)]
        for rows, (b, sc) in zip((k_rows, v_rows), enc):
            for h in range(2):
                for r in range(128):
                    gb, gs, _ = gpu.op_kv_roundtrip(kvt, rows[h, r])
                    assert np.array_equal(gb, b[h, r]) and np.float32(gs) == sc[h, r], f"kv_roundtrip and the oracle differ, head {h} row {r}"
        assert enc[0][1][0, 0] == 1.0
        _store_rows[key] = (k_rows, v_rows, enc)
    return _store_rows[key]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("kvt", kr.FORMATS, ids=FMT_IDS)
def test_store_bit_exact(gpu, orc, kvt, d):
    """Every stored row (and int8 scale) equals the oracle's encoding and lgh_op_kv_roundtrip's of that f32 row; rows outside
    [pos0, pos0 + m) keep their canary bytes and scales."""
    n_kv, max_seq = 2, 160
    k_all, v_all, ((kb_e, ks_e), (vb_e, vs_e)) = _store_inputs(orc, gpu, kvt, d)
    i8 = kvt == kr.KV_INT8
    for pos0, m in STORE_CASES:
        kb = np.full((n_kv, max_seq, d), 0xA5, np.uint8)
        vb = np.full((n_kv, max_seq, d), 0x5A, np.uint8)
        ks = np.full((n_kv, max_seq), 123.5, np.float32) if i8 else None
        vs = np.full((n_kv, max_seq), -7.25, np.float32) if i8 else None
        kb_x, vb_x = kb.copy(), vb.copy()
        kb_x[:, pos0:pos0 + m] = kb_e[:, :m]
        vb_x[:, pos0:pos0 + m] = vb_e[:, :m]
        kb_g, vb_g, ks_g, vs_g = gpu.op_pf_kv8_store(kvt, k_all[:, :m], v_all[:, :m], pos0, kb, vb, ks, vs)
        np.testing.assert_array_equal(kb_g, kb_x, err_msg=f"K bytes pos0={pos0} m={m}")
        np.testing.assert_array_equal(vb_g, vb_x, err_msg=f"V bytes pos0={pos0} m={m}")
        if i8:
            ks_x, vs_x = ks.copy(), vs.copy()
            ks_x[:, pos0:pos0 + m] = ks_e[:, :m]
            vs_x[:, pos0:pos0 + m] = vs_e[:, :m]
            assert np.array_equal(ks_g.view(np.uint32), ks_x.view(np.uint32)), f"K scales pos0={pos0} m={m}"
            assert np.array_equal(vs_g.view(np.uint32), vs_x.view(np.uint32)), f"V scales pos0={pos0} m={m}"


# ---- block attention
BLOCK_CASES = [(0, 1), (0, 16), (0, 17), (3, 33), (130, 40), (250, 128)]   # partial token tiles, kv tiles that straddle pos0, more kv tiles than waves
BLOCK_ROWS = 384
_caches = {}


def _block_caches(orc, kvt, d, n_kv):
    """Byte caches [n_kv, BLOCK_ROWS, d] (+ scales) of encoded normal rows, built once per shape."""
    key = (kvt, d, n_kv)
    if key not in _caches:
        rng = np.random.default_rng([kvt, d, n_kv, 2])
        kb, ks = kr.encode_rows(orc, kvt, rng.standard_normal((n_kv, BLOCK_ROWS, d)))
        vb, vs = kr.encode_rows(orc, kvt, rng.standard_normal((n_kv, BLOCK_ROWS, d)))
        _caches[key] = (kb, vb, ks, vs) if kvt == kr.KV_INT8 else (kb, vb, None, None)
    return _caches[key]


def _poisoned(kvt, kb, vb, ks, vs, n):
    """The caches with every row >= n made unreadable: NaN bytes (FP8), NaN scales (int8)."""
    kb, vb = kb.copy(), vb.copy()
    kb[:, n:] = 0x7F
    vb[:, n:] = 0x7F
    if kvt == kr.KV_INT8:
        ks, vs = ks.copy(), vs.copy()
        ks[:, n:] = np.nan
        vs[:, n:] = np.nan
    return kb, vb, ks, vs


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("kvt", kr.FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("g", [1, 4, 8])
def test_block_attention(gpu, orc, d, kvt, g):
    n_kv = 2 * max(1, 256 // (d * g))   # n_heads * d a multiple of 256 (the XH layout's slab width), at least two kv heads
    nh = n_kv * g
    kb, vb, ks, vs = _block_caches(orc, kvt, d, n_kv)
    scale = 1.0 / np.sqrt(d)
    fails = []
    for pos0, m in BLOCK_CASES:
        rng = np.random.default_rng([d, kvt, g, pos0, m, 3])
        n = pos0 + m
        q = rng.standard_normal((m, nh, d)).astype(np.float32)
        if m == 17:
            q *= 30.0   # scores in the hundreds: the online softmax's rescaling
        ref = kr.block(orc, kvt, q, kb, vb, ks, vs, scale, pos0, m).reshape(m, nh * d)
        s_mag, vmax = kr.magnitudes(orc, kvt, q, kb, vb, ks, vs, scale, n)
        got = gpu.op_attention_prefill_kv8(kvt, q, kb, vb, ks, vs, scale, pos0)
        ratio = ar.worst_ratio(got, ref, s_mag, vmax, n, f16=True)   # (a NaN anywhere counts as infinitely wrong)
        print(f"kv8 block d={d} {kr.NAMES[kvt]} g={g} pos0={pos0} m={m}: err / bound = {ratio:.4f}")
        if not ratio <= 1.0:
            fails.append(f"pos0={pos0} m={m}: err / bound = {ratio:.3g}")
        again = gpu.op_attention_prefill_kv8(kvt, q, kb, vb, ks, vs, scale, pos0)
        assert np.array_equal(_bits(got), _bits(again)), f"two runs differ, pos0={pos0} m={m}"
        blind = gpu.op_attention_prefill_kv8(kvt, q, *_poisoned(kvt, kb, vb, ks, vs, n), scale, pos0)   # rows past the block are never read
        assert np.isfinite(blind).all() and np.array_equal(_bits(got), _bits(blind)), f"a row past the block was read, pos0={pos0} m={m}"
        if m == 33:   # tokens 0..19 see rows <= pos0 + 19: other bytes in the later rows change nothing for them
            kb2, vb2 = kb.copy(), vb.copy()
            kb2[:, pos0 + 20:] ^= 0x80   # (the sign bit: every byte stays a finite value in all three formats)
            vb2[:, pos0 + 20:] ^= 0x80
            later = gpu.op_attention_prefill_kv8(kvt, q, kb2, vb2, ks, vs, scale, pos0)
            assert np.array_equal(_bits(later[:20]), _bits(got[:20])), "a token's output depends on later rows"
            assert not np.array_equal(later[20:], got[20:])
    assert not fails, "\n".join(fails)


# ---- every FP8 code through both operands
@pytest.mark.parametrize("kvt", [kr.KV_FP8_E4M3, kr.KV_FP8_E5M2], ids=["e4m3", "e5m2"])
def test_every_fp8_code_as_a_v_element(gpu, orc, kvt):
    """One visible row with weight 1: the output is the decoded V row itself, exactly (every FP8 value is an f16); both zeros count as
    zero.  256 byte positions per call hold the 256 codes (non-finite ones replaced by 0), rotated so that each code passes through
    each byte of a dword."""
    table = ar.fp8_table(orc, kvt)
    codes = np.where(np.isfinite(table), np.arange(256), 0).astype(np.uint8)
    assert np.isfinite(table).sum() == {kr.KV_FP8_E4M3: 254, kr.KV_FP8_E5M2: 248}[kvt]
    for d in (64, 128):
        n_kv = 256 // d
        q = np.ones((1, n_kv, d), np.float32)
        kb = np.zeros((n_kv, 4, d), np.uint8)
        for roll in range(4):
            row = np.roll(codes, roll)
            vb = np.full((n_kv, 4, d), 0x7F, np.uint8)
            vb[:, 0] = row.reshape(n_kv, d)
            got = gpu.op_attention_prefill_kv8(kvt, q, kb, vb, None, None, 1.0, 0)
            want = table[row]
            bad = np.flatnonzero(got[0].astype(np.float64) != want)
            assert bad.size == 0, f"d={d} roll={roll}: codes {[hex(row[i]) for i in bad[:8]]} read {got[0][bad[:8]]}, want {want[bad[:8]]}"


@pytest.mark.parametrize("kvt", [kr.KV_FP8_E4M3, kr.KV_FP8_E5M2], ids=["e4m3", "e5m2"])
def test_every_fp8_code_as_a_k_element(gpu, orc, kvt):
    """Two rows, K row 0 = 0 and K row 1 = the codes, V = (0, 1), one-hot queries: a head's output is sigmoid(q_j x decoded K[j]) in every
    dim.  q_j = 1 / |value| puts every non-zero code's score at +-1, where a wrong mantissa bit (a factor 1.125 or 1.25) moves the
    output by a hundred bounds.  8 query heads per kv head probe 8 dims per call."""
    table = ar.fp8_table(orc, kvt)
    codes = np.where(np.isfinite(table), np.arange(256), 0).astype(np.uint8)
    one = {kr.KV_FP8_E4M3: 0x38, kr.KV_FP8_E5M2: 0x3C}[kvt]
    assert table[one] == 1.0
    for d in (64, 128):
        n_kv, g = 256 // d, 8
        kb = np.zeros((n_kv, 2, d), np.uint8)
        kb[:, 1] = codes.reshape(n_kv, d)
        vb = np.zeros((n_kv, 2, d), np.uint8)
        vb[:, 1] = one
        val = table[kb[:, 1]]                                             # [n_kv, d]
        for c in range(d // g):
            q = np.zeros((1, n_kv * g, d), np.float32)
            for h in range(n_kv):
                for i in range(g):
                    j = g * c + i
                    q[0, h * g + i, j] = 1.0 / abs(val[h, j]) if val[h, j] != 0 else 1.0
            ref = kr.block(orc, kvt, q, kb, vb, None, None, 1.0, 1, 1).reshape(1, -1)
            s_mag, vmax = kr.magnitudes(orc, kvt, q, kb, vb, None, None, 1.0, 2)
            got = gpu.op_attention_prefill_kv8(kvt, q, kb, vb, None, None, 1.0, 1)
            ratio = ar.worst_ratio(got, ref, s_mag, vmax, 2, f16=True)
            assert ratio <= 1.0, f"d={d} dims {g * c}..{g * c + g - 1}: err / bound = {ratio:.3g}"


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("kvt", [kr.KV_FP8_E4M3, kr.KV_FP8_E5M2], ids=["e4m3", "e5m2"])
def test_fp8_block_equals_f32_block_over_decoded_bytes(gpu, orc, kvt, d):
    """attn_pf_kv8_kernel and attn_pf_mfma_kernel share their softmax core (csrc/attn_block.h) and feed identical f32 operands to the
    same matrix instructions in the same order: over the oracle's decoding of the bytes the f32 op gives the byte op's output bit for
    bit (a -0 for the oracle's +0 changes no sum that starts at +0).  A part-filled token tile; a kv tile that straddles pos0 and ten
    kv tiles over eight waves.  int8 is not held to this: its scale multiplies the score, not the elements."""
    n_kv, g, max_seq = 2, 2, 160
    table = ar.fp8_table(orc, kvt)
    rng = np.random.default_rng([kvt, d, 4])
    kb = rng.integers(0, 256, (n_kv, max_seq, d), dtype=np.uint8) & np.uint8(0xBF)   # magnitude below 2: no NaN or infinity codes
    vb = rng.integers(0, 256, (n_kv, max_seq, d), dtype=np.uint8) & np.uint8(0xBF)
    kc, vc = table[kb].astype(np.float32), table[vb].astype(np.float32)
    assert np.isfinite(kc).all() and np.isfinite(vc).all()
    for pos0, m in ((0, 17), (125, 21)):
        q = rng.standard_normal((m, n_kv * g, d)).astype(np.float32)
        got = gpu.op_attention_prefill_kv8(kvt, q, kb, vb, None, None, d ** -0.5, pos0)
        want = gpu.op_attention_prefill(q, kc, vc, d ** -0.5, pos0)
        assert np.isfinite(got).all()
        assert np.array_equal(_bits(got), _bits(want)), f"pos0={pos0} m={m}: {np.count_nonzero(_bits(got) != _bits(want))} elements differ"


def test_entry_points_refuse(gpu, pkg):
    q = np.zeros((4, 2, 128), np.float32)
    b = np.zeros((2, 64, 128), np.uint8)
    sc = np.ones((2, 64), np.float32)
    rows = np.zeros((2, 4, 128), np.float32)
    for kvt in (gpu.KV_F32, gpu.KV_TQ2, gpu.KV_TQ3, gpu.KV_TQ2_QJL, gpu.KV_TQ3_QJL):
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_attention_prefill_kv8(kvt, q, b, b, sc, sc, 0.1, 0)
        assert ei.value.variant == "Unsupported"
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_pf_kv8_store(kvt, rows, rows, 0, b, b, sc, sc)
        assert ei.value.variant == "Unsupported"
    for kvt in kr.FORMATS:
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_attention_prefill_kv8(kvt, q, b, b, sc, sc, 0.1, 61)                                   # past max_seq
        assert ei.value.variant == "InvalidArgument"
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_pf_kv8_store(kvt, rows, rows, 61, b, b, sc, sc)
        assert ei.value.variant == "InvalidArgument"
        with pytest.raises(pkg.BackendError) as ei:                                                       # head_dim 32
            gpu.op_attention_prefill_kv8(kvt, np.zeros((4, 8, 32), np.float32), np.zeros((2, 64, 32), np.uint8), np.zeros((2, 64, 32), np.uint8), sc, sc, 0.1, 0)
        assert ei.value.variant == "Unsupported"
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_pf_kv8_store(kvt, np.zeros((2, 4, 32), np.float32), np.zeros((2, 4, 32), np.float32), 0, np.zeros((2, 64, 32), np.uint8),
                                np.zeros((2, 64, 32), np.uint8), sc, sc)
        assert ei.value.variant == "Unsupported"
        with pytest.raises(pkg.BackendError) as ei:                                                       # 3 and 16 query heads per kv head
            gpu.op_attention_prefill_kv8(kvt, np.zeros((4, 6, 128), np.float32), b, b, sc, sc, 0.1, 0)
        assert ei.value.variant == "Unsupported"
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_attention_prefill_kv8(kvt, np.zeros((4, 32, 128), np.float32), b, b, sc, sc, 0.1, 0)
        assert ei.value.variant == "Unsupported"


# ---- the switch
def _engine(pkg, name, mix, max_seq, kv_type, flags=0, policy=0, **kw):
    cfg = pkg.make_config(name, max_seq_len=max_seq)
    model = pkg.SynthModel(cfg, mix=mix)
    return cfg, model, pkg.HipGpuInference.from_model(model, max_seq, flags=flags, kv_cache_type=kv_type, prefill_policy=policy, **kw)


def _token_by_token_logits(pkg, model, max_seq, kvt, prompt, tok):
    eng = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=kvt)
    try:
        for t in prompt:
            eng.prefill_token(t)
        return eng.forward(tok)
    finally:
        eng.close()


@pytest.mark.parametrize("kvt", kr.FORMATS, ids=FMT_IDS)
def test_policy_switch(pkg, gpu, kvt):
    """Without the policy a byte cache's prompt is the token-by-token engine's, bit for bit; with it the context takes the batched path;
    LGH_FLAG_EXACT_PREFILL wins; unknown bits are refused and change nothing."""
    on = gpu.PREFILL_BATCH_BYTE_KV
    cfg, model, eng = _engine(pkg, "test-dense", "Q4_K_M", 64, kvt)
    _, _, exact = _engine(pkg, "test-dense", "Q4_K_M", 64, kvt, flags=gpu.FLAG_EXACT_PREFILL, policy=on)
    try:
        prompt = tr.prompt_tokens(cfg, 40)
        want = _token_by_token_logits(pkg, model, 64, kvt, prompt, 5)
        assert eng.prefill_is_batched() is False
        eng.forward_batch(prompt)
        assert np.array_equal(_bits(eng.forward(5)), _bits(want))
        with pytest.raises(pkg.BackendError) as ei:
            eng.set_prefill_policy(on | 2)
        assert ei.value.variant == "InvalidArgument" and eng.prefill_is_batched() is False
        with pytest.raises(pkg.BackendError) as ei:
            eng.set_prefill_policy(1 << 31)
        assert ei.value.variant == "InvalidArgument"
        eng.set_prefill_policy(on)
        assert eng.prefill_is_batched() is True
        eng.reset()
        eng.forward_batch(prompt)
        got = eng.forward(5)
        assert not np.array_equal(_bits(got), _bits(want))                       # another path ...
        assert np.abs(got - want).max() <= K_KV8 * tr.logit_tol(want)           # ... to the same logits
        eng.set_prefill_policy(0)                                                # and back
        assert eng.prefill_is_batched() is False
        eng.reset()
        eng.forward_batch(prompt)
        assert np.array_equal(_bits(eng.forward(5)), _bits(want))
        assert exact.prefill_is_batched() is False
        exact.forward_batch(prompt)
        assert np.array_equal(_bits(exact.forward(5)), _bits(want))
    finally:
        eng.close()
        exact.close()


def test_policy_does_nothing_on_f32_and_turboquant(pkg, gpu):
    for kvt in (gpu.KV_F32, gpu.KV_TQ3):
        cfg, model, plain = _engine(pkg, "test-dense", "Q4_K_M", 64, kvt)
        bit = pkg.HipGpuInference.from_model(model, 64, kv_cache_type=kvt, prefill_policy=gpu.PREFILL_BATCH_BYTE_KV)
        try:
            assert plain.prefill_is_batched() is True and bit.prefill_is_batched() is True
            prompt = tr.prompt_tokens(cfg, 40)
            plain.forward_batch(prompt)
            bit.forward_batch(prompt)
            assert np.array_equal(_bits(plain.forward(5)), _bits(bit.forward(5)))
            bit.batch_create(2)   # TurboQuant slots stay token by token whatever the word says: bit-identical to the own sequence's tokens
            if kvt == gpu.KV_TQ3:
                one = pkg.HipGpuInference.from_model(model, 64, kv_cache_type=kvt)
                for t in prompt[:20]:
                    one.prefill_token(t)
                bit.batch_prefill(1, prompt[:20])
                assert np.array_equal(_bits(bit.forward_multi([1], [7])[0][0]), _bits(one.forward(7)))
                one.close()
        finally:
            plain.close()
            bit.close()
    for kvt in (gpu.KV_TQ2_QJL, gpu.KV_TQ3_QJL):
        _, _, eng = _engine(pkg, "test-dense", "Q4_K_M", 32, kvt, policy=gpu.PREFILL_BATCH_BYTE_KV)
        assert eng.prefill_is_batched() is False
        eng.close()


# ---- engine
@pytest.mark.parametrize("kvt", kr.FORMATS, ids=FMT_IDS)
def test_engine_after_a_batched_prefill(pkg, orc, gpu, kvt):
    """The block scratch is not KV bytes; the same prompt twice gives the same logits; truncate / shift_left and the decode graph work on
    the rows the batched pass left; a prompt beyond the cache is refused before anything moves."""
    max_seq = 192
    cfg, model, eng = _engine(pkg, "test-dense", "Q4_K_M", max_seq, kvt, policy=gpu.PREFILL_BATCH_BYTE_KV)
    ref = tr.oracle_model(orc, cfg, model)
    kr.set_oracle_format(orc, ref, kvt)
    try:
        assert eng.prefill_is_batched()
        kv_bytes = eng.stats()["kv_bytes"]
        prompt = tr.prompt_tokens(cfg, 150)                # two blocks: 128 + 22
        eng.forward_batch(prompt)
        assert eng.position() == 150 and eng.stats()["kv_bytes"] == kv_bytes
        first = eng.forward(9)
        eng.reset()
        eng.forward_batch(prompt)
        assert np.array_equal(_bits(eng.forward(9)), _bits(first))
        ref.forward(prompt + [9])

        def close(got, want):
            err, tol = float(np.abs(got - want).max()), tr.logit_tol(want)
            print(f"{kr.NAMES[kvt]} engine: max|dlogit| = {err / tol:.3f} tol")
            return err <= K_KV8 * tol

        for e in (eng, ref):
            e.kv_shift_left(11)
        assert eng.position() == ref.position == 140
        assert close(eng.forward(5), ref.forward([5]))
        eng.kv_truncate(100)
        ref.kv_truncate(100)
        assert close(eng.forward(6), ref.forward([6]))
        eng.forward_batch(tr.prompt_tokens(cfg, 30))       # a second prompt on top: pos0 = 101, not a multiple of a tile
        ref.forward(tr.prompt_tokens(cfg, 30))
        assert close(eng.forward(7), ref.forward([7]))
        pos = eng.position()
        dev = eng.decode_greedy(3, 8).tolist()              # graph replays == the host loop
        eng.kv_truncate(pos)
        host, tok = [], 3
        for _ in range(8):
            tok = orc.argmax_last(eng.forward(tok))
            host.append(tok)
        assert dev == host
        pos = eng.position()
        with pytest.raises(pkg.BackendError) as ei:
            eng.forward_batch(list(range(max_seq)))
        assert ei.value.variant == "InvalidArgument" and eng.position() == pos
    finally:
        eng.close()
        ref.close()


# ---- slots
def _own_prompt(eng, prompt):
    """The own sequence's prompt through the block kernels.  lgh_prefill_batch hands a one-token prompt to prefill_token (for every cache
    format); lgh_stage_prefill_batch is the block entry point that lgh_batch_prefill's one-token block corresponds to."""
    if len(prompt) >= 2:
        eng.forward_batch(prompt)
    else:
        eng.stage_prefill_batch(prompt, len(prompt))
        eng.synchronize()


def _slots_against_single_engines(pkg, gpu, name, mix, kvt, lengths):
    max_seq, on = 192, gpu.PREFILL_BATCH_BYTE_KV
    cfg, model, multi = _engine(pkg, name, mix, max_seq, kvt, policy=on)
    singles = []
    try:
        multi.batch_create(4)
        assert multi.prefill_is_batched()
        prompts = [[(11 * i + 5 * s + 1) % cfg.vocab_size for i in range(n)] for s, n in enumerate(lengths)]
        slots = list(range(len(lengths)))
        for s, p in zip(slots, prompts):
            multi.batch_prefill(s, p)
            assert multi.batch_position(s) == len(p)
            one = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=kvt, prefill_policy=on)
            singles.append(one)
            _own_prompt(one, p)
            a, b = multi.prefix_save(slot=s), one.prefix_save()      # the slot's rows and the own sequence's, byte for byte
            assert a.to_bytes() == b.to_bytes(), f"slot {s}: the saved rows differ"
            a.free()
            b.free()
        toks = [3 + s for s in slots]
        for step in range(3):
            logits, nxt = multi.forward_multi(slots, toks, greedy=True)
            for s in slots:
                want = singles[s].forward(toks[s])
                assert np.array_equal(_bits(logits[s]), _bits(want)), f"slot {s} step {step}: max|d| = {np.abs(logits[s] - want).max():.3e}"
            toks = [int(t) for t in nxt]
    finally:
        multi.close()
        for e in singles:
            e.close()


@pytest.mark.parametrize("kvt", kr.FORMATS, ids=FMT_IDS)
def test_slots_equal_single_sequence_engines(pkg, gpu, kvt):
    """Ragged prompts into four slots through lgh_batch_prefill, then three multi-sequence steps: every slot's logits are those of a
    single-sequence engine of the same format and policy, bit for bit (the same kernels wrote the same rows)."""
    _slots_against_single_engines(pkg, gpu, "test-dense", "Q4_K_M", kvt, (1, 17, 130, 150))


def test_slots_of_a_moe_model(pkg, gpu):
    _slots_against_single_engines(pkg, gpu, "test-moe", "Q5_K_M", kr.KV_INT8, (1, 17, 130, 150))


# ---- stage contexts
def test_stage_blocks_reproduce_the_single_context_prompt_pass(pkg, gpu):
    """Two stage contexts with an int8 cache and the policy on, the layers split in half: after a 70-token block and one step the logits
    are the single context's, bit for bit."""
    kvt, on = kr.KV_INT8, gpu.PREFILL_BATCH_BYTE_KV
    cfg, model, full = _engine(pkg, "test-dense-d128", "Q4_K_M", 96, kvt, policy=on)
    split = cfg.num_layers // 2
    s0 = pkg.HipGpuInference.from_model(model, 96, layer_range=(0, split), kv_cache_type=kvt)
    s1 = pkg.HipGpuInference.from_model(model, 96, layer_range=(split, cfg.num_layers), kv_cache_type=kvt)
    try:
        assert not s0.prefill_is_batched() and not s1.prefill_is_batched()
        with pytest.raises(pkg.BackendError) as ei:
            s0.stage_prefill_batch([1, 2, 3], 3)
        assert ei.value.variant == "Unsupported"
        s0.set_prefill_policy(on)
        s1.set_prefill_policy(on)
        assert full.prefill_is_batched() and s0.prefill_is_batched() and s1.prefill_is_batched()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        prompt = [(5 * i + 2) % cfg.vocab_size for i in range(70)]
        full.forward_batch(prompt)
        s0.stage_prefill_batch(prompt, len(prompt))
        s0.synchronize()
        assert hip.hipMemcpy(s1.stage_hidden_block_ptr(), s0.stage_hidden_block_ptr(), len(prompt) * cfg.hidden_size * 4, 3) == 0  # D2D
        assert hip.hipDeviceSynchronize() == 0
        s1.stage_prefill_batch(None, len(prompt))
        s1.synchronize()
        assert s0.position() == s1.position() == full.position() == 70
        want = full.forward(3)
        s0.stage_forward(3)
        s0.synchronize()
        assert hip.hipMemcpy(s1.stage_hidden_ptr(), s0.stage_hidden_ptr(), cfg.hidden_size * 4, 3) == 0
        assert hip.hipDeviceSynchronize() == 0
        got = s1.stage_forward(0, want_logits=True)
        assert np.array_equal(_bits(got), _bits(want))
    finally:
        for e in (full, s0, s1):
            e.close()


# ---- model-level parity
_covered = {"steps": 0, "greedy": 0}


@pytest.mark.parametrize("name,mix", [("test-dense", "Q4_K_M"), ("test-dense-d128", "Q4_K_M"), ("test-moe", "Q5_K_M")])
@pytest.mark.parametrize("kvt", kr.FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("n_prompt", [70, 300])
def test_model_parity(pkg, orc, gpu, name, mix, kvt, n_prompt):
    """forward_batch, then 4 forward steps, against the oracle with the same cache format: within the model's K x the batched path's tolerance
    (the module docstring says where K comes from), greedy tokens identical wherever the oracle's top-1 / top-2 gap exceeds 4 x the
    measured error."""
    cfg, model, eng = _engine(pkg, name, mix, n_prompt + 8, kvt, policy=gpu.PREFILL_BATCH_BYTE_KV)
    ref = tr.oracle_model(orc, cfg, model)
    kr.set_oracle_format(orc, ref, kvt)
    try:
        assert eng.prefill_is_batched()
        prompt = tr.prompt_tokens(cfg, n_prompt)
        eng.forward_batch(prompt)
        assert eng.position() == n_prompt
        steps = tr.follow(orc, eng.forward, ref, prompt)
        print(f"{name}/{mix} {kr.NAMES[kvt]} prompt {n_prompt}: max|dlogit| / tol per step = {['%.3f' % (e / t) for e, t, _, _ in steps]}")
        for i, (err, tol, gap, same) in enumerate(steps):
            assert err <= K_BY_MODEL[name] * tol, f"step {i}: max|dlogit| = {err / tol:.3f} tol > K = {K_BY_MODEL[name]}"
            _covered["steps"] += 1
            if gap > 4 * err:
                _covered["greedy"] += 1
                assert same, f"step {i}: greedy token differs with gap {gap:.3e} vs err {err:.3e}"
        print(f"greedy-token identity asserted on {_covered['greedy']} of {_covered['steps']} steps so far")
    finally:
        eng.close()
        ref.close()
