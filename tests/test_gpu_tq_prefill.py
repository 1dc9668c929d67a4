"""The batched prompt pass over a TurboQuantMSE KV cache (kv_cache_type tq2 / tq3), layer by layer:

  store    tq_pf_rows_kernel<D,BITS> through lgh_op_pf_tq_store: the block's rows compressed bit for bit as the oracle compresses them
  block    tq_pf_rows_kernel (expand + query rotation) + attn_pf_mfma_kernel<D,8,TQ> through lgh_op_attention_prefill_tq, against the
           float64 reference (tests/tq_prefill_ref.py) within the derived TurboQuant bound of tests/attention_ref.py plus one f16 rounding
  engine   which contexts take the path, and what holds after it
  model    logits after forward_batch against the oracle with the same sign vectors, within K x the batched path's tolerance

K_TQ (test_model_parity) is a measurement, not a guess — tools/tq_prefill_calibrate.py, profiles/README.md "TurboQuant prompt pass: the
tolerance factor K":
  (a) the f32 batched path against the oracle, max|dlogit| / tol (tol = 1e-2 max|logit| + 1e-2), prompts 70 and 300 + 4 tokens:
      test-dense Q4_K_M 0.1478, test-dense-d128 Q4_K_M 0.1735, test-moe Q5_K_M 0.2141
  (b) the oracle alone with attn_norm / ffn_norm weights times (1 + eps u), eps scaled so that its f32-cache logits move by (a):
      eps = 2^-10.41 / 2^-10.33 / 2^-10.50 (7.37e-4 / 7.74e-4 / 6.89e-4); at that eps the TurboQuant oracle's logits move by, in units of
      tol, worst of the two prompts, perturbation seeds 0..4:
        test-dense       tq2 1.548 1.752 1.847 1.303 1.698   tq3 0.884 1.287 1.414 1.025 1.247
        test-dense-d128  tq2 1.799 1.505 2.073 1.449 1.877   tq3 0.932 1.040 1.183 1.204 1.201
        test-moe         tq2 1.916 1.527 1.607 1.200 1.154   tq3 1.082 1.184 0.905 1.550 0.854
  (c) K = 2 x the largest of those = 2 x 2.073 = 4.146 (the factor 2: cell flips are discrete, their effect heavy-tailed, and five
      seeds do not see the tail)
The batched path itself measured 0.38 ... 1.79 tol over the 12 cases of test_model_parity (worst: test-dense-d128 tq2, prompt 70), while
the token-by-token engine stays below 0.09 tol of the oracle on the same cases.
"""
import numpy as np
import pytest

import attention_ref as ar
import tq_prefill_ref as tr

pytestmark = pytest.mark.gpu

K_TQ = 2 * 2.073   # (c) above


def _kv_type(gpu, bits):
    return gpu.KV_TQ2 if bits == 2 else gpu.KV_TQ3


# ---- store
STORE_CASES = [(0, 1), (0, 17), (5, 16), (19, 128)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("bits", [2, 3])
def test_store_bit_exact(gpu, orc, d, bits):
    """Every stored code row equals the oracle's compression of that f32 row; rows outside [pos0, pos0 + m) keep their canary bytes."""
    n_kv, max_seq, rb = 2, 160, tr.row_bytes(bits, d)
    for pos0, m in STORE_CASES:
        rng = np.random.default_rng([d, bits, pos0, m, 1])
        signs = tr.make_signs(rng, n_kv, d)
        k_rows = rng.standard_normal((n_kv, m, d)).astype(np.float32)
        v_rows = (3.0 * rng.standard_normal((n_kv, m, d))).astype(np.float32)
        kc = np.full((n_kv, max_seq, rb), 0xA5, np.uint8)
        vc = np.full((n_kv, max_seq, rb), 0x5A, np.uint8)
        kc_x, vc_x = kc.copy(), vc.copy()
        kc_x[:, pos0:pos0 + m] = tr.compress_rows(orc, k_rows, bits, signs[:, 0])
        vc_x[:, pos0:pos0 + m] = tr.compress_rows(orc, v_rows, bits, signs[:, 1])
        kc_g, vc_g = gpu.op_pf_tq_store(_kv_type(gpu, bits), k_rows, v_rows, pos0, signs, kc, vc)
        np.testing.assert_array_equal(kc_g, kc_x, err_msg=f"K codes pos0={pos0} m={m}")
        np.testing.assert_array_equal(vc_g, vc_x, err_msg=f"V codes pos0={pos0} m={m}")


# ---- block attention
BLOCK_CASES = [(0, 1), (0, 16), (0, 17), (3, 33), (130, 40), (250, 128)]   # partial token tiles, kv tiles that straddle pos0, more kv tiles than waves
BLOCK_ROWS = 384
_codes = {}


def _block_codes(orc, d, bits, n_kv):
    """Code caches [n_kv, BLOCK_ROWS, row bytes] of random rows and their signs, built once per shape."""
    key = (d, bits, n_kv)
    if key not in _codes:
        rng = np.random.default_rng([d, bits, n_kv, 2])
        signs = tr.make_signs(rng, n_kv, d)
        kc = tr.compress_rows(orc, rng.standard_normal((n_kv, BLOCK_ROWS, d)).astype(np.float32), bits, signs[:, 0])
        vc = tr.compress_rows(orc, rng.standard_normal((n_kv, BLOCK_ROWS, d)).astype(np.float32), bits, signs[:, 1])
        _codes[key] = (signs, kc, vc)
    return _codes[key]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("bits", [2, 3])
@pytest.mark.parametrize("g", [1, 4, 8])
def test_block_attention(gpu, orc, d, bits, g):
    n_kv = 2 * max(1, 256 // (d * g))   # n_heads * d a multiple of 256 (the XH layout's slab width), at least two kv heads
    nh = n_kv * g
    signs, kc, vc = _block_codes(orc, d, bits, n_kv)
    scale = 1.0 / np.sqrt(d)
    kvt = _kv_type(gpu, bits)
    fails = []
    for pos0, m in BLOCK_CASES:
        rng = np.random.default_rng([d, bits, g, pos0, m, 3])
        n = pos0 + m
        q = rng.standard_normal((m, nh, d)).astype(np.float32)
        if m == 17:
            q *= 30.0   # scores in the hundreds: the online softmax's rescaling
        ref = tr.block(orc, q, kc, vc, bits, signs, scale, pos0, m).reshape(m, nh * d)
        s_mag, vmax = tr.magnitudes(orc, q, kc, vc, bits, signs, scale, n)
        got = gpu.op_attention_prefill_tq(kvt, q, kc, vc, signs, scale, pos0)
        ratio = ar.worst_ratio(got, ref, s_mag, vmax, n, f16=True)   # (a NaN anywhere counts as infinitely wrong)
        print(f"tq block d={d} bits={bits} g={g} pos0={pos0} m={m}: err / bound = {ratio:.4f}")
        if not ratio <= 1.0:
            fails.append(f"pos0={pos0} m={m}: err / bound = {ratio:.3g}")
        again = gpu.op_attention_prefill_tq(kvt, q, kc, vc, signs, scale, pos0)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), f"two runs differ, pos0={pos0} m={m}"
        if m == 33:   # tokens 0..19 see rows <= pos0 + 19: other bytes in the later rows change nothing for them
            kc2, vc2 = kc.copy(), vc.copy()
            kc2[:, pos0 + 20:] ^= 0x5B
            vc2[:, pos0 + 20:] ^= 0xC6
            later = gpu.op_attention_prefill_tq(kvt, q, kc2, vc2, signs, scale, pos0)
            assert np.array_equal(later[:20].view(np.uint32), got[:20].view(np.uint32)), "a token's output depends on later rows"
            assert not np.array_equal(later[20:], got[20:])
    assert not fails, "\n".join(fails)


def test_entry_points_refuse(gpu, pkg):
    q = np.zeros((4, 2, 128), np.float32)
    codes = np.zeros((2, 64, 32), np.uint8)
    signs = np.ones((2, 2, 128), np.float32)
    for kvt in (gpu.KV_F32, gpu.KV_INT8, gpu.KV_TQ2_QJL, gpu.KV_TQ3_QJL):
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_attention_prefill_tq(kvt, q, codes, codes, signs, 0.1, 0)
        assert ei.value.variant == "Unsupported"
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_pf_tq_store(kvt, np.zeros((2, 4, 128), np.float32), np.zeros((2, 4, 128), np.float32), 0, signs, codes, codes)
        assert ei.value.variant == "Unsupported"
    with pytest.raises(pkg.BackendError) as ei:
        gpu.op_attention_prefill_tq(gpu.KV_TQ2, q, codes, codes, signs, 0.1, 61)          # past max_seq
    assert ei.value.variant == "InvalidArgument"
    with pytest.raises(pkg.BackendError) as ei:
        gpu.op_pf_tq_store(gpu.KV_TQ2, np.zeros((2, 4, 128), np.float32), np.zeros((2, 4, 128), np.float32), 61, signs, codes, codes)
    assert ei.value.variant == "InvalidArgument"
    with pytest.raises(pkg.BackendError) as ei:
        gpu.op_attention_prefill_tq(gpu.KV_TQ2, q, codes, codes, 2.0 * signs, 0.1, 0)     # not a sign vector
    assert ei.value.variant == "InvalidArgument"


# ---- engine
def _engine(pkg, name, mix, max_seq, kv_type, flags=0, signs=None):
    cfg = pkg.make_config(name, max_seq_len=max_seq)
    model = pkg.SynthModel(cfg, mix=mix)
    return cfg, model, pkg.HipGpuInference.from_model(model, max_seq, flags=flags, kv_cache_type=kv_type, kv_rotation_signs=signs)


def test_which_contexts_take_the_batched_path(pkg, gpu):
    """tq2 and tq3 take it (on the parent commit they did not); the QJL types, int8, FP8 and LGH_FLAG_EXACT_PREFILL do not."""
    for kvt, flags, want in ((gpu.KV_TQ2, 0, True), (gpu.KV_TQ3, 0, True), (gpu.KV_TQ2_QJL, 0, False), (gpu.KV_TQ3_QJL, 0, False),
                             (gpu.KV_INT8, 0, False), (gpu.KV_FP8_E4M3, 0, False), (gpu.KV_FP8_E5M2, 0, False),
                             (gpu.KV_TQ2, gpu.FLAG_EXACT_PREFILL, False), (gpu.KV_TQ3, gpu.FLAG_EXACT_PREFILL, False)):
        _, _, eng = _engine(pkg, "test-dense", "Q4_K_M", 32, kvt, flags)
        try:
            assert eng.prefill_is_batched() == want, (kvt, flags)
        finally:
            eng.close()


@pytest.mark.parametrize("bits", [2, 3])
def test_exact_prefill_flag_is_bit_identical_to_prefill_token(pkg, gpu, bits):
    cfg, model, a = _engine(pkg, "test-dense", "Q4_K_M", 64, _kv_type(gpu, bits), gpu.FLAG_EXACT_PREFILL)
    b = pkg.HipGpuInference.from_model(model, 64, kv_cache_type=_kv_type(gpu, bits))
    try:
        prompt = tr.prompt_tokens(cfg, 40)
        a.forward_batch(prompt)
        for t in prompt:
            b.prefill_token(t)
        for tok in (5, 900):
            assert np.array_equal(a.forward(tok).view(np.uint32), b.forward(tok).view(np.uint32))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("bits", [2, 3])
def test_engine_after_a_batched_prefill(pkg, orc, gpu, bits):
    """The scratch is not KV bytes; the same prompt twice gives the same logits; truncate / shift_left and the decode graph work on the
    rows the batched pass left; a prompt beyond the cache is refused before anything moves."""
    max_seq = 192
    cfg = pkg.make_config("test-dense", max_seq_len=max_seq)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    signs = tr.model_signs(cfg, 7 + bits)
    ref = tr.oracle_model(orc, cfg, model)
    ref.set_kv_turboquant(bits, signs)
    eng = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=_kv_type(gpu, bits), kv_rotation_signs=signs)
    try:
        assert eng.prefill_is_batched()
        kv_bytes = eng.stats()["kv_bytes"]
        prompt = tr.prompt_tokens(cfg, 150)                # two blocks: 128 + 22
        eng.forward_batch(prompt)
        assert eng.position() == 150 and eng.stats()["kv_bytes"] == kv_bytes
        first = eng.forward(9)
        eng.reset()
        eng.forward_batch(prompt)
        assert np.array_equal(eng.forward(9).view(np.uint32), first.view(np.uint32))
        ref.forward(prompt + [9])

        def close(got, want):
            err, tol = float(np.abs(got - want).max()), tr.logit_tol(want)
            print(f"tq{bits} engine: max|dlogit| = {err / tol:.3f} tol")
            return err <= K_TQ * tol

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


# ---- model-level parity
@pytest.mark.parametrize("name,mix", [("test-dense", "Q4_K_M"), ("test-dense-d128", "Q4_K_M"), ("test-moe", "Q5_K_M")])
@pytest.mark.parametrize("bits", [2, 3])
@pytest.mark.parametrize("n_prompt", [70, 300])
def test_model_parity(pkg, orc, gpu, name, mix, bits, n_prompt):
    """forward_batch, then 4 forward steps, against the oracle's TurboQuant cache with the same signs: within K_TQ x the batched path's
    tolerance (the module docstring says where K_TQ comes from), greedy tokens identical wherever the oracle's top-1 / top-2 gap
    exceeds 4 x the measured error."""
    cfg = pkg.make_config(name, max_seq_len=n_prompt + 8)
    model = pkg.SynthModel(cfg, mix=mix)
    signs = tr.model_signs(cfg, 7 + bits)
    ref = tr.oracle_model(orc, cfg, model)
    ref.set_kv_turboquant(bits, signs)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len, kv_cache_type=_kv_type(gpu, bits), kv_rotation_signs=signs)
    try:
        assert eng.prefill_is_batched()
        prompt = tr.prompt_tokens(cfg, n_prompt)
        eng.forward_batch(prompt)
        assert eng.position() == n_prompt
        steps = tr.follow(orc, eng.forward, ref, prompt)
        print(f"{name}/{mix} tq{bits} prompt {n_prompt}: max|dlogit| / tol per step = {['%.3f' % (e / t) for e, t, _, _ in steps]}")
        for i, (err, tol, gap, same) in enumerate(steps):
            assert err <= K_TQ * tol, f"step {i}: max|dlogit| = {err / tol:.3f} tol > K = {K_TQ}"
            if gap > 4 * err:
                assert same, f"step {i}: greedy token differs with gap {gap:.3e} vs err {err:.3e}"
    finally:
        eng.close()
        ref.close()
