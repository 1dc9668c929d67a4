"""The batched prompt pass over a TurboQuantProd KV cache (kv_cache_type tq2-qjl / tq3-qjl) behind LGH_PREFILL_BATCH_TQ_QJL, layer by layer:

  store    tq_pf_rows_qjl_kernel<D,BITS> through lgh_op_pf_tq_store_qjl: codes and QJL words bit for bit as the oracle compresses the rows
  block    the same kernel (expand + query rotation) + attn_pf_tq_qjl_kernel<D,8> through lgh_op_attention_prefill_tq_qjl, against the
           float64 reference (tests/tq_qjl_prefill_ref.py) within the derived TurboQuant bound of tests/attention_ref.py, whose S carries
           the QJL term, plus one f16 rounding
  engine   which contexts take the path, and what holds after it
  model    logits after forward_batch against the oracle with the same signs and projection matrices, within K_QJL x the batched path's
           tolerance

K_QJL is measured as K_TQ was (tests/test_gpu_tq_prefill.py), with step (b) over the TurboQuantProd oracle — tools/tq_prefill_calibrate.py
--qjl, profiles/README.md "TurboQuantProd prompt pass: the tolerance factor K_QJL".  At the eps that moves the f32-cache oracle's logits
by (a) = 0.1478 / 0.1735 / 0.2141 tol, the TurboQuantProd oracle's logits move by, in units of tol, worst of the two prompts,
perturbation seeds 0..4:
    test-dense       tq2-qjl 4.726 4.595 1.940 4.846 5.172       tq3-qjl 3.261 5.291 10.522 16.295 3.520
    test-dense-d128  tq2-qjl 3.757 12.338 5.130 3.659 4.123      tq3-qjl 9.772 11.868 16.968 19.331 4.871
    test-moe         tq2-qjl 7.923 6.222 46.370 6.832 47.417     tq3-qjl 7.339 7.129 59.837 58.464 15.144
K_QJL = 2 x the largest of those = 2 x 59.837 = 119.67 (the factor 2 as for K_TQ: code-cell and sign-bit flips are discrete, their
effect heavy-tailed, and five seeds do not see the tail).  The figures are 3 - 10 x K_TQ's: a flipped sign bit moves a score by
2 coeff |r| |(S rq)_i| with S's entries of unit variance, and test-moe's largest ones are flipped expert selections, as in the byte
caches' table.  Each model is therefore held to twice the largest figure of its OWN row, K_QJL_MODEL below, which is K_QJL for
test-moe and stricter for the dense models (the byte-cache prompt pass does the same).
The batched path itself measured 0.86 ... 18.98 tol on the dense models (worst: test-dense-d128 tq3-qjl, prompt 70, under its 38.66) and
2.19 ... 46.95 tol on test-moe over the 12 cases x 4 steps of test_model_parity.
"""
import numpy as np
import pytest

import attention_ref as ar
import tq_prefill_ref as tr
import tq_qjl_prefill_ref as qr

pytestmark = pytest.mark.gpu

K_QJL = 2 * 59.837   # the table's largest figure
K_QJL_MODEL = {"test-dense": 2 * 16.295, "test-dense-d128": 2 * 19.331, "test-moe": K_QJL}


def _kv_type(gpu, bits):
    return gpu.KV_TQ2_QJL if bits == 2 else gpu.KV_TQ3_QJL


def _compress_rows(orc, rows, bits, signs_k, S):
    """rows [n_kv, n, d] f32 -> the oracle's (code rows [n_kv, n, row bytes], QJL words [n_kv, n, d / 32 + 1] uint32)."""
    out = [[orc.tq_compress_qjl(x, bits, signs_k[h], S[h]) for x in rows[h]] for h in range(rows.shape[0])]
    codes = np.stack([np.stack([c for c, _, _ in r]) for r in out])
    words = np.stack([np.stack([np.concatenate([b.view(np.uint32), np.float32([nrm]).view(np.uint32)]) for _, b, nrm in r]) for r in out])
    return codes, words


# ---- store
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("bits", [2, 3])
def test_store_bit_exact(gpu, orc, d, bits):
    """Every stored K row's codes and QJL words equal the oracle's tq_compress_qjl of that f32 row, V's codes its tq_compress; rows
    outside [pos0, pos0 + m) keep their canaries."""
    n_kv, max_seq, rb = 2, 160, tr.row_bytes(bits, d)
    for pos0, m in [(0, 1), (5, 16), (19, 128)]:
        rng = np.random.default_rng([d, bits, pos0, m, 1])
        signs = tr.make_signs(rng, n_kv, d)
        S = rng.standard_normal((n_kv, d, d)).astype(np.float32)
        k_rows = rng.standard_normal((n_kv, m, d)).astype(np.float32)
        v_rows = (3.0 * rng.standard_normal((n_kv, m, d))).astype(np.float32)
        kc = np.full((n_kv, max_seq, rb), 0xA5, np.uint8)
        vc = np.full((n_kv, max_seq, rb), 0x5A, np.uint8)
        kx = np.full((n_kv, max_seq, d // 32 + 1), 0xC3C3C3C3, np.uint32)
        kc_x, vc_x, kx_x = kc.copy(), vc.copy(), kx.copy()
        kc_x[:, pos0:pos0 + m], kx_x[:, pos0:pos0 + m] = _compress_rows(orc, k_rows, bits, signs[:, 0], S)
        vc_x[:, pos0:pos0 + m] = tr.compress_rows(orc, v_rows, bits, signs[:, 1])
        kc_g, vc_g, kx_g = gpu.op_pf_tq_store_qjl(_kv_type(gpu, bits), k_rows, v_rows, pos0, signs, S, kc, vc, kx)
        np.testing.assert_array_equal(kc_g, kc_x, err_msg=f"K codes pos0={pos0} m={m}")
        np.testing.assert_array_equal(vc_g, vc_x, err_msg=f"V codes pos0={pos0} m={m}")
        np.testing.assert_array_equal(kx_g, kx_x, err_msg=f"K QJL words pos0={pos0} m={m}")


# ---- block attention
BLOCK_CASES = [(0, 1), (0, 17), (3, 33), (130, 40), (250, 128)]   # a part-filled token tile, kv tiles that straddle pos0, more kv tiles than waves
BLOCK_ROWS = 384
_caches = {}


def _block_cache(orc, d, bits, n_kv):
    """Code caches, QJL words, signs and projection matrices of BLOCK_ROWS random rows, built once per shape."""
    key = (d, bits, n_kv)
    if key not in _caches:
        rng = np.random.default_rng([d, bits, n_kv, 2])
        signs = tr.make_signs(rng, n_kv, d)
        S = rng.standard_normal((n_kv, d, d)).astype(np.float32)
        kc, kx = _compress_rows(orc, rng.standard_normal((n_kv, BLOCK_ROWS, d)).astype(np.float32), bits, signs[:, 0], S)
        vc = tr.compress_rows(orc, rng.standard_normal((n_kv, BLOCK_ROWS, d)).astype(np.float32), bits, signs[:, 1])
        _caches[key] = (signs, S, kc, vc, kx)
    return _caches[key]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("bits", [2, 3])
@pytest.mark.parametrize("g", [1, 4])
def test_block_attention(gpu, orc, d, bits, g):
    n_kv = 2 * max(1, 256 // (d * g))   # n_heads * d a multiple of 256 (the XH layout's slab width), at least two kv heads
    nh = n_kv * g
    signs, S, kc, vc, kx = _block_cache(orc, d, bits, n_kv)
    scale = 1.0 / np.sqrt(d)
    kvt = _kv_type(gpu, bits)
    fails = []
    for pos0, m in BLOCK_CASES:
        rng = np.random.default_rng([d, bits, g, pos0, m, 3])
        n = pos0 + m
        q = rng.standard_normal((m, nh, d)).astype(np.float32)
        if m == 17:
            q *= 30.0   # scores in the hundreds: the online softmax's rescaling
        ref, s_mag, vmax = qr.block(orc, q, kc, vc, kx, bits, signs, S, scale, pos0)
        got = gpu.op_attention_prefill_tq_qjl(kvt, q, kc, vc, kx, signs, S, scale, pos0)
        ratio = ar.worst_ratio(got, ref.reshape(m, nh * d), s_mag, vmax, n, f16=True)   # (a NaN anywhere counts as infinitely wrong)
        print(f"tq-qjl block d={d} bits={bits} g={g} pos0={pos0} m={m}: err / bound = {ratio:.4f}")
        if not ratio <= 1.0:
            fails.append(f"pos0={pos0} m={m}: err / bound = {ratio:.3g}")
        again = gpu.op_attention_prefill_tq_qjl(kvt, q, kc, vc, kx, signs, S, scale, pos0)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), f"two runs differ, pos0={pos0} m={m}"
        if m == 33:
            # tokens 0..19 see rows <= pos0 + 19: other sign words and norms in the later rows change nothing for them
            kx2 = kx.copy()
            kx2[:, pos0 + 20:] ^= 0x5B5B5B5B
            later = gpu.op_attention_prefill_tq_qjl(kvt, q, kc, vc, kx2, signs, S, scale, pos0)
            assert np.array_equal(later[:20].view(np.uint32), got[:20].view(np.uint32)), "a token's output depends on later rows' QJL words"
            assert not np.array_equal(later[20:], got[20:])
            # an all-zero S: the correction is additive and the sign operand does not leak into the code scores
            S0 = np.zeros_like(S)
            _, s_mag0, vmax0 = qr.block(orc, q, kc, vc, kx, bits, signs, S0, scale, pos0)
            got0 = gpu.op_attention_prefill_tq_qjl(kvt, q, kc, vc, kx, signs, S0, scale, pos0)
            mse = gpu.op_attention_prefill_tq(gpu.KV_TQ2 if bits == 2 else gpu.KV_TQ3, q, kc, vc, signs, scale, pos0)
            r0 = ar.worst_ratio(got0, mse, s_mag0, vmax0, n, f16=True)
            print(f"tq-qjl block d={d} bits={bits} g={g}: zero S against the tq{bits} kernel, err / bound = {r0:.4f}")
            assert r0 <= 1.0
    assert not fails, "\n".join(fails)


# ---- engine
def _model_inputs(cfg, bits):
    qjl = np.random.default_rng(17 + bits).standard_normal(cfg.num_layers * cfg.num_kv_heads * cfg.head_dim * cfg.head_dim).astype(np.float32)
    return tr.model_signs(cfg, 7 + bits), qjl


def test_policy_bit(pkg, gpu):
    """Opt-in: a QJL context is batched with the bit only, never under LGH_FLAG_EXACT_PREFILL; the bit changes nothing elsewhere."""
    bit = gpu.PREFILL_BATCH_TQ_QJL
    model = pkg.SynthModel(pkg.make_config("test-dense", max_seq_len=32), mix="Q4_K_M")
    for kvt, flags, before, after in ((gpu.KV_TQ2_QJL, 0, False, True), (gpu.KV_TQ3_QJL, 0, False, True),
                                      (gpu.KV_TQ3_QJL, gpu.FLAG_EXACT_PREFILL, False, False), (gpu.KV_INT8, 0, False, False),
                                      (gpu.KV_TQ3, 0, True, True)):
        eng = pkg.HipGpuInference.from_model(model, 32, flags=flags, kv_cache_type=kvt)
        try:
            assert eng.prefill_is_batched() == before, (kvt, flags)
            eng.set_prefill_policy(bit)
            assert eng.prefill_is_batched() == after, (kvt, flags)
            eng.set_prefill_policy(0)
            assert eng.prefill_is_batched() == before, (kvt, flags)
        finally:
            eng.close()


@pytest.mark.parametrize("bits", [2, 3])
def test_bit_cleared_is_bit_identical_to_prefill_token(pkg, gpu, bits):
    cfg = pkg.make_config("test-dense", max_seq_len=64)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    a = pkg.HipGpuInference.from_model(model, 64, kv_cache_type=_kv_type(gpu, bits), prefill_policy=gpu.PREFILL_BATCH_TQ_QJL)
    b = pkg.HipGpuInference.from_model(model, 64, kv_cache_type=_kv_type(gpu, bits))
    try:
        a.set_prefill_policy(0)
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
    """Truncate, a second batched prompt at a pos0 that is no multiple of a tile, and the decode graph work on the rows (codes and QJL
    words) the batched pass left."""
    max_seq = 192
    cfg = pkg.make_config("test-dense", max_seq_len=max_seq)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    signs, qjl = _model_inputs(cfg, bits)
    ref = tr.oracle_model(orc, cfg, model)
    ref.set_kv_turboquant(bits, signs)
    ref.set_kv_turboquant_qjl(qjl)
    eng = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=_kv_type(gpu, bits), kv_rotation_signs=signs, kv_qjl_matrices=qjl,
                                         prefill_policy=gpu.PREFILL_BATCH_TQ_QJL)
    try:
        assert eng.prefill_is_batched()
        prompt = tr.prompt_tokens(cfg, 150)                # two blocks: 128 + 22
        eng.forward_batch(prompt)
        assert eng.position() == 150
        ref.forward(prompt)
        eng.kv_truncate(100)
        ref.kv_truncate(100)
        eng.forward_batch(tr.prompt_tokens(cfg, 30))       # a second prompt on top: pos0 = 100, not a multiple of a tile
        ref.forward(tr.prompt_tokens(cfg, 30))
        got, want = eng.forward(7), ref.forward([7])
        err, tol = float(np.abs(got - want).max()), tr.logit_tol(want)
        print(f"tq{bits}-qjl engine: max|dlogit| = {err / tol:.3f} tol")
        assert err <= K_QJL_MODEL["test-dense"] * tol
        pos = eng.position()
        dev = eng.decode_greedy(3, 8).tolist()              # graph replays == the host loop
        eng.kv_truncate(pos)
        host, tok = [], 3
        for _ in range(8):
            tok = orc.argmax_last(eng.forward(tok))
            host.append(tok)
        assert dev == host
    finally:
        eng.close()
        ref.close()


# ---- model-level parity
@pytest.mark.parametrize("name,mix", [("test-dense", "Q4_K_M"), ("test-dense-d128", "Q4_K_M"), ("test-moe", "Q5_K_M")])
@pytest.mark.parametrize("bits", [2, 3])
@pytest.mark.parametrize("n_prompt", [70, 300])
def test_model_parity(pkg, orc, gpu, name, mix, bits, n_prompt):
    """forward_batch, then 4 forward steps, against the oracle's TurboQuantProd cache with the same signs and matrices: within K_QJL_MODEL x the
    batched path's tolerance (the module docstring says where it comes from), greedy tokens identical wherever the oracle's top-1 /
    top-2 gap exceeds 4 x the measured error."""
    cfg = pkg.make_config(name, max_seq_len=n_prompt + 8)
    model = pkg.SynthModel(cfg, mix=mix)
    signs, qjl = _model_inputs(cfg, bits)
    ref = tr.oracle_model(orc, cfg, model)
    ref.set_kv_turboquant(bits, signs)
    ref.set_kv_turboquant_qjl(qjl)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len, kv_cache_type=_kv_type(gpu, bits), kv_rotation_signs=signs, kv_qjl_matrices=qjl,
                                         prefill_policy=gpu.PREFILL_BATCH_TQ_QJL)
    try:
        assert eng.prefill_is_batched()
        prompt = tr.prompt_tokens(cfg, n_prompt)
        eng.forward_batch(prompt)
        assert eng.position() == n_prompt
        steps = tr.follow(orc, eng.forward, ref, prompt)
        print(f"{name}/{mix} tq{bits}-qjl prompt {n_prompt}: max|dlogit| / tol per step = {['%.3f' % (e / t) for e, t, _, _ in steps]}")
        for i, (err, tol, gap, same) in enumerate(steps):
            assert err <= K_QJL_MODEL[name] * tol, f"step {i}: max|dlogit| = {err / tol:.3f} tol > K = {K_QJL_MODEL[name]}"
            if gap > 4 * err:
                assert same, f"step {i}: greedy token differs with gap {gap:.3e} vs err {err:.3e}"
    finally:
        eng.close()
        ref.close()
