"""Q4_1, Q5_0 and Q5_1 weights kept quantized in HBM (LGH_WEIGHTS_LEGACY_TILES): the decode mat-vec (|delta| <= 1e-4 sum|x_i w_i| + 1e-6),
the prompt GEMM (prefill_ref's f32 bound over the kernel's own f16 operands) and the engine (2e-3 max|logit| + 2e-3) against float64
references over the oracle's dequantize.  Worst measured error / bound: mat-vec 1.5e-3, GEMM 1.5e-2 (profiles/legacy_weights.md)."""
import numpy as np
import pytest

import matvec_ref as mr
import prefill_ref as pr

pytestmark = pytest.mark.gpu
TYPES = ("Q4_1", "Q5_0", "Q5_1")
ROW_BYTES, EPS = {"Q4_1": 160, "Q5_0": 176, "Q5_1": 192}, 1e-5                                   # tile bytes / 16 per 256 elements
BLOCK, QH = {"Q4_1": 20, "Q5_0": 22, "Q5_1": 24}, {"Q5_0": slice(2, 6), "Q5_1": slice(4, 8)}    # {d, [m], [qh[4]], qs[16]}


def _inputs(pkg, orc, tname, k, n, seed):
    """(raw, w, u, s, o): the generator's blocks with the minima of Q4_1 / Q5_1 redrawn in both signs independently of d (it ties m to
    -7.5 d / -15.5 d, which would hide a minimum of the wrong block or sign); the oracle's w; the unsigned quant u, scale s = d and ADDED
    minimum o = m (None for Q5_0) from the oracle over the same bytes with d 1, m 0 / quants 1, m 0 / quants 0.  Every code occurs."""
    t, bb = mr.TYPE[tname], BLOCK[tname]
    raw = pkg.synth.fill_tensor("blk.0.ffn_up.weight", t, n * k, k, 0, seed)
    b = raw.reshape(n, k // 32, bb)
    if tname != "Q5_0":
        m = (0.05 * np.random.default_rng(seed + 1).standard_normal((n, k // 32))).astype(np.float16)
        b[..., 2:4] = m.view(np.uint8).reshape(n, k // 32, 2)
        assert (m > 0).any() and (m < 0).any()
    deq = lambda bytes_: orc.dequantize(t, bytes_.reshape(-1), n * k).astype(np.float64).reshape(n, k)
    hb, qb, zb = b.copy(), b.copy(), b.copy()
    hb[..., 0:2], qb[..., bb - 16:], zb[..., bb - 16:] = (0x00, 0x3C), 0x11, 0
    if tname == "Q5_0":
        qb[..., QH[tname]] = 0xFF                                # q 17: y = d
        u, s, o = deq(hb) + 16.0, deq(qb), None
    else:
        hb[..., 2:4] = qb[..., 2:4] = 0
        if tname == "Q5_1":
            qb[..., QH[tname]] = zb[..., QH[tname]] = 0
        u, s, o = deq(hb), deq(qb), deq(zb)
    assert set(np.unique(u)) == set(range(16 if tname == "Q4_1" else 32))
    return raw, deq(b), u, s, o


@pytest.mark.parametrize("k,n", [(256, 7), (1024, 40), (5632, 33)])
@pytest.mark.parametrize("tname", TYPES)
def test_decode_matvec(gpu, pkg, orc, tname, k, n):
    """lgh_op_vec_mat_ex under the policy, with and without the norm prologue, against float64 dequantize(W) . x."""
    t, (raw, w, u, s, o) = mr.TYPE[tname], _inputs(pkg, orc, tname, k, n, 11 * k + n)
    assert pr.domain(w, 0.0, 0.0, pr.f16(s * pr.SCALE), None if o is None else pr.f16(o * pr.SCALE))
    nw = (1 + 0.2 * np.random.default_rng(k).standard_normal(k)).astype(np.float32)
    for ai, kind in enumerate(mr.ACT_KINDS):
        x = mr.activation(kind, k, 100 * ai + n)
        for norm in (None, nw):
            v = x.astype(np.float64) if norm is None else (x * norm).astype(np.float64) * mr.inv_rms(x, EPS)
            got, dev_bytes = gpu.op_vec_mat_ex(t, raw, x, n, gpu.WEIGHTS_LEGACY_TILES, norm_w=norm, eps=EPS)
            err, bound = np.abs(got - w @ v), 1e-4 * (np.abs(w) @ np.abs(v)) + 1e-6
            print("%s k=%d n=%d %s norm=%s: worst err / bound %.3g" % (tname, k, n, kind, norm is not None, float((err / bound).max())))
            assert np.all(err <= bound), (kind, norm is not None, float((err / bound).max()))
            assert dev_bytes == (n + 15) // 16 * 16 * (k // 256) * ROW_BYTES[tname]
    # without the policy the _ex entry is the existing entry point: the f32-expanded matrix, the same bits
    x = mr.activation("normal", k, 5)
    got, dev_bytes = gpu.op_vec_mat_ex(t, raw, x, n, 0)
    assert dev_bytes == 4 * n * k and np.array_equal(got.view(np.uint32), gpu.op_vec_mat(t, raw, x, n).view(np.uint32))
    got, _ = gpu.op_vec_mat_ex(t, raw, x, n, 0, norm_w=nw, eps=EPS)
    assert np.array_equal(got.view(np.uint32), gpu.op_norm_vec_mat(t, raw, x, nw, EPS, n).view(np.uint32))


@pytest.mark.parametrize("m", (1, 17, 128))
@pytest.mark.parametrize("tname", TYPES)
def test_prompt_gemm(gpu, pkg, orc, tname, m):
    """lgh_op_mat_mat_ex at k = 512, n = 48 against the float64 product of the kernel's f16 operands, prefill_ref's bound and domain."""
    k, n = 512, 48
    raw, w, u, s, o = _inputs(pkg, orc, tname, k, n, 77 + m)
    S = pr.f16(s * pr.SCALE)
    O, X = pr.f16(S * -16.0 if tname == "Q5_0" else o * pr.SCALE), pr.act_block(k, m, 3 * k + m)
    wq = pr.w_operand(tname, u, S, O)
    W, wsub = wq / pr.SCALE, pr.w_sub_term(u, S, O, wq)
    assert pr.domain(W, 0.0, X, S, O)
    splits, Xq = pr.pf_plan([n], k)[1], pr.x_operand(X)
    want, bound = pr.gemm(W, Xq, splits), pr.gemm_bound(W, wsub, Xq, splits)
    # (the operands are the format's: W' against the oracle's weights within the f16 roundings of S, O and the fma)
    assert np.all(np.abs(W - w) <= 3 * pr.UH * (np.abs(u * s) + np.abs(w) + (0 if o is None else np.abs(o))) + 2.0 ** -24)
    err = np.abs(gpu.op_mat_mat_ex(mr.TYPE[tname], raw, X, n, gpu.WEIGHTS_LEGACY_TILES) - want)
    print("%s m=%d: worst err / bound %.3g" % (tname, m, float((err / bound).max())))
    assert np.all(err <= bound), float((err / bound).max())
    with pytest.raises(pkg.BackendError) as ei:   # without the policy the type has no tile layout, as ever
        gpu.op_mat_mat_ex(mr.TYPE[tname], raw, X, n, 0)
    assert ei.value.variant == "Unsupported"


@pytest.mark.parametrize("mix", TYPES)
def test_engine(gpu, pkg, orc, mix):
    """Batched prompt + decode against the oracle without the f32 mat-vec; multi-sequence steps bit-identical; the f32 matrix-core policy."""
    _within = lambda got, want: float(np.abs(got - want).max()) <= 2e-3 * float(np.abs(want).max()) + 2e-3
    cfg = pkg.make_config("test-dense", max_seq_len=40)
    model, ref = pkg.SynthModel(cfg, mix=mix), orc.Model(cfg.as_dict())
    for name, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(name, t, ne, data)
    ref.finalize()
    make = lambda: pkg.HipGpuInference.from_model(model, 40, attn_direct=255, weight_policy=gpu.WEIGHTS_LEGACY_TILES)
    eng, single = make(), make()
    assert eng.stats()["weight_bytes"] == model.weight_bytes() and eng.prefill_is_batched()
    toks = [int(t) for t in np.random.default_rng(7).integers(0, cfg.vocab_size, size=24)]
    eng.forward_batch(toks[:20])                 # lgh_prefill_batch: the batched pass (an Unsupported status would raise)
    eng.set_profiling(True)
    for i in range(20, 24):                      # (the oracle keeps its context: the prompt rides along with the first token)
        assert _within(eng.forward(toks[i]), ref.forward(toks[:21] if i == 20 else [toks[i]])), i
    sym = eng.stats()["symbols"]
    eng.set_profiling(False)
    assert "lgh::f32_matvec_kernel" not in sym and sym["lgh::mvq_legacy_kernel<128u>"]["launches"] > 0, sym
    # ---- multi-sequence steps of 3 and 5 sequences, each bit-identical to the single-sequence context built the same way
    eng.batch_create(5)
    hist = [[int(t) for t in np.random.default_rng(50 + s).integers(0, cfg.vocab_size, size=3)] for s in range(5)]
    want, want_ref = [], []
    for h in hist:
        single.reset(), ref.reset()
        want.append([single.forward(t).copy() for t in h])
        want_ref.append([ref.forward([t]) for t in h])
    for B, f32 in ((3, False), (5, False), (3, True)):   # last: the same steps on the f32 matrix cores, inside the oracle's bound
        if f32:
            eng.set_batch_policy(gpu.BATCH_F32_MATRIX | 2 << 8)
        before = gpu.mvqf_launches()
        for s in range(B):
            eng.batch_reset(s)
        for step in range(3):
            logits, _ = eng.forward_multi(list(range(B)), [hist[s][step] for s in range(B)])
            for s in range(B):
                ok = _within(logits[s], want_ref[s][step]) if f32 else np.array_equal(logits[s].view(np.uint32), want[s][step].view(np.uint32))
                assert ok, (B, f32, s, step)
        assert (gpu.mvqf_launches() > before) == f32


def test_weight_policy_word(gpu, pkg):
    """8, 9 and 13 are accepted before the first upload; 8 after it and 2 at any time are refused and change nothing (the f32 expansion)."""
    model = pkg.SynthModel(pkg.make_config("test-dense", max_seq_len=8), mix="Q5_0")
    for word in (8, 9, 13):
        eng = pkg.HipGpuInference.from_model(model, 8, weight_policy=word)
        assert eng.stats()["weight_bytes"] == model.weight_bytes() and eng.prefill_is_batched()
    eng = pkg.HipGpuInference.from_model(model, 8)
    for call in (lambda: pkg.HipGpuInference.from_model(model, 8, weight_policy=2), lambda: eng.set_weight_policy(gpu.WEIGHTS_LEGACY_TILES)):
        with pytest.raises(pkg.BackendError) as ei:
            call()
        assert ei.value.variant == "InvalidArgument"
    f32_bytes = sum(s.n_elems * 4 if len(s.ne) == 2 and s.name != "token_embd.weight" else s.nbytes for s in model.specs())
    assert eng.stats()["weight_bytes"] == f32_bytes and not eng.prefill_is_batched()
