"""Q3_K and Q2_K weights kept quantized in HBM (lgh_set_weight_policy: LGH_WEIGHTS_LOWBIT_TILES) and multiplied on the matrix cores:
the decode mat-vec, the prompt GEMM and the engine (batched prompt, decode, multi-sequence steps) against float64 references.

The formats are the reference's sequential layouts (dequant.rs:129-200), restated by the oracle's dequantize — the reference of every
check here.  Bounds: the mat-vec's standing |delta| <= 1e-4 sum|x_i w_i| + 1e-6; the GEMM's f32-accumulation bound of
tests/prefill_ref.py over the kernel's own f16 operands; the engine's 2e-3 max|logit| + 2e-3 against orc.Model.forward."""
import numpy as np
import pytest

import matvec_ref as mr
import prefill_ref as pr

pytestmark = pytest.mark.gpu

TYPES = ("Q3_K", "Q2_K")
ROW_BYTES = {"Q3_K": 114, "Q2_K": 84}          # tile bytes / 16 per 256 elements
BLOCK = {"Q3_K": 110, "Q2_K": 84}
EPS = 1e-5


def _raw(pkg, tname, k, n, seed):
    """Valid blocks from the synthetic generator in which every quant, scale and min code occurs."""
    raw = pkg.synth.fill_tensor("blk.0.ffn_up.weight", mr.TYPE[tname], n * k, k, 0, seed)
    b = raw.reshape(n, k // 256, BLOCK[tname])
    if tname == "Q2_K":   # (the generator draws scales 1..15 with the min tied to them: one block with all 16 codes of both)
        b[0, 0, :16] = np.arange(16) | (15 - np.arange(16)) << 4
        assert set(b[..., :16].ravel() & 15) == set(range(16)) and set(b[..., :16].ravel() >> 4) == set(range(16))
    else:                 # (four blocks whose 6-bit scales are 0..63, packed as the format's 3-byte groups)
        v = np.arange(64).reshape(4, 4, 4)
        groups = np.stack([v[..., 0] | (v[..., 1] & 3) << 6, v[..., 1] >> 2 | (v[..., 2] & 15) << 4, v[..., 2] >> 4 | v[..., 3] << 2], -1)
        b[:4, 0, 96:108] = groups.reshape(4, 12)
    return raw


def _fields(orc, tname, raw, k, n):
    """(u, s, o) as prefill_ref.fields reads them: the unsigned quant, the per-element scale and the subtracted min, from the oracle's
    dequantization of the same bytes with every header field set to one / every quant set to one / every quant zero."""
    t, b = mr.TYPE[tname], raw.reshape(n, k // 256, BLOCK[tname])
    deq = lambda bytes_: orc.dequantize(t, bytes_.reshape(-1), n * k).astype(np.float64).reshape(n, k)
    hb, qb, zb = b.copy(), b.copy(), b.copy()
    if tname == "Q2_K":
        hb[..., :16], hb[..., 80:84] = 1, (0x00, 0x3C, 0, 0)            # sc 1, mn 0, d 1, dmin 0
        qb[..., 16:80], qb[..., 82:84] = 0x55, 0                         # q 1, dmin 0
        zb[..., 16:80] = 0
        return deq(hb), deq(qb), -deq(zb)
    hb[..., 96:108], hb[..., 108:110] = np.tile(np.uint8([97, 24, 134]), 4), (0x00, 0x3C)   # every 6-bit scale 33, d 1: y = q - 4
    qb[..., :32], qb[..., 32:96] = 0xFF, 0x55                            # q 5: y = d * (s6 - 32)
    return deq(hb) + 4.0, deq(qb), None


@pytest.mark.parametrize("k,n", [(256, 7), (1024, 40), (5632, 33)])
@pytest.mark.parametrize("tname", TYPES)
def test_decode_matvec(gpu, pkg, orc, tname, k, n):
    """lgh_op_vec_mat_ex under the policy, with and without the norm prologue, against float64 dequantize(W) . x."""
    t = mr.TYPE[tname]
    raw = _raw(pkg, tname, k, n, 11 * k + n)
    w = orc.dequantize(t, raw, n * k).astype(np.float64).reshape(n, k)
    u, s, _ = _fields(orc, tname, raw, k, n)
    assert set(np.unique(u)) == set(range(8 if tname == "Q3_K" else 4))
    if tname == "Q3_K":
        d = raw.reshape(n, k // 256, 110)[..., 108:110].copy().view(np.float16).astype(np.float64)
        assert set(np.rint(s.reshape(n, k // 256, 256)[..., ::16] / d).ravel()) == set(range(-32, 32))
    nw = (1 + 0.2 * np.random.default_rng(k).standard_normal(k)).astype(np.float32)
    for ai, kind in enumerate(mr.ACT_KINDS):
        x = mr.activation(kind, k, 100 * ai + n)
        for norm in (None, nw):
            v = x.astype(np.float64) if norm is None else (x * norm).astype(np.float64) * mr.inv_rms(x, EPS)
            got, dev_bytes = gpu.op_vec_mat_ex(t, raw, x, n, gpu.WEIGHTS_LOWBIT_TILES, norm_w=norm, eps=EPS)
            want, bound = w @ v, 1e-4 * (np.abs(w) @ np.abs(v)) + 1e-6
            err = np.abs(got - want)
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
    raw = _raw(pkg, tname, k, n, 77 + m)
    u, s, o = _fields(orc, tname, raw, k, n)
    S = pr.f16(s * pr.SCALE)
    O = pr.f16(-o * pr.SCALE) if tname == "Q2_K" else pr.f16(S * -4.0)
    wq = pr.w_operand(tname, u, S, O)
    W, wsub = wq / pr.SCALE, pr.w_sub_term(u, S, O, wq)
    X = pr.act_block(k, m, 3 * k + m)
    Xq = pr.x_operand(X)
    assert pr.domain(W, 0.0, X, S, O)
    splits = pr.pf_plan([n], k)[1]
    want, bound = pr.gemm(W, Xq, splits), pr.gemm_bound(W, wsub, Xq, splits)
    # the operands are the format's: W' against the oracle's dequantized weights within the f16 roundings of S, O and the fma
    w = orc.dequantize(mr.TYPE[tname], raw, n * k).astype(np.float64).reshape(n, k)
    assert np.all(np.abs(W - w) <= 3 * pr.UH * (np.abs(u * s) + np.abs(w) + (0 if o is None else np.abs(o))) + 2.0 ** -24)
    got = gpu.op_mat_mat_ex(mr.TYPE[tname], raw, X, n, gpu.WEIGHTS_LOWBIT_TILES)
    err = np.abs(got - want)
    print("%s m=%d: worst err / bound %.3g" % (tname, m, float((err / bound).max())))
    assert np.all(err <= bound), float((err / bound).max())
    with pytest.raises(pkg.BackendError) as ei:   # without the policy the type has no tile layout, as ever
        gpu.op_mat_mat_ex(mr.TYPE[tname], raw, X, n, 0)
    assert ei.value.variant == "Unsupported"


def _within(got, want):
    return float(np.abs(got - want).max()) <= 2e-3 * float(np.abs(want).max()) + 2e-3


@pytest.mark.parametrize("mix", ("Q3_K", "Q2_K", "Q3_K_M"))
def test_engine(gpu, pkg, orc, mix):
    """2 layers, hidden 512, max_seq 40: batched prompt + decode against the oracle, native weight bytes, multi-sequence steps
    bit-identical to the single-sequence engine, and the f32 matrix-core policy inside the oracle's bound."""
    cfg = pkg.make_config("test-dense", max_seq_len=40)
    model = pkg.SynthModel(cfg, mix=mix)
    ref = orc.Model(cfg.as_dict())
    for name, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(name, t, ne, data)
    ref.finalize()
    make = lambda: pkg.HipGpuInference.from_model(model, 40, attn_direct=255, weight_policy=gpu.WEIGHTS_LOWBIT_TILES)
    eng, single = make(), make()
    assert eng.stats()["weight_bytes"] == model.weight_bytes()
    assert eng.prefill_is_batched()
    toks = [int(t) for t in np.random.default_rng(7).integers(0, cfg.vocab_size, size=24)]
    eng.forward_batch(toks[:20])                 # lgh_prefill_batch: the batched pass (an Unsupported status would raise)
    assert eng.position() == 20
    for i in range(20, 24):                      # (the oracle keeps its context: the prompt rides along with the first token)
        assert _within(eng.forward(toks[i]), ref.forward(toks[:21] if i == 20 else [toks[i]])), i
    # ---- multi-sequence steps: 3 and 5 sequences, each bit-identical to the single-sequence context built the same way
    eng.batch_create(5)
    hist = [[int(t) for t in np.random.default_rng(50 + s).integers(0, cfg.vocab_size, size=3)] for s in range(5)]
    want, want_ref = [], []
    for h in hist:
        single.reset()
        ref.reset()
        want.append([single.forward(t).copy() for t in h])
        want_ref.append([ref.forward([t]) for t in h])
    for B in (3, 5):
        for s in range(B):
            eng.batch_reset(s)
        for step in range(3):
            logits, _ = eng.forward_multi(list(range(B)), [hist[s][step] for s in range(B)])
            for s in range(B):
                assert np.array_equal(logits[s].view(np.uint32), want[s][step].view(np.uint32)), (B, s, step)
    # ---- the same steps on the f32 matrix cores: inside the oracle's bound, and the kernel ran
    eng.set_batch_policy(gpu.BATCH_F32_MATRIX | 2 << 8)
    before = gpu.mvqf_launches()
    for s in range(3):
        eng.batch_reset(s)
    for step in range(3):
        logits, _ = eng.forward_multi([0, 1, 2], [hist[s][step] for s in range(3)])
        for s in range(3):
            assert _within(logits[s], want_ref[s][step]), (s, step)
    assert gpu.mvqf_launches() > before


def test_weight_policy_call(gpu, pkg):
    """Unknown bits and a call after the first upload are refused and change nothing: the context keeps the f32 expansion."""
    cfg = pkg.make_config("test-dense", max_seq_len=8)
    model = pkg.SynthModel(cfg, mix="Q2_K")
    with pytest.raises(pkg.BackendError) as ei:
        pkg.HipGpuInference.from_model(model, 8, weight_policy=2)
    assert ei.value.variant == "InvalidArgument"
    eng = pkg.HipGpuInference.from_model(model, 8)
    with pytest.raises(pkg.BackendError) as ei:
        eng.set_weight_policy(gpu.WEIGHTS_LOWBIT_TILES)
    assert ei.value.variant == "InvalidArgument"
    f32_bytes = sum(s.n_elems * 4 if len(s.ne) == 2 and s.name != "token_embd.weight" else s.nbytes for s in model.specs())
    assert eng.stats()["weight_bytes"] == f32_bytes and not eng.prefill_is_batched()
