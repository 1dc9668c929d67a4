"""IQ4_NL and IQ4_XS weights kept quantized in HBM (LGH_WEIGHTS_IQ4_TILES): the decode mat-vec (|delta| <= 1e-4 sum|x_i w_i| + 1e-6), the
prompt GEMM (prefill_ref's f32 bound over the kernel's own f16 operands) and the engine (2e-3 max|logit| + 2e-3) against float64
references over the NumPy dequantizer of test_iq4_synth.py; the default (f32 expansion) against matvec_ref's f32-family bound."""
import numpy as np
import pytest

import matvec_ref as mr
import prefill_ref as pr
from test_iq4_synth import KV, dequant

pytestmark = pytest.mark.gpu
TYPES = ("IQ4_NL", "IQ4_XS")
ROW_BYTES, EPS = {"IQ4_NL": 144, "IQ4_XS": 136}, 1e-5   # tile bytes / 16 per 256 elements


def _inputs(pkg, tname, k, n, seed):
    """(raw, q, s): the generator's bytes — for IQ4_XS with the scale fields redrawn so that ls runs through 32 (a zero scale), 33 ..
    63, 0 .. 31: all 64 values where the matrix has 64 sub-blocks, both signs always — and the dequantizer's codes and scales."""
    raw = pkg.synth.fill_tensor("blk.0.ffn_up.weight", pkg.synth.TYPE_IDS[tname], n * k, k, 0, seed)
    if tname == "IQ4_XS":
        b = raw.reshape(n * k // 256, 136)
        ls = np.random.default_rng(seed).permutation((32 + np.arange(n * k // 32)) % 64).reshape(-1, 8)
        b[:, 4:8] = (ls[:, 0::2] & 15) | (ls[:, 1::2] & 15) << 4
        b[:, 2:4] = ((ls >> 4) << (2 * np.arange(8))).sum(axis=1).astype(np.uint16)[:, None].view(np.uint8)
    q, s = dequant(tname, raw, n, k)
    assert set(np.unique(q)) == set(range(16))
    if tname == "IQ4_XS":
        d = np.ascontiguousarray(raw.reshape(-1, 136)[:, :2]).view(np.float16).astype(np.float64)
        got_ls = set(np.unique(np.rint(s.reshape(-1, 256) / d + 32).astype(int)))
        assert got_ls == set((32 + np.arange(min(64, n * k // 32))) % 64) and (s > 0).any() and (s < 0).any() and (s == 0).any()
    return raw, q, s


@pytest.mark.parametrize("k,n", [(256, 7), (1024, 40), (5632, 33)])
@pytest.mark.parametrize("tname", TYPES)
def test_decode_matvec(gpu, pkg, tname, k, n):
    """lgh_op_vec_mat_ex under the policy, with and without the norm prologue, against float64 W . x; without it the f32 expansion."""
    t, (raw, q, s) = pkg.synth.TYPE_IDS[tname], _inputs(pkg, tname, k, n, 11 * k + n)
    w = s * KV[q]
    nw = (1 + 0.2 * np.random.default_rng(k).standard_normal(k)).astype(np.float32)
    for ai, kind in enumerate(mr.ACT_KINDS):
        x = mr.activation(kind, k, 100 * ai + n)
        for norm in (None, nw):
            v = x.astype(np.float64) if norm is None else (x * norm).astype(np.float64) * mr.inv_rms(x, EPS)
            got, dev_bytes = gpu.op_vec_mat_ex(t, raw, x, n, gpu.WEIGHTS_IQ4_TILES, norm_w=norm, eps=EPS)
            err, bound = np.abs(got - w @ v), 1e-4 * (np.abs(w) @ np.abs(v)) + 1e-6
            print("%s k=%d n=%d %s norm=%s: worst err / bound %.3g" % (tname, k, n, kind, norm is not None, float((err / bound).max())))
            assert np.all(err <= bound), (kind, norm is not None, float((err / bound).max()))
            assert dev_bytes == (n + 15) // 16 * 16 * (k // 256) * ROW_BYTES[tname]
    # without the policy: the f32-expanded matrix, the bits of the plain entry points, within the f32 mat-vec's bound of float64
    x = mr.activation("normal", k, 5)
    for norm, plain in ((None, gpu.op_vec_mat(t, raw, x, n)), (nw, gpu.op_norm_vec_mat(t, raw, x, nw, EPS, n))):
        got, dev_bytes = gpu.op_vec_mat_ex(t, raw, x, n, 0, norm_w=norm, eps=EPS)
        assert dev_bytes == 4 * n * k and np.array_equal(got.view(np.uint32), plain.view(np.uint32))
        y, err = mr.matvec(w, np.zeros_like(w), x, norm, EPS, family="f32")
        assert np.all(np.abs(got - y) <= err), float((np.abs(got - y) / err).max())


@pytest.mark.parametrize("m", (1, 17, 128))
@pytest.mark.parametrize("tname", TYPES)
def test_prompt_gemm(gpu, pkg, tname, m):
    """lgh_op_mat_mat_ex at k = 512, n = 48 against the float64 product of the kernel's f16 operands f16(kv * S), S = f16(256 s)."""
    k, n = 512, 48
    raw, q, s = _inputs(pkg, tname, k, n, 77 + m)
    u, S, O, X = KV[q], pr.f16(s * pr.SCALE), np.zeros((n, k)), pr.act_block(k, m, 3 * k + m)
    wq = pr.w_operand(tname, u, S, O)
    W, wsub = wq / pr.SCALE, pr.w_sub_term(u, S, O, wq)
    assert pr.domain(W, 0.0, X, S, O)
    assert np.all(np.abs(W - s * u) <= 2 * pr.UH * np.abs(s * u) + 2.0 ** -24)   # the operands are the format's, within the roundings of S and the product
    splits, Xq = pr.pf_plan([n], k)[1], pr.x_operand(X)
    want, bound = pr.gemm(W, Xq, splits), pr.gemm_bound(W, wsub, Xq, splits)
    err = np.abs(gpu.op_mat_mat_ex(pkg.synth.TYPE_IDS[tname], raw, X, n, gpu.WEIGHTS_IQ4_TILES) - want)
    print("%s m=%d: worst err / bound %.3g" % (tname, m, float((err / bound).max())))
    assert np.all(err <= bound), float((err / bound).max())
    with pytest.raises(pkg.BackendError) as ei:   # without the policy the type has no tile layout
        gpu.op_mat_mat_ex(pkg.synth.TYPE_IDS[tname], raw, X, n, 0)
    assert ei.value.variant == "Unsupported"


@pytest.mark.parametrize("mix", TYPES)
def test_engine(gpu, pkg, orc, mix):
    """Batched prompt + decode against the oracle over the f32-dequantized tensors (exact: 18 / 24 significant bits), without the f32
    mat-vec; multi-sequence steps bit-identical; the f32 matrix-core policy."""
    _within = lambda got, want: float(np.abs(got - want).max()) <= 2e-3 * float(np.abs(want).max()) + 2e-3
    cfg = pkg.make_config("test-dense", max_seq_len=40)
    model, ref = pkg.SynthModel(cfg, mix=mix), orc.Model(cfg.as_dict())
    for name, t, ne, data in model.tensors(keep=True):
        if t == pkg.synth.TYPE_IDS[mix]:
            q, s = dequant(mix, data, int(np.prod(ne)) // ne[0], ne[0])
            t, data = 0, (s * KV[q]).astype(np.float32).reshape(-1).view(np.uint8)
        ref.add_tensor(name, t, ne, data)
    ref.finalize()
    make = lambda: pkg.HipGpuInference.from_model(model, 40, attn_direct=255, weight_policy=gpu.WEIGHTS_IQ4_TILES)
    eng, single = make(), make()
    assert eng.stats()["weight_bytes"] == model.weight_bytes() and eng.prefill_is_batched()
    toks = [int(t) for t in np.random.default_rng(7).integers(0, cfg.vocab_size, size=24)]
    eng.forward_batch(toks[:20])                 # lgh_prefill_batch: the batched pass (an Unsupported status would raise)
    eng.set_profiling(True)
    for i in range(20, 24):                      # (the oracle keeps its context: the prompt rides along with the first token)
        assert _within(eng.forward(toks[i]), ref.forward(toks[:21] if i == 20 else [toks[i]])), i
    sym = eng.stats()["symbols"]
    eng.set_profiling(False)
    assert "lgh::f32_matvec_kernel" not in sym and sym["lgh::mvq_iq4_kernel<1024u>"]["launches"] > 0, sym
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
    """16, 17 and 29 are accepted before the first upload; 16 after it is refused and changes nothing (the f32 expansion)."""
    model = pkg.SynthModel(pkg.make_config("test-dense", max_seq_len=8), mix="IQ4_XS")
    for word in (16, 17, 29):
        eng = pkg.HipGpuInference.from_model(model, 8, weight_policy=word)
        assert eng.stats()["weight_bytes"] == model.weight_bytes() and eng.prefill_is_batched()
    eng = pkg.HipGpuInference.from_model(model, 8)
    with pytest.raises(pkg.BackendError) as ei:
        eng.set_weight_policy(gpu.WEIGHTS_IQ4_TILES)
    assert ei.value.variant == "InvalidArgument"
    f32_bytes = sum(s.n_elems * 4 if len(s.ne) == 2 and s.name != "token_embd.weight" else s.nbytes for s in model.specs())
    assert eng.stats()["weight_bytes"] == f32_bytes and not eng.prefill_is_batched()
