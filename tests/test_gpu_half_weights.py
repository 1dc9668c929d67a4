"""F16 and BF16 weights kept 16-bit in HBM (lgh_set_weight_policy: LGH_WEIGHTS_HALF_TILES): their decode mat-vec (csrc/matvec_h16.hip),
their prompt GEMM (pf_gemm_half_kernel, csrc/prefill.hip) and the engine against float64 references.

Bounds: the mat-vec's standing |delta| <= 1e-4 sum|x_i w_i| + 1e-6 against the oracle's dequantization (both conversions are exact, so
the special values hold it too); the GEMM's f32-accumulation bound of tests/prefill_ref.py over the kernel's own f16 operands, which
for these types are the weights themselves; the engine's 2e-3 max|logit| + 2e-3 against orc.Model.forward over the f32 expansion of
the same tensors — what the reference's GPU path computes with; its CPU path rejects 16-bit 2-D weights (oracle/model.cpp:95)."""
import numpy as np
import pytest

import matvec_ref as mr
import prefill_ref as pr

pytestmark = pytest.mark.gpu

TYPE = {"F16": 1, "BF16": 30}
EPS = 1e-5
# Row 0: +-0 and the large magnitudes; row 1: zeros but for the small ones.  F16: largest normal, smallest normal, subnormal.  BF16: 2^40
# and 2^-40 — both are lost if BF16 is routed through f16 — then smallest normal and subnormal.  Row 2: the type's largest normal alone,
# at column BIG_COL, where every activation is set to 2^-64: BF16's 3.4e38 times an O(1) activation would leave f32's range.
BIG = {"F16": 0x7BFF, "BF16": 0x7F7F}
BIG_COL = 5
SPECIAL = {"F16": ((0x0000, 0x8000, 0x7BFF, 0xFBFF), (0x0400, 0x8400, 0x0001, 0x8001)),
           "BF16": ((0x0000, 0x8000, 0x5380, 0xD380), (0x2B80, 0xAB80, 0x0080, 0x0001))}


def _raw(pkg, tname, k, n, seed):
    raw = pkg.synth.fill_tensor("blk.0.ffn_up.weight", TYPE[tname], n * k, k, 0, seed)
    h = raw.view(np.uint16).reshape(n, k)
    h[1:3] = 0
    h[2, BIG_COL] = BIG[tname]
    for r in (0, 1):
        h[r, 3:3 + 4 * 67:67] = SPECIAL[tname][r]   # (columns 3, 70, 137, 204: four different lane chunks of the first tile)
    return raw


@pytest.mark.parametrize("k,n", [(256, 7), (1024, 40), (5632, 33)])
@pytest.mark.parametrize("tname", ("F16", "BF16"))
def test_decode_matvec(gpu, pkg, orc, tname, k, n):
    """lgh_op_vec_mat_ex under the policy, every activation kind with and without the norm prologue, against float64 dequantize(W) . x."""
    t = TYPE[tname]
    raw = _raw(pkg, tname, k, n, 13 * k + n)
    w = orc.dequantize(t, raw, n * k).astype(np.float64).reshape(n, k)
    assert np.abs(w[0]).max() == (65504.0 if tname == "F16" else 2.0 ** 40) and 0 < np.abs(w[1]).max() < 1e-4
    assert w[2, BIG_COL] == (65504.0 if tname == "F16" else 2.0 ** 128 - 2.0 ** 120) and np.count_nonzero(w[2]) == 1
    nw = (1 + 0.2 * np.random.default_rng(k).standard_normal(k)).astype(np.float32)
    for ai, kind in enumerate(mr.ACT_KINDS):
        x = mr.activation(kind, k, 100 * ai + n)
        x[BIG_COL] = 2.0 ** -64
        for norm in (None, nw):
            v = x.astype(np.float64) if norm is None else (x * norm).astype(np.float64) * mr.inv_rms(x, EPS)
            got, dev_bytes = gpu.op_vec_mat_ex(t, raw, x, n, gpu.WEIGHTS_HALF_TILES, norm_w=norm, eps=EPS)
            want, bound = w @ v, 1e-4 * (np.abs(w) @ np.abs(v)) + 1e-6
            err = np.abs(got - want)
            print("%s k=%d n=%d %s norm=%s: worst err / bound %.3g" % (tname, k, n, kind, norm is not None, float((err / bound).max())))
            assert np.all(err <= bound), (kind, norm is not None, float((err / bound).max()))
            assert dev_bytes == (n + 15) // 16 * 16 * k * 2
    # without the policy the _ex entry is the existing entry point: the f32-expanded matrix, the same bits
    x = mr.activation("normal", k, 5)
    got, dev_bytes = gpu.op_vec_mat_ex(t, raw, x, n, 0)
    assert dev_bytes == 4 * n * k and np.array_equal(got.view(np.uint32), gpu.op_vec_mat(t, raw, x, n).view(np.uint32))
    got, _ = gpu.op_vec_mat_ex(t, raw, x, n, 0, norm_w=nw, eps=EPS)
    assert np.array_equal(got.view(np.uint32), gpu.op_norm_vec_mat(t, raw, x, nw, EPS, n).view(np.uint32))


@pytest.mark.parametrize("m", (1, 17, 128))
@pytest.mark.parametrize("tname", ("F16", "BF16"))
def test_prompt_gemm(gpu, pkg, orc, tname, m):
    """lgh_op_mat_mat_ex at k = 512, n = 48 against the float64 product of the kernel's f16 operands f16(256 w) / 256 — the weights
    themselves inside the GEMM's domain — with prefill_ref's bound (no subnormal term: no operand is one)."""
    k, n, t = 512, 48, TYPE[tname]
    raw = pkg.synth.fill_tensor("blk.0.ffn_up.weight", t, n * k, k, 0, 77 + m)
    w = orc.dequantize(t, raw, n * k).astype(np.float64).reshape(n, k)
    wq = pr.f16(w * pr.SCALE)
    W = wq / pr.SCALE
    X = pr.act_block(k, m, 3 * k + m)
    Xq = pr.x_operand(X)
    assert pr.domain(W, 0.0, X) and np.all((w == 0) | (np.abs(wq) >= pr.F16_TINY)) and np.array_equal(W, w)
    splits = pr.pf_plan([n], k)[1]
    want, bound = pr.gemm(W, Xq, splits), pr.gemm_bound(W, np.zeros_like(W), Xq, splits)
    got = gpu.op_mat_mat_ex(t, raw, X, n, gpu.WEIGHTS_HALF_TILES)
    err = np.abs(got - want)
    print("%s m=%d: worst err / bound %.3g" % (tname, m, float((err / bound).max())))
    assert np.all(err <= bound), float((err / bound).max())
    with pytest.raises(pkg.BackendError) as ei:   # without the policy the type has no tile layout, as ever
        gpu.op_mat_mat_ex(t, raw, X, n, 0)
    assert ei.value.variant == "Unsupported"


# (F16_M: the generator's `_M` recipe over F16 — Q6_K attn_v and ffn_down in layer 1 and a Q6_K output: a QKV launch whose matrices are
# of both families, split per family in the prompt GEMM as in decode)
@pytest.mark.parametrize("config,mix", [("test-dense", "F16"), ("test-dense", "BF16"), ("test-moe", "F16"), ("test-dense", "F16_M")])
def test_engine(gpu, pkg, orc, config, mix):
    """2 layers, hidden 512, max_seq 40: a 20-token batched prompt, 4 decode steps and 3 greedy steps against the oracle over the f32
    expansion; native weight bytes; every projection a launch of the new kernel and none of the f32 mat-vec."""
    cfg = pkg.make_config(config, max_seq_len=40)
    model = pkg.SynthModel(cfg, mix=mix)
    ref = orc.Model(cfg.as_dict())
    plain = mix in TYPE
    for name, t, ne, data in model.tensors(keep=True):
        if t == TYPE[mix[:-2] if not plain else mix]:
            t, data = 0, orc.dequantize(t, data, int(np.prod(ne))).astype(np.float32).view(np.uint8)
        ref.add_tensor(name, t, ne, data)
    ref.finalize()
    eng = pkg.HipGpuInference.from_model(model, 40, weight_policy=gpu.WEIGHTS_HALF_TILES)
    assert eng.stats()["weight_bytes"] == model.weight_bytes()
    assert eng.prefill_is_batched()
    toks = [int(t) for t in np.random.default_rng(7).integers(0, cfg.vocab_size, size=24)]
    eng.forward_batch(toks[:20])
    assert eng.position() == 20
    eng.set_profiling(True)
    for i in range(20, 24):                      # (the oracle keeps its context: the prompt rides along with the first token)
        got, want = eng.forward(toks[i]), ref.forward(toks[:21] if i == 20 else [toks[i]])
        assert float(np.abs(got - want).max()) <= 2e-3 * float(np.abs(want).max()) + 2e-3, i
    sym = eng.stats()["symbols"]
    eng.set_profiling(False)
    # per token and layer QKV, wo, gate|up and down (MoE: the two selected experts share each launch), then the output projection
    if plain:
        assert sym["lgh::mvh_kernel<%s>" % ("true" if mix == "BF16" else "false")]["launches"] == 4 * (cfg.num_layers * 4 + 1), sym
    assert "lgh::f32_matvec_kernel" not in sym
    # greedy steps: the output projection's arg-max parts against the arg-max of the logits the same context returns
    nxt = int(np.argmax(got))
    for _ in range(3):
        logits = eng.forward(nxt)
        eng.kv_truncate(eng.position() - 1)
        top = np.flatnonzero(logits == logits.max())[-1]
        assert eng.forward_argmax(nxt) == top
        nxt = int(top)


def test_weight_policy_word(gpu, pkg):
    """4 and 5 are accepted before the first upload, 4 is refused after it (bit 1 stays refused: test_gpu_lowbit_weights pins it)."""
    cfg = pkg.make_config("test-dense", max_seq_len=8)
    model = pkg.SynthModel(cfg, mix="F16")
    for word in (4, 5):
        eng = pkg.HipGpuInference.from_model(model, 8, weight_policy=word)
        assert eng.stats()["weight_bytes"] == model.weight_bytes()
    eng = pkg.HipGpuInference.from_model(model, 8)
    with pytest.raises(pkg.BackendError) as ei:
        eng.set_weight_policy(gpu.WEIGHTS_HALF_TILES)
    assert ei.value.variant == "InvalidArgument"
    assert eng.stats()["weight_bytes"] > model.weight_bytes()   # (the f32 expansion, as ever)
