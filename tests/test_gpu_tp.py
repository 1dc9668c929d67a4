"""Tensor-parallel decode on the MI355X (lgh_tp_*, csrc/tensor_parallel.hip), all ranks on one device unless a test says otherwise.

The synchronisation-point kernel on its own (lgh_op_tp_reduce): `out` is bit for bit the f32 restatement of
resid + (((p0 + p1) + p2) ...); its XQ image and sums of squares are held to float64 of `out` the way the mat-vec epilogues'
are (matvec_multi_ref.image_ref); bytes it does not own keep a canary; two runs give the same bits.

The engine: logits against the oracle's forward on the UNSHARDED model within the decode tolerance 2e-3 * max|logit| + 2e-3
 — tensor parallelism only regroups the f32 sums of wo and down —, greedy tokens identical wherever the oracle's
top-1 / top-2 gap exceeds 4x the measured error, and the exact properties of the single context (graph replay == eager launches,
device greedy loop == host arg-max loop, reset / kv_truncate reproduce, errors leave the position alone)."""
import numpy as np
import pytest

import matvec_multi_ref as mm
import tp_ref
from test_gpu_matvec import Worst

pytestmark = pytest.mark.gpu

FILL = 0x5A


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


# ---- tp_reduce_kernel
# 4112 = 257 chunks of 16: the last workgroup holds one chunk, the last record 16 elements
@pytest.mark.parametrize("H", [256, 512, 4096, 4112])
def test_reduce_kernel_sum_order_image_and_canaries(gpu, H):
    W = Worst()
    rng = np.random.default_rng(H)
    nw_full = (1 + 0.2 * rng.standard_normal(H)).astype(np.float32)
    for n in (1, 2, 3, 8):
        for kind in ("gauss", "orders"):
            P = tp_ref.partials(kind, n, H, 100 * n + H)
            for resid in (None, (3 * rng.standard_normal(H)).astype(np.float32)):
                for nw in (None, nw_full):
                    what = "H=%d n=%d %s resid=%s nw=%s" % (H, n, kind, resid is not None, nw is not None)
                    want = tp_ref.ordered_sum(P, resid)
                    plain = gpu.op_tp_reduce(P, resid, nw, fill=FILL)
                    W.expect(np.array_equal(_bits(plain["out"]), _bits(want)), what + ": out differs from the rank-order f32 sum")
                    r = gpu.op_tp_reduce(P, resid, nw, image=True, ssq=nw is not None, fill=FILL)
                    r2 = gpu.op_tp_reduce(P, resid, nw, image=True, ssq=nw is not None, fill=FILL)
                    W.expect(np.array_equal(_bits(r["out"]), _bits(want)), what + ": out (with image) differs from the rank-order f32 sum")
                    x, xs = mm.xq_decode(r["image"], H)
                    (v, ev), (sums, es), (sq, eq) = mm.image_ref(r["out"], nw)
                    W.check("image", x, v, ev, what + " elements")
                    W.check("image", xs, sums, es, what + " chunk sums")
                    if nw is not None:
                        W.check("ssq", r["ssq"], sq, eq, what + " sums of squares")
                    # what the kernel does not own: the last 128 bytes of every record, and records' chunks past H
                    rec = r["image"].reshape(-1, 1280)
                    W.expect(np.all(rec[:, 1152:] == FILL), what + ": record tails changed")
                    if H % 256:
                        used = (H % 256) // 16
                        limb = rec[-1, :1024].reshape(8, 4, 2, 16)   # [g][digit][chunk j & 1][element]: chunk j = 2 g + (j & 1)
                        W.expect(np.all(limb.transpose(0, 2, 1, 3).reshape(16, -1)[used:] == FILL), what + ": limbs of chunks past H changed")
                        slot = np.array([(j & 3) * 4 + (j >> 2) for j in range(used, 16)])   # chunk j's sum and scale sit at this slot
                        W.expect(np.all(rec[-1, 1024:1152].reshape(2, 16, 4)[:, slot] == FILL), what + ": sums / scales of chunks past H changed")
                    for key in ("out", "image", "ssq"):
                        a, b = r[key], r2[key]
                        W.expect((a is None and b is None) or np.array_equal(_bits(a), _bits(b)), what + ": %s differs between two runs" % key)
    W.done()


def test_reduce_kernel_refuses_bad_shapes(gpu, pkg):
    for P in (np.zeros((9, 256), np.float32), np.zeros((2, 264), np.float32)):   # more than 8 ranks; H not a multiple of 16
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_tp_reduce(P)
        assert ei.value.variant == "InvalidArgument"


# ---- the engine
def _tol(want):
    return 2e-3 * float(np.abs(want).max()) + 2e-3


def _check_against_oracle(pkg, orc, tp, cfg, prompt, fed, logits, what):
    """Prompt through GpuModelWrapper (prefill_token x (n - 1) + forward), then the oracle's tokens one by one."""
    wrap, ctx = pkg.GpuModelWrapper(tp), pkg.InferenceContext()
    got = wrap.forward(prompt, ctx)
    assert tp.position() == len(prompt)
    errs, gaps = [], []
    for i, want in enumerate(logits):
        err = float(np.abs(got - want).max())
        print("%s step %d: max|dlogit| %.3e tol %.3e" % (what, i, err, _tol(want)))
        assert np.all(np.isfinite(got)) and err <= _tol(want), (what, i, err, _tol(want))
        srt = np.sort(want)
        gaps.append(float(srt[-1] - srt[-2]))
        errs.append(err)
        if gaps[-1] > 4 * err:
            assert orc.argmax_last(got) == orc.argmax_last(want), "%s step %d: greedy token diverged with gap %.3e vs err %.3e" % (what, i, gaps[-1], err)
        if i < len(fed):
            got = wrap.forward([fed[i]], ctx)
    assert tp.position() == len(prompt) + len(fed)
    print("%s: max|dlogit|=%.3e tol=%.3e min_gap=%.3e" % (what, max(errs), _tol(logits[-1]), min(gaps)))


D128 = dict(intermediate_size=2048, num_kv_heads=4)
ENGINE_CASES = [("test-dense", "Q4_K_M", {}, 2), ("test-dense", "Q8_0", dict(num_heads=16, num_kv_heads=4), 4),
                ("test-dense-d128", "Q4_K_M", D128, 2), ("test-dense-d128", "Q4_K_M", D128, 4), ("test-dense", "Q4_K_M", {}, 1),
                # ffn_down shards of k = 1792 (7 k-slices, 448-thread workgroups) and k = 1280 (5 k-slices, 320 threads)
                ("test-dense-d128", "Q4_K_M", dict(num_kv_heads=4, intermediate_size=3584, num_layers=2), 2),
                ("test-dense-d128", "Q4_K_M", dict(num_kv_heads=4, intermediate_size=5120, num_layers=2), 4)]


@pytest.mark.parametrize("name,mix,over,n", ENGINE_CASES)
def test_logits_and_greedy_tokens_match_oracle(gpu, pkg, orc, name, mix, over, n):
    cfg, model, prompt, fed, logits = tp_ref.oracle_logits(pkg, orc, name, mix, over, 20, 6, 64)
    tp = pkg.HipTensorParallel.from_model(model, 64, n)
    try:
        assert tp.ranks() == n
        _check_against_oracle(pkg, orc, tp, cfg, prompt, fed, logits, "%s/%s %s N=%d" % (name, mix, over, n))
        assert tp.graph_nodes() > 0
    finally:
        tp.close()


@pytest.mark.parametrize("mix,over,with_bias,n", [("Q8_0", dict(tie_embeddings=True), False, 2), ("Q4_K_M", {}, True, 2)])
def test_tied_output_and_biases(gpu, pkg, orc, mix, over, with_bias, n):
    """The tied output projection is sharded from token_embd's rows at finalize; attn_q / attn_k / attn_v biases go with their heads."""
    cfg, model, prompt, fed, logits = tp_ref.oracle_logits(pkg, orc, "test-dense", mix, over, 6, 3, 32, with_bias=with_bias)
    tp = pkg.HipTensorParallel.from_model(model, 32, n)
    try:
        _check_against_oracle(pkg, orc, tp, cfg, prompt, fed, logits, "test-dense/%s %s bias=%s N=%d" % (mix, over, with_bias, n))
    finally:
        tp.close()


def test_long_context_takes_the_split_attention(gpu, pkg, orc):
    """Past the ranks' default threshold of 256 rows (engine.hip: kDirectAttnDefaultKv) they run the attention splits + merge; up to
    it, the single-launch attention is all that runs.  A prompt of 260 tokens in a cache of 288: the prompt's last four steps and the
    four decode steps attend 257 .. 264 rows.  The witness that both forms ran: a twin whose ranks never take the single launch
    (flags = 255 << 16), fed the same way, gives other bits at a step attending 200 rows — one form sums in another tree than the
    other — while a twin with the default threshold spelled out (4 << 16) gives the same."""
    cfg, model, prompt, fed, logits = tp_ref.oracle_logits(pkg, orc, "test-dense", "Q4_K_M", {}, 260, 4, 288)
    tp = pkg.HipTensorParallel.from_model(model, 288, 2)
    never = pkg.HipTensorParallel.from_model(model, 288, 2, flags=255 << 16)
    same = pkg.HipTensorParallel.from_model(model, 288, 2, flags=4 << 16)
    try:
        _check_against_oracle(pkg, orc, tp, cfg, prompt, fed, logits, "test-dense/Q4_K_M prompt 260 N=2")
        tp.reset()
        got = [pkg.GpuModelWrapper(e).forward(prompt[:200], pkg.InferenceContext()) for e in (tp, never, same)]
        assert tp.position() == never.position() == same.position() == 200
        assert np.array_equal(_bits(got[0]), _bits(got[2]))
        assert not np.array_equal(_bits(got[0]), _bits(got[1])), "the default ranks and ranks that never take the single launch agree at 200 rows"
        assert float(np.abs(got[0] - got[1]).max()) <= 1e-4 * float(np.abs(got[0]).max())   # another summation tree, not another context
        # ... and past 256 rows the default ranks still follow the never-switching ones within that: both run splits + merge there
        for e in (tp, never):
            for t in prompt[200:259]:
                e.prefill_token(t)
        a, b = tp.forward(prompt[259]), never.forward(prompt[259])
        assert float(np.abs(a - b).max()) <= 1e-4 * float(np.abs(a).max())
        assert float(np.abs(a - logits[0]).max()) <= _tol(logits[0]) and float(np.abs(b - logits[0]).max()) <= _tol(logits[0])
    finally:
        tp.close()
        never.close()
        same.close()


def test_distinct_devices(gpu, pkg, orc):
    if gpu.device_count() < 2:
        pytest.skip("needs two HIP devices")
    cfg, model, prompt, fed, logits = tp_ref.oracle_logits(pkg, orc, "test-dense", "Q4_K_M", {}, 20, 6, 64)
    tp = pkg.HipTensorParallel.from_model(model, 64, 2, devices=[0, 1])
    try:
        _check_against_oracle(pkg, orc, tp, cfg, prompt, fed, logits, "test-dense/Q4_K_M devices [0, 1]")
    finally:
        tp.close()


def test_exact_properties(gpu, pkg, orc):
    cfg, model, prompt, fed, _ = tp_ref.oracle_logits(pkg, orc, "test-dense", "Q4_K_M", {}, 20, 6, 64)
    toks = prompt[:9]
    tp = pkg.HipTensorParallel.from_model(model, 64, 2)
    eager = pkg.HipTensorParallel.from_model(model, 64, 2, flags=gpu.FLAG_NO_GRAPH)
    try:
        def run(e, tokens):
            for t in tokens[:-1]:
                e.prefill_token(t)
            return e.forward(tokens[-1])

        # graph replay == eager launches, and the same history twice gives the same bits
        a = [run(tp, toks)] + [tp.forward(t) for t in (5, 900, 31)]
        b = [run(eager, toks)] + [eager.forward(t) for t in (5, 900, 31)]
        assert tp.graph_nodes() > 0 and eager.graph_nodes() == 0
        assert tp.position() == eager.position() == len(toks) + 3
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))
        tp.reset()
        assert tp.position() == 0
        a2 = [run(tp, toks)] + [tp.forward(t) for t in (5, 900, 31)]
        for x, y in zip(a, a2):
            assert np.array_equal(_bits(x), _bits(y))
        # kv_truncate(k), then the same tokens: the earlier logits
        tp.kv_truncate(len(toks))
        assert tp.position() == len(toks)
        assert np.array_equal(_bits(tp.forward(5)), _bits(a[1])) and np.array_equal(_bits(tp.forward(900)), _bits(a[2]))
        with pytest.raises(pkg.BackendError) as ei:
            tp.kv_truncate(tp.position() + 1)
        assert ei.value.variant == "InvalidArgument"
        # the device greedy loop (token fed back on the device into every rank) == the host arg-max loop over forward
        tp.kv_truncate(len(toks))
        dev = tp.decode_greedy(3, 16).tolist()
        assert tp.position() == len(toks) + 16
        tp.kv_truncate(len(toks))
        host, tok = [], 3
        for _ in range(16):
            tok = orc.argmax_last(tp.forward(tok))
            host.append(tok)
        assert dev == host
        eager.kv_truncate(len(toks))
        assert eager.decode_greedy(3, 16).tolist() == host
        # errors leave the position alone
        pos = tp.position()
        with pytest.raises(pkg.BackendError) as ei:
            tp.forward(cfg.vocab_size)
        assert ei.value.variant == "InvalidArgument" and tp.position() == pos
        with pytest.raises(pkg.BackendError) as ei:
            tp.prefill_token(cfg.vocab_size + 7)
        assert ei.value.variant == "InvalidArgument" and tp.position() == pos
        tp.reset()
        tp.decode_greedy(1, 64)
        assert tp.position() == 64
        for call in (lambda: tp.forward(1), lambda: tp.prefill_token(1), lambda: tp.decode_greedy(1, 1)):
            with pytest.raises(pkg.BackendError) as ei:
                call()
            assert ei.value.variant == "InvalidArgument" and tp.position() == 64
        # GpuModelWrapper's reset rule (mod.rs:334-336) on the handle
        wrap = pkg.GpuModelWrapper(tp)
        x = wrap.forward(toks, pkg.InferenceContext())
        assert tp.position() == len(toks) and np.array_equal(_bits(x), _bits(a[0]))
    finally:
        tp.close()
        eager.close()


def test_refusals_name_the_reason(gpu, pkg):
    TP, BE = pkg.HipTensorParallel, pkg.BackendError

    def refused(variant, words, name, mix, n, over=None, **kw):
        model = pkg.SynthModel(pkg.make_config(name, max_seq_len=32, **(over or {})), mix=mix)
        with pytest.raises(BE) as ei:
            TP.from_model(model, 32, n, **kw).close()
        assert ei.value.variant == variant, str(ei.value)
        for w in words:
            assert w in str(ei.value), str(ei.value)

    refused("InvalidArgument", ["num_heads (8) must be divisible by world_size (3)"], "test-dense", "Q4_K_M", 3)
    refused("InvalidArgument", ["num_kv_heads (2) must be divisible by world_size (4)"], "test-dense", "Q4_K_M", 4)
    refused("InvalidArgument", ["ffn_dim (1000) must be divisible by world_size (3)"], "test-dense", "Q4_K_M", 3,
            dict(num_heads=12, num_kv_heads=3, intermediate_size=1000))
    refused("InvalidArgument", ["world_size (9)"], "test-dense", "Q4_K_M", 9)
    refused("InvalidArgument", ["world_size (0)"], "test-dense", "Q4_K_M", 0)
    refused("Unsupported", ["MoE"], "test-moe", "Q4_K_M", 2)
    refused("Unsupported", ["1408", "256"], "test-dense-d128", "Q4_K_M", 2)            # 2816 / 2 is not a multiple of 256
    refused("Unsupported", ["128", "256"], "test-dense", "Q4_K_M", 4, dict(num_kv_heads=4))   # 2 heads x 64 per rank
    refused("Unsupported", ["kv_cache_type"], "test-dense", "Q4_K_M", 2, kv_cache_type=gpu.KV_INT8)
    refused("Unsupported", ["f32 KV cache"], "test-dense", "Q4_K_M", 2, flags=gpu.FLAG_KV_INT8)
    refused("InvalidArgument", ["layer_begin"], "test-dense", "Q4_K_M", 2, layer_range=(0, 1))
    refused("InvalidArgument", ["layer_begin"], "test-dense", "Q4_K_M", 2, layer_range=(1, 2))
    refused("Unsupported", ["tile layouts"], "test-dense", "Q5_0", 2)                  # a 2-D weight the engine expands to f32
