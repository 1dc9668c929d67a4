"""The tensor-parallel prompt pass on the MI355X (lgh_tp_prefill_batch, csrc/tp_prefill.hip + the driver in csrc/tensor_parallel.hip),
all ranks on one device unless a test says otherwise.

Per launch (lgh_op_tp_pf_reduce): hidden is bit for bit the f32 restatement of tests/tp_prefill_ref.py (splits in order from a zero
start, bias on rank 0, ranks in rank order, residual last); the XH image is bit for bit f16(f32(hidden * nw)) of the RETURNED
hidden, with every byte the m tokens do not own still the canary; the sums of squares are held to float64 of the returned hidden
with the row-epilogue test's bound (prefill_ref.ssq_ref); rows t >= m and chunks past the row's keep the canary; two runs give the
same bits; and with one rank the two launches equal pf_row_epi_launch (path 1) in all three outputs.

Every (H, n) case walks all 12 (m, S, data kind) triples; the 8 (col0, bias, nw) combinations rotate over them, so each appears
with every H and n and at least once with every m, S and kind.

The engine: logits against the oracle on the UNSHARDED model within the batched path's own tolerance (tests/test_gpu_prefill.py:
1e-2 * max|logit| + 1e-2), greedy tokens identical wherever the oracle's top-1 / top-2 gap exceeds 4x the measured error, and the
exact properties of the single context's prompt pass.  Each parity case prints `RATIO <case>: err / tol`.

Measured on the MI355X (worst err / tol over the prompt's last token and 4 greedy steps, prompts of 70 / 150 tokens): test-dense
Q4_K_M N = 1 and N = 2 0.168 / 0.130, Q8_0 N = 4 0.065 / 0.063, test-dense-d128 N = 2 0.175 / 0.154, N = 4 0.174 / 0.154
(profiles/tp_prefill.md)."""
import itertools

import numpy as np
import pytest

import prefill_ref as pr
import tp_prefill_ref as tpr
import tp_ref
from test_gpu_matvec import Worst
from test_gpu_tp import ENGINE_CASES

pytestmark = pytest.mark.gpu

FILL = 0x5A
EXTRA = 72           # ncols = H + EXTRA > col0 + H for col0 in (0, 64)
TRIPLES = list(itertools.product((1, 17, 128), (1, 3), ("gauss", "orders")))
COMBOS = list(itertools.product((0, 64), (False, True), (False, True)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def _is_fill(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))


@pytest.fixture(scope="module")
def data():
    memo = {}

    def get(kind, n, H):
        if (kind, n, H) not in memo:
            rng = np.random.default_rng(1000 * n + H)
            P = tpr.split_partials(kind, n, 3, H + EXTRA, 100 * n + H + (kind == "orders"))
            P.setflags(write=False)
            memo[kind, n, H] = (P, (3 * rng.standard_normal((128, H))).astype(np.float32), rng.standard_normal(H).astype(np.float32),
                                (1 + 0.2 * rng.standard_normal(H)).astype(np.float32))
        return memo[kind, n, H]
    return get


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("H", [256, 2048, 2304])      # 2304: two chunks of sums of squares, the second one partial
def test_partial_and_reduce_launches(gpu, data, H, n):
    W = Worst()
    chunks = -(-H // pr.SSQ_COLS)
    for idx, (m, S, kind) in enumerate(TRIPLES):
        col0, with_bias, with_nw = COMBOS[(idx + n + H // 256) % len(COMBOS)]
        P3, resid_full, bias_full, nw_full = data(kind, n, H)
        P = np.ascontiguousarray(P3[:, :S])
        resid, bias, nw = resid_full[:m], bias_full if with_bias else None, nw_full if with_nw else None
        what = "H=%d n=%d m=%d S=%d %s col0=%d bias=%d nw=%d" % (H, n, m, S, kind, col0, with_bias, with_nw)
        want = tpr.hidden_ref(P, col0, resid, bias)
        r = gpu.op_tp_pf_reduce(P, resid, col0=col0, bias=bias, norm_w=nw, fill=FILL)
        hid = r["hidden"]
        W.expect(np.array_equal(_bits(hid[:m]), _bits(want)), what + ": hidden differs from the f32 restatement at %d elements" %
                 int((_bits(hid[:m]) != _bits(want)).sum()))
        W.expect(_is_fill(hid[m:]), what + ": hidden rows t >= m changed")
        bad = int((r["xh"] != tpr.xh_image(hid[:m], nw, FILL)).sum())
        W.expect(bad == 0, what + ": XH is not f16(f32(hidden * nw)) of the returned hidden, or bytes outside the block changed (%d bytes)" % bad)
        s, es = pr.ssq_ref(hid[:m])
        W.check("ssq", r["ssq"][:m, :chunks], s, es, what)
        W.expect(_is_fill(r["ssq"][m:]) and _is_fill(r["ssq"][:m, chunks:]), what + ": sums of squares written outside the block's chunks")
        r2 = gpu.op_tp_pf_reduce(P, resid, col0=col0, bias=bias, norm_w=nw, fill=FILL)
        W.expect(all(np.array_equal(_bits(r[k]), _bits(r2[k])) for k in r), what + ": two runs differ")
        if n == 1:
            y = gpu.op_tp_pf_reduce(P, resid, col0=col0, bias=bias, norm_w=nw, path=1, fill=FILL)
            for k in ("hidden", "xh", "ssq"):
                W.expect(np.array_equal(_bits(r[k]), _bits(y[k])), what + ": %s differs from pf_row_epi_launch on the same inputs" % k)
    W.done()


def test_launch_refusals(gpu, pkg):
    P = np.zeros((1, 1, 128, 264), np.float32)
    R = np.zeros((3, 256), np.float32)
    bad = [dict(partials=np.zeros((9, 1, 128, 264), np.float32)), dict(partials=np.zeros((0, 1, 128, 264), np.float32)),
           dict(resid=np.zeros((129, 256), np.float32)), dict(resid=np.zeros((0, 256), np.float32)),
           dict(resid=np.zeros((3, 252), np.float32)),                       # H % 8
           dict(partials=np.zeros((1, 1, 128, 266), np.float32)),            # ncols % 4
           dict(col0=2), dict(col0=12),                                     # col0 % 4; col0 + H > ncols
           dict(partials=np.zeros((2, 1, 128, 264), np.float32), path=1), dict(path=2)]
    for kw in bad:
        args = dict(partials=P, resid=R)
        args.update(kw)
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_tp_pf_reduce(args.pop("partials"), args.pop("resid"), **args)
        assert ei.value.variant == "InvalidArgument", kw


# ---- the engine
MAX_SEQ = 192


def _tol(want):
    return 1e-2 * float(np.abs(want).max()) + 1e-2


def _parity(orc, tp, prompt, fed, logits, what):
    """forward_batch(prompt[:-1]) + forward(prompt[-1]), then the oracle's greedy tokens one by one; -> worst err / tol"""
    tp.forward_batch(prompt[:-1])
    assert tp.position() == len(prompt) - 1
    got = tp.forward(prompt[-1])
    worst = 0.0
    for i, want in enumerate(logits):
        err = float(np.abs(got - want).max())
        worst = max(worst, err / _tol(want))
        print("%s step %d: max|dlogit| %.3e tol %.3e" % (what, i, err, _tol(want)))
        assert np.all(np.isfinite(got)) and err <= _tol(want), (what, i, err, _tol(want))
        srt = np.sort(want)
        if float(srt[-1] - srt[-2]) > 4 * err:
            assert orc.argmax_last(got) == orc.argmax_last(want), "%s step %d: greedy token diverged" % (what, i)
        if i < len(fed):
            got = tp.forward(fed[i])
    assert tp.position() == len(prompt) + len(fed)
    print("RATIO %s: err / tol = %.3f" % (what, worst))
    return worst


@pytest.mark.parametrize("n_prompt", [70, 150])       # 150: two blocks, 128 + 21 of the pass, the second with a partial token tile
@pytest.mark.parametrize("name,mix,over,n", ENGINE_CASES)
def test_prompt_pass_matches_oracle(gpu, pkg, orc, name, mix, over, n, n_prompt):
    cfg, model, prompt, fed, logits = tp_ref.oracle_logits(pkg, orc, name, mix, over, n_prompt, 4, MAX_SEQ)
    tp = pkg.HipTensorParallel.from_model(model, MAX_SEQ, n)
    try:
        assert tp.prefill_is_batched()
        _parity(orc, tp, prompt, fed, logits, "%s/%s %s N=%d prompt %d" % (name, mix, over, n, n_prompt))
    finally:
        tp.close()


def test_exact_properties(gpu, pkg, orc):
    cfg, model, prompt, fed, logits = tp_ref.oracle_logits(pkg, orc, "test-dense", "Q4_K_M", {}, 70, 4, MAX_SEQ)
    TP = pkg.HipTensorParallel
    tp = TP.from_model(model, MAX_SEQ, 2)
    exact = TP.from_model(model, MAX_SEQ, 2, flags=gpu.FLAG_EXACT_PREFILL)
    one = TP.from_model(model, MAX_SEQ, 2, flags=gpu.FLAG_EXACT_PREFILL)
    try:
        assert tp.prefill_is_batched() and not exact.prefill_is_batched()
        # EXACT_PREFILL: forward_batch is prefill_token one by one
        exact.forward_batch(prompt[:40])
        for t in prompt[:40]:
            one.prefill_token(t)
        assert exact.position() == one.position() == 40
        assert np.array_equal(_bits(exact.forward(5)), _bits(one.forward(5)))
        # the batched pass: scratch grows at the first call, KV bytes do not; the same prompt twice gives the same bits
        before = tp.stats(1)
        tp.forward_batch(prompt[:69])
        assert tp.position() == 69
        after = tp.stats(1)
        assert after["scratch_bytes"] > before["scratch_bytes"] and after["kv_bytes"] == before["kv_bytes"]
        assert after["tokens_processed"] == before["tokens_processed"] + 69
        a = tp.forward(prompt[69])
        assert tp.position() == 70
        tp.reset()
        assert tp.position() == 0
        tp.forward_batch(prompt[:69])
        assert tp.stats(1)["scratch_bytes"] == after["scratch_bytes"]
        assert np.array_equal(_bits(tp.forward(prompt[69])), _bits(a))
        # a second block on top at a position that is no multiple of 16, then forward: within tolerance of the oracle
        cfg2, _, prompt2, _, logits2 = tp_ref.oracle_logits(pkg, orc, "test-dense", "Q4_K_M", {}, 101, 0, MAX_SEQ)
        assert prompt2[:70] == prompt and tp.position() % 16 != 0
        tp.forward_batch(prompt2[70:100])
        assert tp.position() == 100
        b = tp.forward(prompt2[100])
        err = float(np.abs(b - logits2[0]).max())
        print("RATIO second block at position 70: err / tol = %.3f" % (err / _tol(logits2[0])))
        assert err <= _tol(logits2[0])
        # kv_truncate back into the batched rows, then forward: the earlier logits
        tp.kv_truncate(69)
        assert tp.position() == 69
        assert np.array_equal(_bits(tp.forward(prompt[69])), _bits(a))
        # the device greedy loop after a batched prompt == the host arg-max loop over forward
        tp.kv_truncate(69)
        dev = tp.decode_greedy(prompt[69], 8).tolist()
        assert tp.position() == 77
        tp.kv_truncate(69)
        host, tok = [], prompt[69]
        for _ in range(8):
            tok = orc.argmax_last(tp.forward(tok))
            host.append(tok)
        assert dev == host
        # errors leave the position alone
        pos = tp.position()
        for toks in ([1, 2, cfg.vocab_size, 3], list(range(MAX_SEQ - pos + 1))):
            with pytest.raises(pkg.BackendError) as ei:
                tp.forward_batch(toks)
            assert ei.value.variant == "InvalidArgument" and tp.position() == pos
    finally:
        tp.close()
        exact.close()
        one.close()


def test_distinct_devices(gpu, pkg, orc):
    if gpu.device_count() < 2:
        pytest.skip("needs two HIP devices")
    cfg, model, prompt, fed, logits = tp_ref.oracle_logits(pkg, orc, "test-dense", "Q4_K_M", {}, 150, 4, MAX_SEQ)
    tp = pkg.HipTensorParallel.from_model(model, MAX_SEQ, 2, devices=[0, 1])
    try:
        _parity(orc, tp, prompt, fed, logits, "test-dense/Q4_K_M devices [0, 1] prompt 150")
    finally:
        tp.close()
