"""The batched-prompt GEMM (csrc/prefill.hip) against the float64 restatement in tests/prefill_ref.py: the kernel's own f16 operands
are emulated exactly, so the bound is the f32 accumulation's — C_pf(k, S) 2^-24 sum |w' x'| plus the subnormal allowance —
counted from the kernel in prefill_ref's header, not fitted.  Each test prints `WORST <path>: err / bound`.

Shapes: (256, 16) one block, one tile of a 16-tile workgroup (the tile clamp); (512, 272) two row groups, the second with one
tile, two splits; (1280, 13312) and (2048, 16640) the smallest shapes whose plan holds more than one block per split — 2, 2, 1
and 3, 3, 2: the LDS double buffer, the prefetch, the re-requested last block and the short last split.

The QKV, wo and dense-FFN steps run through lgh_op_pf_qkv / _linear / _ffn: prefill_block's own launch sequences on a scratch filled
with NaN patterns, so a value consumed without having been produced shows in the output."""
import numpy as np
import pytest

import matvec_ref as mr
import prefill_ref as pr
from test_gpu_matvec import Worst

pytestmark = pytest.mark.gpu

M = 17


def _raw(pkg, orc, tname, kind, k, n, seed):
    return mr.weights(tname, kind, k, n, seed, orc=orc, synth_fill=pkg.synth.fill_tensor)


def _bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


@pytest.mark.parametrize("tname", mr.FUSED)
def test_gemm_formats(gpu, pkg, orc, tname):
    """Every weight generator x every activation kind (token t carries kind t % 6) at m = 17, and run-to-run identity."""
    W = Worst()
    t = mr.TYPE[tname]
    for k, n in [(256, 16), (512, 272)]:
        rg, S, per, last = pr.pf_plan([n], k)
        X = pr.act_block(k, M, 7 * k + n)
        Xq = pr.x_operand(X)
        for wi, kind in enumerate(mr.WEIGHT_KINDS):
            raw = _raw(pkg, orc, tname, kind, k, n, 300 + 10 * wi + k)
            y, e = pr.gemm_ref(tname, raw, k, n, Xq, S)
            got = gpu.op_mat_mat(t, raw, X, n)
            W.check("gemm %s %s" % (tname, kind), got, y, e, "k=%d n=%d" % (k, n))
            W.expect(np.array_equal(_bits(got), _bits(gpu.op_mat_mat(t, raw, X, n))), "%s %s k=%d: not deterministic" % (tname, kind, k))
    W.done()


@pytest.mark.parametrize("k,n,plan", [(1280, 13312, (52, 3, 2, 1)), (2048, 16640, (65, 3, 3, 2))])
@pytest.mark.parametrize("tname", mr.FUSED)
def test_gemm_several_blocks_per_split(gpu, pkg, orc, tname, k, n, plan):
    """More than one k-block per workgroup and a last split shorter than the others, at m = 17 and m = 1."""
    assert pr.pf_plan([n], k) == plan
    W = Worst()
    t = mr.TYPE[tname]
    raw = _raw(pkg, orc, tname, "full", k, n, k)
    X = pr.act_block(k, M, k + 1)
    y, e = pr.gemm_ref(tname, raw, k, n, pr.x_operand(X), plan[1])
    got = gpu.op_mat_mat(t, raw, X, n)
    W.check("gemm %s k=%d m=17" % (tname, k), got, y, e)
    one = gpu.op_mat_mat(t, raw, X[:1], n)
    W.check("gemm %s k=%d m=1" % (tname, k), one, y[:1], e[:1])
    W.expect(np.array_equal(_bits(one), _bits(got[:1])), "token 0 alone differs from token 0 of 17")
    W.done()


MS = (1, 15, 16, 17, 32, 33, 64, 65, 127, 128)


@pytest.mark.parametrize("tname", mr.FUSED)
def test_gemm_token_tile_widths(gpu, pkg, orc, tname):
    """The MT = 2 / 4 / 8 instances at their edges: rows 0..m-1 inside the bound, and bit-identical when the same rows are
    followed by other rows in a larger block (token independence across the instances)."""
    assert [pr.m_tile_width(m) for m in MS] == [2, 2, 2, 2, 2, 4, 4, 8, 8, 8]
    W = Worst()
    t = mr.TYPE[tname]
    k, n = 512, 272
    raw = _raw(pkg, orc, tname, "quantized", k, n, 77)
    X = pr.act_block(k, 128, 5)
    Z = np.random.default_rng(6).standard_normal((128, k)).astype(np.float32)
    y, e = pr.gemm_ref(tname, raw, k, n, pr.x_operand(X), pr.pf_plan([n], k)[1])
    got = {m: gpu.op_mat_mat(t, raw, X[:m], n) for m in MS}
    for i, m in enumerate(MS):
        W.check("gemm %s widths" % tname, got[m], y[:m], e[:m], "m=%d" % m)
        if i + 1 < len(MS):
            m2 = MS[i + 1]
            big = gpu.op_mat_mat(t, raw, np.concatenate([X[:m], Z[m:m2]]), n)
            W.expect(np.array_equal(_bits(big[:m]), _bits(got[m])), "%s: rows 0..%d change inside a block of %d" % (tname, m - 1, m2))
    W.done()


# ---- the layer steps
EPS = 1e-5
NAN_BITS = np.uint32(0x7FC0BEEF)
MAX_SEQ = 160
ROPE_BASE = 10000.0
QKV_MIXES = [("Q4_K", "Q4_K", "Q6_K"), ("Q5_K", "Q5_K", "Q6_K"), ("Q4_K", "Q8_0", "Q4_0"), ("Q8_0", "Q8_0", "Q8_0")]
# head_dim, q heads per kv head, biases, NeoX pairing, pos0 (None: the block ends at the cache's last row), tokens
QKV_CASES = [(64, 1, False, 0, 0, 1), (64, 4, True, 1, 5, 19), (128, 1, True, 0, None, 128), (128, 4, False, 1, 5, 128),
             (64, 4, False, 0, None, 19), (128, 4, True, 1, 0, 1),
             # the pairs the six above leave out: NeoX with g = 1, one token at the cache's last row, the cache's end with biases and NeoX
             (64, 1, True, 1, None, 1), (128, 1, False, 1, 5, 19), (64, 4, True, 1, None, 128), (128, 1, True, 1, 0, 128)]


def _block(H, m, seed):
    rng = np.random.default_rng(seed)
    return pr.act_block(H, m, seed), (1 + 0.2 * rng.standard_normal(H)).astype(np.float32)


@pytest.fixture(scope="module")
def rope_cs(orc):
    memo = {}

    def get(pos, head_dim):
        if (pos, head_dim) not in memo:
            memo[pos, head_dim] = mr.rope_cs(orc, pos, head_dim, ROPE_BASE, 1.0)
        return memo[pos, head_dim]
    return get


@pytest.mark.parametrize("mix", QKV_MIXES, ids=lambda mx: "-".join(mx))
def test_qkv_step(gpu, pkg, orc, rope_cs, mix):
    """Three segments in one launch (the mixed-format kernel instances), 1/rms from the sums of squares, biases, both RoPE pairings;
    q and the cache rows pos0 .. pos0 + m - 1 inside the bound, every other cache element untouched, bit for bit."""
    W = Worst()
    H = 256
    for ci, (hd, g, with_bias, neox, pos0, m) in enumerate(QKV_CASES):
        n_kv = 256 // hd if g == 1 else 1
        n_heads = n_kv * g
        if n_heads * hd % 256:
            n_heads, n_kv = 2 * n_heads, 2 * n_kv
        QD, KD = n_heads * hd, n_kv * hd
        pos0 = MAX_SEQ - m if pos0 is None else pos0
        rng = np.random.default_rng(40 + ci)
        raws = [_raw(pkg, orc, t, mr.WEIGHT_KINDS[(ci + s) % 4], H, n, 500 + 10 * ci + s) for s, (t, n) in enumerate(zip(mix, (QD, KD, KD)))]
        ops = [pr.Operand(t, raw, H, n) for t, raw, n in zip(mix, raws, (QD, KD, KD))]
        biases = [rng.standard_normal(n).astype(np.float32) if with_bias else None for n in (QD, KD, KD)]
        h, nw = _block(H, m, 60 + ci)
        assert all(pr.domain(op.a, op.o, h * nw, op.S, op.O) for op in ops)
        cs = [rope_cs(pos0 + t, hd) for t in range(m)]
        (q, eq), (k, ek), (v, ev) = pr.qkv_step(ops, h, nw, EPS, biases, cs, hd, n_kv, bool(neox))
        cache = np.full((n_kv, MAX_SEQ, hd), NAN_BITS, np.uint32).view(np.float32)
        args = ([mr.TYPE[t] for t in mix], raws, biases, h, nw, EPS, hd, n_heads, n_kv, neox, cache, cache, pos0, ROPE_BASE, 1.0)
        gq, gk, gv = gpu.op_pf_qkv(*args)
        what = "hd=%d g=%d bias=%d neox=%d pos0=%d m=%d" % (hd, g, with_bias, neox, pos0, m)
        W.check("qkv %s q" % "-".join(mix), gq, q, eq, what)
        for name, got, ref, err in (("k", gk, k, ek), ("v", gv, v, ev)):
            W.check("qkv %s %s rows" % ("-".join(mix), name), got[:, pos0:pos0 + m].transpose(1, 0, 2), ref, err, what)
            rest = np.delete(_bits(got), np.s_[pos0:pos0 + m], axis=1)
            W.expect(bool(np.all(rest == NAN_BITS)), "%s cache touched outside rows %d..%d (%s)" % (name, pos0, pos0 + m - 1, what))
        if ci == 1:
            again = gpu.op_pf_qkv(*args)
            W.expect(all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((gq, gk, gv), again)), "qkv step not deterministic (%s)" % what)
    W.done()


def _check_block_outputs(W, path, hidden, xh, ssq, next_nw, what):
    """The step's by-products: the next XH is f16(hidden * next_nw) of the RETURNED f32 hidden bit for bit (none without a next norm
    weight), the sums of squares are those of the returned hidden (chunks past the row's are never written: they keep the NaN fill)."""
    if next_nw is None:
        W.expect(bool(np.isnan(xh).all()), "%s %s: a next XH was returned although no next norm weight was given" % (path, what))
    else:
        want = pr.x_operand(hidden, next_nw)
        bad = np.argwhere(xh.astype(np.float64) != want)
        W.expect(len(bad) == 0, "%s %s: next XH is not f16(hidden * nw) at %d elements, first (token, column) %s: got %r want %r" % (
            path, what, len(bad), bad[:1].tolist(), xh[tuple(bad[0])] if len(bad) else None, want[tuple(bad[0])] if len(bad) else None))
    s, es = pr.ssq_ref(hidden)
    W.check(path + " ssq", ssq[:, :s.shape[1]], s, es, what)
    W.expect(bool(np.all(_bits(ssq[:, s.shape[1]:]) == NAN_BITS)), "%s %s: sums of squares written past the row's chunks" % (path, what))


@pytest.mark.parametrize("k,H", [(512, 2048), (256, 4096)])
@pytest.mark.parametrize("tname", mr.FUSED)
def test_linear_step(gpu, pkg, orc, tname, k, H):
    """The wo step: residual + bias, the next XH and the sums of squares (H = 4096: two chunks)."""
    W = Worst()
    m = 19
    raw = _raw(pkg, orc, tname, "quantized", k, H, k + H)
    op = pr.Operand(tname, raw, k, H)
    rng = np.random.default_rng(k)
    x = pr.act_block(k, m, 3 * k)
    resid, bias = rng.standard_normal((m, H)).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    nn = (1 + 0.2 * rng.standard_normal(H)).astype(np.float32)
    y, e = pr.resid_step(op, pr.x_operand(x), resid, bias)
    hid, xh, ssq = gpu.op_pf_linear(mr.TYPE[tname], raw, x, resid, nn, bias=bias)
    W.check("linear %s" % tname, hid, y, e, "k=%d H=%d" % (k, H))
    _check_block_outputs(W, "linear %s" % tname, hid, xh, ssq, nn, "k=%d H=%d" % (k, H))
    again = gpu.op_pf_linear(mr.TYPE[tname], raw, x, resid, nn, bias=bias)
    W.expect(all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((hid, xh, ssq), again)), "linear step not deterministic")
    W.done()


@pytest.mark.parametrize("H,F,with_next", [(2048, 768, True), (4096, 512, False)])
@pytest.mark.parametrize("tname", mr.FUSED)
def test_ffn_step(gpu, pkg, orc, tname, H, F, with_next):
    """The dense FFN step: gate|up in one launch (two segments), SwiGLU with the 1/rms from the sums of squares -> the f16 rows the
    down GEMM reads (checked against the reference plus one f16 rounding), the down GEMM judged on those rows, the residual."""
    W = Worst()
    m = 19
    tdown = "Q6_K" if tname in ("Q4_K", "Q5_K") else tname                  # the _M mixes' ffn_down
    rg, ru = _raw(pkg, orc, tname, "quantized", H, F, H + 1), _raw(pkg, orc, tname, "synth", H, F, H + 2)
    rd = _raw(pkg, orc, tdown, "quantized", F, H, H + 3)
    h, nw = _block(H, m, H + F)
    nn = (1 + 0.2 * np.random.default_rng(F).standard_normal(H)).astype(np.float32) if with_next else None
    og, ou, od = pr.Operand(tname, rg, H, F), pr.Operand(tname, ru, H, F), pr.Operand(tdown, rd, F, H)
    act, eact = pr.swiglu_step(og, ou, h, nw, EPS)
    hid, xh, ssq, gact = gpu.op_pf_ffn(mr.TYPE[tname], rg, ru, mr.TYPE[tdown], rd, h, nw, F, next_nw=nn, eps=EPS)
    what = "H=%d F=%d" % (H, F)
    W.check("ffn %s act" % tname, gact, act, pr.f16_store_bound(act, eact), what)
    W.expect(np.array_equal(gact.astype(np.float64), pr.f16(gact)), "act rows are not f16 values")
    y, e = pr.resid_step(od, gact.astype(np.float64), h)
    W.check("ffn %s down" % tname, hid, y, e, what)
    _check_block_outputs(W, "ffn %s" % tname, hid, xh, ssq, nn, what)
    again = gpu.op_pf_ffn(mr.TYPE[tname], rg, ru, mr.TYPE[tdown], rd, h, nw, F, next_nw=nn, eps=EPS, want_act=with_next)
    W.expect(all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((hid, ssq), (again[0], again[2]))), "ffn step not deterministic")
    W.expect(np.array_equal(_bits(gact), _bits(again[3])) if with_next else again[3] is None, "ffn step: act rows not deterministic")
    W.done()


# ---- the MoE step
MOE_FORMATS = [("Q5_K", "Q6_K"), ("Q4_K", "Q6_K"), ("Q8_0", "Q8_0"), ("Q4_0", "Q4_0")]
# experts, per token, tokens, expert width, routing
MOE_CASES = [(8, 2, 1, 256, "random"), (8, 2, 20, 1024, "random"), (8, 2, 128, 256, "random"), (4, 1, 20, 256, "random"),
             (4, 1, 128, 1024, "random"), (8, 2, 128, 256, "same"), (8, 2, 20, 256, "ragged")]


def _moe_inputs(E, top_k, m, routing, seed):
    """(hidden [m][256], router [E][256]).  random: Gaussian rows and router.  same: every token picks experts 2 then 5 (counts m, m
    and zeros: the GEMM's early return).  ragged: 20 tokens in three groups that pick (0, 1) x 16, (1, 2) x 1, (3, 4) x 3: counts
    16, 17, 1, 3, 3 — a full tile, a tile and one row, a single row."""
    H = 256
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((m, H)).astype(np.float32)
    wr = (rng.standard_normal((E, H)) / 16).astype(np.float32)
    if routing != "random":
        # column d(t) carries the token's group; the router reads only those columns: logit_e = c[e][d] * x'_d
        group = np.zeros(m, int) if routing == "same" else np.repeat([0, 1, 2], [16, 1, 3])
        h = (0.1 * h).astype(np.float32)
        h[:, :4] = 0.0
        h[np.arange(m), group] = 4.0
        c = -np.arange(1.0, E + 1)[:, None] * np.ones((1, 4))
        for d, (first, second) in enumerate([(2, 5)] if routing == "same" else [(0, 1), (1, 2), (3, 4)]):
            c[first, d], c[second, d] = 3.0, 2.0
        wr = np.zeros((E, H), np.float32)
        wr[:, :4] = c
    return h, wr


@pytest.mark.parametrize("case", range(len(MOE_CASES)), ids=lambda i: "E%d-k%d-m%d-w%d-%s" % MOE_CASES[i])
def test_moe_step(gpu, pkg, orc, case):
    """The router, the grouping tables against their restatement, every expert's SwiGLU rows, and the hidden output against the
    float64 sum in selection order; routing from the float64 router, the kernel's own where the margin is inside the router's bound."""
    E, top_k, m, EI, routing = MOE_CASES[case]
    tgu, tdn = MOE_FORMATS[case % len(MOE_FORMATS)]
    H = 256
    W = Worst()
    assert pr.moe_eligible(E, top_k)
    h, wr = _moe_inputs(E, top_k, m, routing, 90 + case)
    rng = np.random.default_rng(case)
    nw, nn = ((1 + 0.2 * rng.standard_normal(H)).astype(np.float32) for _ in range(2))
    kinds = ["quantized", "synth", "full", "quantized"]
    rg = [_raw(pkg, orc, tgu, kinds[e % 4], H, EI, 1000 * case + e) for e in range(E)]
    ru = [_raw(pkg, orc, tgu, kinds[(e + 1) % 4], H, EI, 1000 * case + 100 + e) for e in range(E)]
    rd = [_raw(pkg, orc, tdn, kinds[(e + 2) % 4], EI, H, 1000 * case + 200 + e) for e in range(E)]
    o = gpu.op_pf_moe(mr.TYPE[tgu], np.concatenate(rg), np.concatenate(ru), mr.TYPE[tdn], np.concatenate(rd), wr, E, top_k, h, nw, EI,
                      next_nw=nn, eps=EPS)
    # routing
    sel, w, marg, werr = pr.route(h, nw, EPS, wr, top_k)
    print("MARGINAL %d of %d tokens" % (marg.sum(), m))
    assert marg.sum() <= 0.05 * m, "the reference's own routing is not decided for %d of %d tokens" % (marg.sum(), m)
    W.expect(np.array_equal(o["sel"][~marg], sel[~marg]), "selection differs from the float64 router on a decided token")
    ok_sel = bool(np.all((o["sel"] >= 0) & (o["sel"] < E))) and all(len(set(r)) == top_k for r in o["sel"].tolist())
    assert ok_sel, "the kernel's selection is not %d distinct experts per token" % top_k
    w[marg] = pr.route_weights(h[marg], nw, EPS, wr, o["sel"][marg])
    W.check("moe router weights", o["w"], w, np.broadcast_to(werr[:, None], w.shape), MOE_CASES[case])
    # the tables, from the kernel's own selection
    counts, bases, lists, rowmap, tokmap = pr.moe_group(o["sel"], E)
    for name, want in (("counts", counts), ("bases", bases), ("lists", lists), ("rowmap", rowmap), ("tokmap", tokmap)):
        W.expect(np.array_equal(o[name], want), "grouping table %s differs from its restatement" % name)
    if routing == "same":
        W.expect(counts.tolist() == [0, 0, m, 0, 0, m, 0, 0], "routing 'same' did not give counts m, m and zeros: %s" % counts.tolist())
    if routing == "ragged":
        W.expect(counts.tolist() == [16, 17, 1, 3, 3, 0, 0, 0], "routing 'ragged' gave counts %s" % counts.tolist())
    # the experts and the combine
    ops = lambda t, raws, k, n: [pr.Operand(t, r, k, n) for r in raws]
    y, e, acts = pr.moe_step(ops(tgu, rg, H, EI), ops(tgu, ru, H, EI), ops(tdn, rd, EI, H), h, nw, EPS, o["sel"], o["w"], act_got=o["act"])
    for ex in range(E):
        c = int(counts[ex])
        if c:
            W.check("moe %s act" % tgu, o["act"][ex, :c], acts[ex][0], pr.f16_store_bound(*acts[ex]), "expert %d" % ex)
        W.expect(bool(np.isnan(o["act"][ex, c:]).all()), "expert %d: SwiGLU rows written past its %d rows" % (ex, c))
    W.check("moe %s/%s hidden" % (tgu, tdn), o["hidden"], y, e, MOE_CASES[case])
    _check_block_outputs(W, "moe", o["hidden"], o["xh"], o["ssq"], nn, MOE_CASES[case])
    if case in (1, 6):
        again = gpu.op_pf_moe(mr.TYPE[tgu], np.concatenate(rg), np.concatenate(ru), mr.TYPE[tdn], np.concatenate(rd), wr, E, top_k, h, nw, EI,
                              next_nw=nn, eps=EPS, want_act=case == 1)                  # (case 6: the entry point without act_out)
        W.expect(all(np.array_equal(_bits(o[k_]), _bits(again[k_])) for k_ in again), "MoE step not deterministic")
    W.done()


@pytest.mark.parametrize("E,top_k", [(8, 2), (9, 2), (8, 4)])
def test_moe_eligibility(pkg, E, top_k):
    """The batched path takes a MoE model only when a full block's rows, padded to 16 per expert, fit the shared row space; a model
    outside it prefills token by token, bit-identical to prefill_token."""
    cfg = pkg.make_config("test-moe", max_seq_len=64, num_experts=E, num_experts_per_token=top_k)
    model = pkg.SynthModel(cfg, mix="Q5_K_M")
    a = pkg.HipGpuInference.from_model(model, 64)
    try:
        assert a.prefill_is_batched() == pr.moe_eligible(E, top_k) == ((E, top_k) == (8, 2))
        if not a.prefill_is_batched():
            b = pkg.HipGpuInference.from_model(model, 64)
            try:
                prompt = [3, 500, 41, 7, 900, 12, 77, 5]
                a.forward_batch(prompt)
                for t in prompt:
                    b.prefill_token(t)
                assert np.array_equal(a.forward(5), b.forward(5))
            finally:
                b.close()
    finally:
        a.close()
