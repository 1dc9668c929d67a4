"""The launches of a decode step around the fused mat-vecs, each on its own against tests/step_ref.py: the three embedding launches
(rows bit for bit, the first layer's XQ image and sums of squares, the state words, the multi-sequence strides), qkv_forward's unfused
and staged branches (NeoX and interleaved RoPE, expanded weight types, kv_store_kernel), the unfused gate / up pair with silu_mul in
place, both two-stage arg-max launches on ties, and lgh_batch_create's refusals by reason.  Each test prints `WORST <path>: err / bound`
and collects every failure before asserting.  tests/test_step_ref.py shows on the CPU that these inputs tell the kernels from their
likely mistakes.

Tables are 40 rows: the row index times hidden is computed in 64 bits by all three kernels, and a table past 2^32 elements — the only
size at which that could show — would take gigabytes; it is deliberately left out."""
import numpy as np
import pytest

import matvec_ref as mr
import step_ref as sr
from test_gpu_matvec import Worst

pytestmark = pytest.mark.gpu

SENTINEL_POS = -0x5A5A5A5B        # what op_embed presets the position word to


def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(sr.bits(a[k]), sr.bits(b[k])) for k in ("rows", "image", "ssq", "state"))


def _check_image(W, path, what, r, s, row, nw):
    W.expect(r["image"] is not None, "%s: no image was left" % what)
    if r["image"] is None:
        return
    ri, rs, rq = sr.image_ratios(r["image"][s], r["ssq"][s], row, nw)
    for name, ratio in (("image", ri), ("sums", rs), ("ssq", rq)):
        key = "%s %s" % (path, name)
        W.w[key] = max(W.w.get(key, 0.0), ratio)
        W.expect(ratio <= 1.0, "%s: %s ratio %.3g" % (what, name, ratio))
    W.expect(sr.image_tails_kept(r["image"][s]), "%s: record tails changed" % what)
    W.expect(sr.filled(r["ssq"][s][len(row) // 16:]), "%s: floats behind the row's sums of squares changed" % what)


@pytest.mark.parametrize("tname", sr.EMBED_TYPES)
def test_embedding_launches(gpu, pkg, orc, tname):
    W = Worst()
    t = sr.TYPE[tname]
    for hidden in sr.embed_hiddens(tname):
        raw = sr.table(tname, hidden, orc, pkg.synth.fill_tensor)
        nw = sr.norm_weight(hidden, 3)
        rows = {tok: sr.embed_row(orc, tname, raw, hidden, tok) for tok in sr.EMBED_TOKENS}
        has_img = hidden % 256 == 0
        # ---- embed_kernel through embed_forward: the row, the image when the engine asks for one, the state words
        for tok, p in zip(sr.EMBED_TOKENS, (0, sr.MAX_SEQ - 1, 5)):
            for use_nw in (True, False):
                what = "embed %s hidden %d token %d nw=%s" % (tname, hidden, tok, use_nw)
                kw = dict(norm_w=nw if use_nw else None, fill=sr.FILL, state=(tok, p))
                r, r2 = gpu.op_embed(0, t, raw, sr.VOCAB, hidden, None, **kw), gpu.op_embed(0, t, raw, sr.VOCAB, hidden, None, **kw)
                W.expect(_same(r, r2), what + ": two runs differ")
                W.expect(np.array_equal(sr.bits(r["rows"][0]), sr.bits(rows[tok])), what + ": the row differs from the oracle's dequantization")
                st = r["state"]
                W.expect((st[0], st[1], st[2]) == (tok, p, p + 1) and not np.any(st[3:]),
                         what + ": state words %s from token %d, position %d, next %d" % (list(st), tok, SENTINEL_POS, p))
                if use_nw and has_img:
                    _check_image(W, "embed", what, r, 0, rows[tok], nw)
                else:
                    W.expect(r["image"] is None, what + ": an image the engine does not ask for")
        # ---- embed_multi_kernel: one grid row per sequence, the images and partials at the step's strides
        for toks in ([17], [0, sr.VOCAB - 1, 17], [17, 0, 17] + [sr.VOCAB - 1 - i for i in range(13)]):
            what = "embed_multi %s hidden %d n %d" % (tname, hidden, len(toks))
            r, r2 = (gpu.op_embed(1, t, raw, sr.VOCAB, hidden, toks, norm_w=nw, fill=sr.FILL) for _ in range(2))
            W.expect(_same(r, r2), what + ": two runs differ")
            W.expect(r["rows"].shape[0] == len(toks) + 1 and sr.filled(r["rows"][len(toks)]), what + ": the row behind the last sequence changed")
            W.expect((r["image"] is not None) == has_img, what + ": image left %s" % (r["image"] is not None))
            if r["image"] is not None:
                W.expect(sr.filled(r["image"][len(toks)]) and sr.filled(r["ssq"][len(toks)]), what + ": image or partials behind the last sequence changed")
            for s, tok in enumerate(toks):
                row = rows[tok] if tok in rows else sr.embed_row(orc, tname, raw, hidden, tok)
                W.expect(np.array_equal(sr.bits(r["rows"][s]), sr.bits(row)), "%s: sequence %d differs from row %d" % (what, s, tok))
                if has_img:
                    _check_image(W, "embed_multi", "%s sequence %d" % (what, s), r, s, row, nw)
        # ---- embed_batch_kernel: m rows, no image
        rng = np.random.default_rng(hidden)
        for m in (1, 17, 128):
            toks = np.concatenate([[17, 0, sr.VOCAB - 1, 17][:m], rng.integers(0, sr.VOCAB, max(0, m - 4))]).astype(np.int32)
            what = "embed_batch %s hidden %d m %d" % (tname, hidden, m)
            r, r2 = (gpu.op_embed(2, t, raw, sr.VOCAB, hidden, toks, norm_w=nw, fill=sr.FILL) for _ in range(2))
            W.expect(_same(r, r2), what + ": two runs differ")
            W.expect(r["image"] is None and sr.filled(r["rows"][m]), what + ": an image was left or the row behind the last token changed")
            whole = orc.dequantize(t, raw, sr.VOCAB * hidden).reshape(sr.VOCAB, hidden)
            W.expect(np.array_equal(sr.bits(r["rows"][:m]), sr.bits(whole[toks])), what + ": rows differ from the oracle's dequantization")
    W.done()


def _qkv_case(W, gpu, orc, types, neox, with_bias, staged, hd, nh, nkv):
    ws, nw, biases, rows = sr.qkv_inputs(types, hd, nh, nkv, with_bias, orc)
    tids = [sr.TYPE[t] for t in types]
    fam = mr.kernel_family(types[0], sr.QKV_HIDDEN)
    path = "qkv %s %s%s" % (fam, "neox" if neox else "interleaved", " staged" if staged else "")
    for pi, pos in enumerate(sr.QKV_POS):
        x = sr.qkv_x(pi, with_bias, pos)
        kc, vc = sr.nan_cache(nkv, hd), sr.nan_cache(nkv, hd)
        args = (tids, ws, biases, x, nw, sr.EPS, hd, nh, nkv, kc, vc, pos, sr.ROPE_BASE, sr.ROPE_SCALE)
        out, out2 = (gpu.op_qkv_forward(*args, neox=neox, staged=staged) for _ in range(2))
        tag = "%s/%s/%s d%d%s%s%s pos %d" % (types + (hd, " neox" if neox else "", " bias" if with_bias else "", " staged" if staged else "", pos))
        W.expect(all(np.array_equal(sr.bits(a), sr.bits(b)) for a, b in zip(out, out2)), tag + ": two runs differ")
        q, k2, v2, st = out
        (yq, eq), (yk, ek), (yv, ev) = sr.qkv_ref(orc, types, ws, nw, biases, rows, x, pos, hd, neox)
        W.check(path + " Q", q, yq, eq, tag)
        if staged:
            W.check(path + " K row", st[0], yk, ek, tag)
            W.check(path + " V row", st[1], yv, ev, tag)
            W.expect(np.all(sr.bits(k2) == sr.NAN_BITS) and np.all(sr.bits(v2) == sr.NAN_BITS), tag + ": a staged launch wrote a cache")
        else:
            W.check(path + " K row", k2[:, pos, :].reshape(-1), yk, ek, tag)
            W.check(path + " V row", v2[:, pos, :].reshape(-1), yv, ev, tag)
            for f in sr.cache_failures(k2, pos, yk, ek, tag + " K cache") + sr.cache_failures(v2, pos, yv, ev, tag + " V cache"):
                W.expect(False, f)


@pytest.mark.parametrize("hd,nh,nkv", sr.QKV_SHAPES)
@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("types,neox,with_bias", sr.QKV_UNFUSED)
def test_unfused_qkv(gpu, pkg, orc, types, neox, with_bias, staged, hd, nh, nkv):
    """Three mat-vec launches, rope_kernel in either pairing, then kv_store_kernel — or, staged, the rows left in kv_tmp."""
    W = Worst()
    _qkv_case(W, gpu, orc, types, neox, with_bias, staged, hd, nh, nkv)
    W.done()


@pytest.mark.parametrize("hd,nh,nkv", sr.QKV_SHAPES)
@pytest.mark.parametrize("types,neox,with_bias", sr.QKV_FUSED)
def test_fused_qkv_staged(gpu, pkg, orc, types, neox, with_bias, hd, nh, nkv):
    """The fused interleaved launch as the byte and TurboQuant caches run it: EPI_ROPE_Q on K into k_new, EPI_STORE on V into v_new."""
    W = Worst()
    _qkv_case(W, gpu, orc, types, neox, with_bias, True, hd, nh, nkv)
    W.done()


@pytest.mark.parametrize("types,neox", [(("Q5_0", "Q5_0", "Q5_0"), False), (("F16", "F16", "F16"), True)])
def test_unfused_qkv_refuses_biases_on_expanded_types(gpu, pkg, orc, types, neox):
    hd, nh, nkv = sr.QKV_SHAPES[0]
    ws, nw, biases, _ = sr.qkv_inputs(types, hd, nh, nkv, True, orc)
    kc = sr.nan_cache(nkv, hd)
    with pytest.raises(pkg.BackendError) as ei:
        gpu.op_qkv_forward([sr.TYPE[t] for t in types], ws, biases, sr.qkv_x(0, True, 0), nw, sr.EPS, hd, nh, nkv, kc, kc, 0, sr.ROPE_BASE,
                           sr.ROPE_SCALE, neox=neox)
    assert ei.value.variant == "Unsupported" and "bias on a non-quantized linear layer" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("tg,tu", sr.GATEUP_CASES)
def test_unfused_gate_up(gpu, pkg, orc, tg, tu):
    """Two mat-vec launches and silu_mul_kernel with `out` aliasing `gate`, as ffn_gateup_forward runs them."""
    W = Worst()
    wg, wu, nw = sr.gateup_inputs(tg, tu, orc)
    path = "gate/up %s/%s" % (tg, tu)
    for ai, act in enumerate(mr.ACT_KINDS):
        x = mr.activation(act, sr.FFN_HIDDEN, 40 + ai)
        got, got2 = (gpu.op_ffn_gateup(sr.TYPE[tg], wg, sr.TYPE[tu], wu, x, nw, sr.EPS, sr.FFN) for _ in range(2))
        W.expect(np.array_equal(sr.bits(got), sr.bits(got2)), "%s %s: two runs differ" % (path, act))
        y, e = sr.gateup_ref(orc, tg, wg, tu, wu, nw, x)
        W.check(path, got, y, e, act)
    W.done()


@pytest.mark.parametrize("n", sr.ARGMAX_N)
def test_argmax_ties(gpu, orc, n):
    """argmax_stage1/2 and argmax_multi_stage1/2, exact: the last maximal index, for maxima planted in one workgroup, across workgroups,
    at both ends, as signed zeros and infinities, with every sequence's maxima somewhere else — and n below the 64 x 256 grid, where
    workgroups have no element."""
    fails = []
    rows = sr.argmax_rows(n, n)
    for name, row, is_tie in rows:
        want = sr.argmax_last(row)
        assert want == orc.argmax_last(row) and is_tie == (int(np.sum(row == row.max())) > 1), (n, name)   # the case is what it claims
        got = int(gpu.op_argmax(row)[0])
        if got != want:
            fails.append("n %d %s: argmax_launch gave %d, want %d" % (n, name, got, want))
    for n_seq in sr.ARGMAX_SEQS[1:]:
        for b, batch in enumerate(sr.argmax_batches(n, n_seq, n)):
            want = [sr.argmax_last(r) for r in batch]
            got = gpu.op_argmax(batch, multi=True).tolist()
            if got != want:
                fails.append("n %d n_seq %d batch %d: argmax_multi_launch gave %s, want %s" % (n, n_seq, b, got, want))
            if got != gpu.op_argmax(batch, multi=True).tolist():
                fails.append("n %d n_seq %d batch %d: two runs differ" % (n, n_seq, b))
    # NaN logits are outside the reference's domain (its comparison panics): only that both launches pick the same token
    nan_row = rows[0][1].copy()
    nan_row[[0, n // 2, n - 1]] = np.nan
    one = int(gpu.op_argmax(nan_row)[0])
    for n_seq in (1, 3):
        many = gpu.op_argmax(np.stack([nan_row] * n_seq), multi=True).tolist()
        if many != [one] * n_seq:
            fails.append("n %d NaN row: argmax_launch %d, argmax_multi_launch %s" % (n, one, many))
    assert not fails, "\n".join(fails[:20])


REFUSALS = [
    ("NeoX RoPE is not fused into the QKV launch", "Q4_K_M", dict(use_neox_rope=True)),
    ("not in a matrix-core tile layout", "Q5_0", {}),
    ("hidden size and heads x head_dim must be multiples of 256", "Q8_0", dict(num_heads=14, num_kv_heads=2, hidden_size=896)),
    ("attention shape outside the split kernels", "Q4_K_M", dict(num_heads=8, num_kv_heads=4, head_dim=96, hidden_size=768, intermediate_size=1536)),
]


@pytest.mark.parametrize("words,mix,over", REFUSALS)
def test_batch_create_refusals_name_the_reason(gpu, pkg, words, mix, over):
    cfg = pkg.make_config("test-dense", max_seq_len=32, **over)
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix=mix), 32)
    try:
        before = eng.forward(3)
        eng.reset()
        for _ in range(2):
            with pytest.raises(pkg.BackendError) as ei:
                eng.batch_create(4)
            assert ei.value.variant == "Unsupported" and "multi-sequence decode" in str(ei.value) and words in str(ei.value), str(ei.value)
        # the context's single-sequence decode is what it was
        after = eng.forward(3)
        assert eng.position() == 1 and np.all(np.isfinite(after)) and np.array_equal(sr.bits(after), sr.bits(before))
        toks = eng.decode_greedy(int(np.argmax(after)), 4)
        assert eng.position() == 5 and np.all((toks >= 0) & (toks < cfg.vocab_size))
    finally:
        eng.close()
