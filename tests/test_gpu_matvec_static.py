"""The static launch plans of the matrix-core mat-vec (csrc/matvec_mfma.hip: mvqs_kernel) against the generic kernel, bit for bit.

A plan is chosen by geometry (k = 4096 or 14336, formats, passes, epilogues), never by the number of rows, so a launch of a few
tiles runs the code of the full-size one.  Every launch goes through the engine's own launch assembly twice — once as it runs by
default and once with LGH_FLAG_MV_GENERIC, which makes mvq_launch ignore the plan table — and everything the launch leaves is
compared bitwise: outputs, XQ images, sums of squares, cache rows.  One case per plan also goes against the float64 restatement in
tests/matvec_ref.py with that module's own bound, so that a defect both kernels share cannot hide behind the equality."""
import contextlib

import numpy as np
import pytest

import matvec_ref as mr

pytestmark = pytest.mark.gpu

EPS = 1e-5
NAN_BITS = np.uint32(0x7FC0BEEF)


@contextlib.contextmanager
def generic(gpu):
    prev = gpu.op_set_flags(gpu.FLAG_MV_GENERIC)
    try:
        yield
    finally:
        gpu.op_set_flags(prev)


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def within(got, ref, err):
    got = np.asarray(got, np.float64)
    r = np.abs(got - ref) / err
    r[~np.isfinite(got)] = np.inf
    return float(r.max())


def both(gpu, *args, plan=True, **kw):
    """The launch as it runs by default and under LGH_FLAG_MV_GENERIC; asserts which kernel each of them ran."""
    s = gpu.op_linear_image(*args, **kw)
    with generic(gpu):
        g = gpu.op_linear_image(*args, **kw)
    assert s["static"] == (1 if plan else 0), "the default launch ran %s" % ("the generic kernel" if plan else "a static plan")
    assert g["static"] == 0, "LGH_FLAG_MV_GENERIC did not keep the launch on the generic kernel"
    return s, g


def ref_rows(tname, raw, k, n, x, nw=None, bias=None):
    a, o = mr.decode(tname, raw, k, n, None, "mfma")
    return mr.matvec(a, o, x, nw=nw, eps=EPS, bias=bias, family="mfma")


def expect_same(fails, tag, s, g, image):
    if not same(s["out"], g["out"]):
        fails.append("%s: outputs differ (max %.3g)" % (tag, np.abs(s["out"] - g["out"]).max()))
    if image and (s["image"] is None or g["image"] is None):
        fails.append("%s: no XQ image left (static %s, generic %s)" % (tag, s["image"] is not None, g["image"] is not None))
    if not same(s["image"], g["image"]):
        fails.append("%s: XQ images differ" % tag)
    if not same(s["ssq"], g["ssq"]):
        fails.append("%s: sums of squares differ" % tag)


# ---- wo, down (Q4_K and Q6_K): residual, XQ image times the next norm's weights, sums of squares
@pytest.mark.parametrize("tname,k", [("Q4_K", 4096), ("Q4_K", 14336), ("Q6_K", 14336)])
def test_residual_plans(gpu, tname, k):
    n, fails = 48, []
    rng = np.random.default_rng(k + len(tname))
    raw = mr.weights(tname, "full", k, n, 5)
    res = (3 * rng.standard_normal(n)).astype(np.float32)
    nnw = (1 + 0.2 * rng.standard_normal(n)).astype(np.float32)
    for ai, act in enumerate(mr.ACT_KINDS):
        x = mr.activation(act, k, ai + 1)
        s, g = both(gpu, mr.TYPE[tname], raw, k, n, x, resid=res, xq_next=2, next_nw=nnw)
        expect_same(fails, "%s k=%d resid %s" % (tname, k, act), s, g, True)
        if ai == 1:
            y, e = mr.resid(*ref_rows(tname, raw, k, n, x), res)
            r = within(s["out"], y, e)
            print("WORST static %s k=%d resid: %.3g" % (tname, k, r))
            if not r <= 1.0:
                fails.append("%s k=%d resid vs float64: ratio %.3g" % (tname, k, r))
    assert not fails, "\n".join(fails)


# ---- gate | up: two passes, SwiGLU, plain XQ image
def test_gate_up_plan(gpu):
    k, n, fails = 4096, 48, []
    gate, up = mr.weights("Q4_K", "full", k, n, 1), mr.weights("Q4_K", "full", k, n, 2)
    nw = (1 + 0.2 * np.random.default_rng(3).standard_normal(k)).astype(np.float32)
    for ai, act in enumerate(mr.ACT_KINDS):
        x = mr.activation(act, k, ai + 11)
        s, g = both(gpu, mr.TYPE["Q4_K"], gate, k, n, x, w_up=up, norm_w=nw, eps=EPS, xq_next=1)
        expect_same(fails, "gate|up %s" % act, s, g, True)
        if ai == 1:
            y, e = mr.swiglu(*ref_rows("Q4_K", gate, k, n, x, nw=nw), *ref_rows("Q4_K", up, k, n, x, nw=nw))
            r = within(s["out"], y, e)
            print("WORST static gate|up: %.3g" % r)
            if not r <= 1.0:
                fails.append("gate|up vs float64: ratio %.3g" % r)
    assert not fails, "\n".join(fails)


# ---- output projection: norm, store; 40 rows end in a ragged tile
@pytest.mark.parametrize("n", [48, 40])
def test_output_plan(gpu, n):
    k, fails = 4096, []
    raw = mr.weights("Q6_K", "full", k, n, 7)
    nw = (1 + 0.2 * np.random.default_rng(n).standard_normal(k)).astype(np.float32)
    for ai, act in enumerate(mr.ACT_KINDS):
        x = mr.activation(act, k, ai + 21)
        s, g = both(gpu, mr.TYPE["Q6_K"], raw, k, n, x, norm_w=nw, eps=EPS)
        expect_same(fails, "output n=%d %s" % (n, act), s, g, False)
        if ai == 1:
            y, e = ref_rows("Q6_K", raw, k, n, x, nw=nw)
            r = within(s["out"], y, e)
            print("WORST static output n=%d: %.3g" % (n, r))
            if not r <= 1.0:
                fails.append("output n=%d vs float64: ratio %.3g" % (n, r))
    assert not fails, "\n".join(fails)


# ---- fused QKV: one q head, one kv head
@pytest.mark.parametrize("types", [("Q4_K", "Q4_K", "Q6_K"), ("Q4_K", "Q4_K", "Q4_K")])
def test_fused_qkv_plans(gpu, orc, types):
    hidden, hd, nh, nkv, max_seq, base, scale = 4096, 128, 1, 1, 8, 500000.0, 1.0
    fails = []
    rng = np.random.default_rng(len(types[2]) + 40)
    rows = (nh * hd, nkv * hd, nkv * hd)
    ws = [mr.weights(types[s], "full", hidden, rows[s], 30 + s) for s in range(3)]
    nw = (1 + 0.2 * rng.standard_normal(hidden)).astype(np.float32)
    tids = [mr.TYPE[t] for t in types]
    ci = 0
    for with_bias in (False, True):
        biases = [rng.standard_normal(r).astype(np.float32) if with_bias else None for r in rows]
        for pos in (0, 5):
            x = mr.activation(mr.ACT_KINDS[ci % len(mr.ACT_KINDS)], hidden, ci + 31)
            ci += 1
            kc = np.full((nkv, max_seq, hd), NAN_BITS, np.uint32).view(np.float32)
            vc = kc.copy()
            n0 = gpu.static_launches()
            q, k2, v2 = gpu.op_qkv_rope(tids, ws, biases, x, nw, EPS, hd, nh, nkv, kc, vc, pos, base, scale)
            n1 = gpu.static_launches()
            with generic(gpu):
                qg, k2g, v2g = gpu.op_qkv_rope(tids, ws, biases, x, nw, EPS, hd, nh, nkv, kc, vc, pos, base, scale)
            assert (n1 - n0, gpu.static_launches() - n1) == (1, 0), "which kernel ran: static launches %d by default, %d under the flag" % (
                n1 - n0, gpu.static_launches() - n1)
            tag = "%s/%s/%s%s pos %d" % (types + (" bias" if with_bias else "", pos))
            if not (same(q, qg) and same(k2, k2g) and same(v2, v2g)):
                fails.append("%s: q / K cache / V cache differ between the static and the generic kernel" % tag)
            others = np.ones(max_seq, bool)
            others[pos] = False
            if not (np.all(k2[:, others].view(np.uint32) == NAN_BITS) and np.all(v2[:, others].view(np.uint32) == NAN_BITS)):
                fails.append("%s: a cache row other than pos changed" % tag)
            if np.any(k2[:, pos].view(np.uint32) == NAN_BITS) or np.any(v2[:, pos].view(np.uint32) == NAN_BITS):
                fails.append("%s: cache row pos not written" % tag)
            if with_bias and pos == 5:
                c, s = mr.rope_cs(orc, pos, hd, base, scale)
                refs = [ref_rows(types[i], ws[i], hidden, rows[i], x, nw=nw, bias=biases[i]) for i in range(3)]
                yq, eq = mr.rope(*refs[0], c, s, hd)
                yk, ek = mr.rope(*refs[1], c, s, hd)
                r = max(within(q, yq, eq), within(k2[:, pos, :].reshape(-1), yk, ek), within(v2[:, pos, :].reshape(-1), *refs[2]))
                print("WORST static qkv %s: %.3g" % (tag, r))
                if not r <= 1.0:
                    fails.append("%s vs float64: ratio %.3g" % (tag, r))
    assert not fails, "\n".join(fails)


# ---- the arg-max parts the output projection's plan leaves: 1040 rows = 65 workgroups of one tile
@pytest.fixture(scope="module", params=[1040, 1048])
def vocab_case(gpu, request):
    """1040 rows = 65 full workgroups; 1048 = 66, the last one with half a tile (lanes without a row in the last part)."""
    k, n = 4096, request.param
    raw = mr.weights("Q6_K", "full", k, n, 9)
    x = mr.activation("normal", k, 10)
    nw = (1 + 0.2 * np.random.default_rng(11).standard_normal(k)).astype(np.float32)
    with generic(gpu):
        logits = gpu.op_linear_image(mr.TYPE["Q6_K"], raw, k, n, x, norm_w=nw, eps=EPS)["out"]
    return k, n, raw, x, nw, int(np.argmax(logits)), int(np.argmin(logits))


@pytest.mark.parametrize("where", [(35, 44), (35, 44, 700), (0,), (-1,), (0, -1)])
def test_fused_argmax(gpu, vocab_case, where):
    """The maximum twice in one workgroup; once more in a later one (the last index wins); in the first row; in the last row."""
    k, n, raw, x, nw, top, low = vocab_case
    where = tuple(r % n for r in where)
    rb = raw.size // n
    w = raw.copy().reshape(n, rb)
    w[top] = raw.reshape(n, rb)[low]          # the maximum lives only where the case puts it
    for r in where:
        w[r] = raw.reshape(n, rb)[top]
    w = w.reshape(-1)
    kw = dict(norm_w=nw, eps=EPS, want_argmax=True)
    s = gpu.op_linear_image(mr.TYPE["Q6_K"], w, k, n, x, **kw)
    with generic(gpu):
        g = gpu.op_linear_image(mr.TYPE["Q6_K"], w, k, n, x, **kw)
    lg = g["out"]
    assert same(s["out"], lg), "logits differ"
    bits = lg.view(np.uint32)
    assert all(bits[r] == bits[where[0]] for r in where) and np.sum(lg >= lg[where[0]]) == len(where), "the case is not the tie it should be"
    assert g["parts"] == 0 and s["parts"] == (n + 15) // 16, (g["parts"], s["parts"])
    assert (s["static"], g["static"]) == (1, 0)
    assert s["token"] == g["token"] == max(where), (s["token"], g["token"], where)


# ---- a geometry outside the table runs the generic kernel whatever the flag says
def test_plan_table_miss(gpu):
    k, n = 5632, 48
    raw = mr.weights("Q4_K", "full", k, n, 13)
    x = mr.activation("outlier", k, 14)
    nw = (1 + 0.2 * np.random.default_rng(15).standard_normal(k)).astype(np.float32)
    res = np.random.default_rng(16).standard_normal(n).astype(np.float32)
    for kw in (dict(norm_w=nw, eps=EPS, want_argmax=True), dict(resid=res, xq_next=2, next_nw=nw[:n].copy())):
        s, g = both(gpu, mr.TYPE["Q4_K"], raw, k, n, x, plan=False, **kw)
        assert same(s["out"], g["out"]) and same(s["image"], g["image"]) and same(s["ssq"], g["ssq"])
        assert s["token"] == g["token"] and s["parts"] == g["parts"] and s["parts"] in (0, -1)


# ---- whole model at the Llama-3-8B widths: every plan in its place in the decode graph
def test_two_layer_model_static_against_generic(pkg, gpu):
    cfg = pkg.make_config("llama-3-8b", max_seq_len=32, num_layers=2, vocab_size=1040)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")   # layer 0: V and down in Q4_K; layer 1: in Q6_K
    prompt = [3, 1000, 17, 512, 9, 77]
    runs = []
    counts = []
    for flags in (0, gpu.FLAG_MV_GENERIC):
        n0 = gpu.static_launches()
        eng = pkg.HipGpuInference.from_model(model, 32, flags=flags)
        for t in prompt[:-1]:
            eng.prefill_token(t)
        toks = eng.decode_greedy(prompt[-1], 8)
        logits = eng.forward(int(toks[-1]))
        runs.append((toks.copy(), logits.copy(), eng.stats()["graph_nodes"]))
        eng.close()
        counts.append(gpu.static_launches() - n0)
    # every mat-vec launch that was enqueued (eagerly or into a graph) took a plan by default, none under the flag
    assert counts[0] > 0 and counts[1] == 0, counts
    (ts, ls, ns), (tg, lg, ng) = runs
    assert np.array_equal(ts, tg), (ts, tg)
    assert same(ls, lg), "final logits differ (max %.3g)" % np.abs(ls - lg).max()
    assert np.all(np.isfinite(ls))
    assert ns == ng - 1, (ns, ng)   # the first arg-max stage is gone from the greedy graph
