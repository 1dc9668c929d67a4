"""Every decode mat-vec launch against the float64 restatement in tests/matvec_ref.py, through the engine's own launch assembly
(launch_mv -> build_mv_group): the five fused formats on the int8 matrix cores and on the VALU kernel, the f32 fallback, every
epilogue, the fused QKV launch, XQ images handed from launch to launch, and the MoE router.  Each test prints
`WORST <path>: err / bound` and collects every failure before asserting."""
import numpy as np
import pytest

import matvec_ref as mr

pytestmark = pytest.mark.gpu

EPS = 1e-5
NAN_BITS = np.uint32(0x7FC0BEEF)


class Worst:
    def __init__(self):
        self.w, self.fail = {}, []

    def check(self, path, got, ref, err, what=""):
        got = np.asarray(got, np.float64)
        bad = ~np.isfinite(got)
        r = np.abs(got - ref) / err
        r[bad] = np.inf
        m = float(r.max()) if r.size else 0.0
        self.w[path] = max(self.w.get(path, 0.0), m)
        if not m <= 1.0:
            i = int(np.argmax(r))
            self.fail.append("%s %s: index %d got %r ref %r bound %.3g (ratio %.3g)" % (path, what, i, got.flat[i], ref.flat[i], err.flat[i], m))

    def expect(self, cond, msg):
        if not cond:
            self.fail.append(msg)

    def done(self):
        for p in sorted(self.w):
            print("WORST %s: %.3g" % (p, self.w[p]))
        assert not self.fail, "\n".join(self.fail[:20])


def _raw(pkg, orc, tname, kind, k, n, seed):
    return mr.weights(tname, kind, k, n, seed, orc=orc, synth_fill=pkg.synth.fill_tensor)


def _ref(tname, raw, k, n, x, family, orc=None, nw=None, bias=None, xerr=None, rows=2048):
    """matvec_ref.matvec over row slices (keeps the float64 copies of a full-size matrix small)."""
    rb = raw.size // n
    ys, es = [], []
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        a, o = mr.decode(tname, raw[r0 * rb:r1 * rb], k, r1 - r0, orc, family)
        y, e = mr.matvec(a, o, x, nw=nw, eps=EPS, bias=None if bias is None else bias[r0:r1], family=family, xerr=xerr)
        ys.append(y)
        es.append(e)
    return np.concatenate(ys), np.concatenate(es)


MFMA_K = (256, 4096, 5632, 14336, 28672)
MFMA_N = (1, 15, 16, 17, 130, 1024)


@pytest.mark.parametrize("tname", mr.FUSED)
def test_formats_mfma(gpu, pkg, orc, tname):
    W = Worst()
    t = mr.TYPE[tname]
    i = 0
    for wi, kind in enumerate(mr.WEIGHT_KINDS):
        for k in MFMA_K:
            for n in MFMA_N:
                if k * n > 4096 * 1024:
                    continue
                raw = _raw(pkg, orc, tname, kind, k, n, 1000 * wi + k + n)
                acts = mr.ACT_KINDS if (k, n) == (4096, 130) else (mr.ACT_KINDS[i % len(mr.ACT_KINDS)],)
                for act in acts:
                    i += 1
                    x = mr.activation(act, k, i)
                    y, e = _ref(tname, raw, k, n, x, "mfma")
                    got = gpu.op_vec_mat(t, raw, x, n)
                    W.check("mfma %s %s" % (tname, kind), got, y, e, "k=%d n=%d %s" % (k, n, act))
                    if (k, n) == (4096, 130):
                        nw = (1 + 0.2 * np.random.default_rng(i).standard_normal(k)).astype(np.float32)
                        y, e = _ref(tname, raw, k, n, x, "mfma", nw=nw)
                        got2 = gpu.op_norm_vec_mat(t, raw, x, nw, EPS, n)
                        W.check("mfma %s %s norm" % (tname, kind), got2, y, e, act)
                        W.expect(np.array_equal(got.view(np.uint32), gpu.op_vec_mat(t, raw, x, n).view(np.uint32)),
                                 "mfma %s %s %s: not deterministic" % (tname, kind, act))
    W.done()


@pytest.mark.parametrize("tname,k,n", [("Q4_K", 4096, 14336), ("Q6_K", 4096, 128256)])
def test_full_size(gpu, pkg, orc, tname, k, n):
    """The Llama-3-8B gate / up shape and its output head in full."""
    W = Worst()
    raw = mr.weights(tname, "full", k, n, 77)
    x = mr.activation("outlier", k, 78)
    nw = (1 + 0.2 * np.random.default_rng(79).standard_normal(k)).astype(np.float32)
    got = gpu.op_norm_vec_mat(mr.TYPE[tname], raw, x, nw, EPS, n)
    y, e = _ref(tname, raw, k, n, x, "mfma", nw=nw)
    W.check("full-size %s %dx%d" % (tname, n, k), got, y, e)
    W.done()


VALU_K = (32, 96, 576, 896, 960, 4896)


@pytest.mark.parametrize("tname", ["Q8_0", "Q4_0"])
def test_formats_valu(gpu, pkg, orc, tname):
    """mv_kernel: Q8_0 / Q4_0 matrices whose k is not a multiple of 256."""
    W = Worst()
    t = mr.TYPE[tname]
    i = 0
    for wi, kind in enumerate(mr.WEIGHT_KINDS):
        for k in VALU_K:
            for n in (1, 17, 130):
                raw = _raw(pkg, orc, tname, kind, k, n, 2000 * wi + k + n)
                for act in mr.ACT_KINDS if n == 17 else (mr.ACT_KINDS[i % 6],):
                    i += 1
                    x = mr.activation(act, k, i)
                    y, e = _ref(tname, raw, k, n, x, "valu")
                    W.check("valu %s %s" % (tname, kind), gpu.op_vec_mat(t, raw, x, n), y, e, "k=%d n=%d %s" % (k, n, act))
                    nw = (1 + 0.2 * np.random.default_rng(i).standard_normal(k)).astype(np.float32)
                    y, e = _ref(tname, raw, k, n, x, "valu", nw=nw)
                    W.check("valu %s %s norm" % (tname, kind), gpu.op_norm_vec_mat(t, raw, x, nw, EPS, n), y, e, "k=%d n=%d %s" % (k, n, act))
    W.done()


@pytest.mark.parametrize("tname", mr.EXPANDED)
def test_f32_fallback(gpu, pkg, orc, tname):
    W = Worst()
    t = mr.TYPE[tname]
    for k, n in ((256, 7), (1024, 40), (4096, 33)):
        raw = _raw(pkg, orc, tname, "quantized", k, n, k + n)
        for ai, act in enumerate(mr.ACT_KINDS):
            x = mr.activation(act, k, ai)
            y, e = _ref(tname, raw, k, n, x, "f32", orc=orc)
            W.check("f32 %s" % tname, gpu.op_vec_mat(t, raw, x, n), y, e, "k=%d %s" % (k, act))
            nw = (1 + 0.2 * np.random.default_rng(ai).standard_normal(k)).astype(np.float32)
            y, e = _ref(tname, raw, k, n, x, "f32", orc=orc, nw=nw)
            W.check("f32 %s norm" % tname, gpu.op_norm_vec_mat(t, raw, x, nw, EPS, n), y, e, "k=%d %s" % (k, act))
    W.done()


# ---- epilogues and XQ chains: launch A (+ its XQ image) -> launch B
CHAIN_CASES = [
    # (type A, k, n_a, type B, n_b)
    ("Q4_K", 4096, 1024, "Q4_K", 256),
    ("Q6_K", 5632, 2048, "Q6_K", 130),
    ("Q5_K", 2048, 5632, "Q4_K", 64),
    ("Q8_0", 4096, 512, "Q8_0", 48),
    ("Q4_0", 4096, 768, "Q4_0", 40),
    ("Q8_0", 896, 4864, "Q8_0", 32),     # A on the VALU kernel (Qwen2.5-0.5B widths), B on the matrix cores
    ("Q4_0", 576, 1536, "Q4_K", 32),
]


@pytest.mark.parametrize("ta,k,na,tb,nb", CHAIN_CASES)
def test_epilogues_and_xq_chain(gpu, pkg, orc, ta, k, na, tb, nb):
    chain_case(gpu, ta, k, na, tb, nb)


def chain_case(gpu, ta, k, na, tb, nb, tag=""):
    """The seven (epilogue, xq_next) pairs of launch A [na, k] feeding launch B [nb, na]; `tag` leads every WORST line."""
    W = Worst()
    fam_a, fam_b = mr.kernel_family(ta, k), mr.kernel_family(tb, na)
    rng = np.random.default_rng(k + na)
    wa = mr.weights(ta, "full", k, na, 1)
    wu = mr.weights(ta, "full", k, na, 2)
    wb = mr.weights(tb, "full", na, nb, 3)
    ab, ob = mr.decode(tb, wb, na, nb, family=fam_b)
    nw = (1 + 0.2 * rng.standard_normal(k)).astype(np.float32)
    nnw = (1 + 0.2 * rng.standard_normal(na)).astype(np.float32)
    bias = rng.standard_normal(na).astype(np.float32)
    res = (3 * rng.standard_normal(na)).astype(np.float32)
    for ci, (epi, xq_next) in enumerate([("store", 0), ("store", 1), ("store+bias", 2), ("resid", 2), ("resid+bias", 1),
                                         ("swiglu", 1), ("swiglu", 0)]):
        x = mr.activation(mr.ACT_KINDS[ci % 6], k, ci)
        kw = dict(norm_w=nw, eps=EPS, xq_next=xq_next, next_nw=nnw if xq_next == 2 else None)
        if epi == "swiglu":
            kw["w_a_up"] = wu
        if "bias" in epi:
            kw["bias_a"] = bias
        if epi.startswith("resid"):
            kw["resid"] = res
        oa, ob1, ob2, used = gpu.op_linear_chain(mr.TYPE[ta], wa, k, na, x, mr.TYPE[tb], wb, nb, **kw)
        oa2, ob1b, _, _ = gpu.op_linear_chain(mr.TYPE[ta], wa, k, na, x, mr.TYPE[tb], wb, nb, **kw)
        path = "%s%s %s %s" % (tag, fam_a, ta, epi)
        W.expect(np.array_equal(oa.view(np.uint32), oa2.view(np.uint32)) and np.array_equal(ob1.view(np.uint32), ob1b.view(np.uint32)),
                 "%s: not deterministic" % path)
        y, e = _ref(ta, wa, k, na, x, fam_a, nw=nw, bias=kw.get("bias_a"))
        if epi == "swiglu":
            u, eu = _ref(ta, wu, k, na, x, fam_a, nw=nw)
            y, e = mr.swiglu(y, e, u, eu)
        elif epi.startswith("resid"):
            y, e = mr.resid(y, e, res)
        W.check(path, oa, y, e, "xq_next=%d" % xq_next)
        # B reads A's f32 output exactly as the kernel left it
        yb, eb = mr.matvec(ab, ob, oa, nw=nnw if xq_next == 2 else None, eps=EPS, family=fam_b)
        W.check("%s%s %s fed by %s %s" % (tag, fam_b, tb, fam_a, epi), ob1, yb, eb, "xq_next=%d" % xq_next)
        W.check("%s%s %s fed by xq_quantize" % (tag, fam_b, tb), ob2, yb, eb, "xq_next=%d" % xq_next)
        if xq_next and fam_b == "mfma" and na % 16 == 0:
            W.expect(used, "%s xq_next=%d: A left no XQ image" % (path, xq_next))
        W.expect(np.array_equal(ob1.view(np.uint32), ob2.view(np.uint32)),
                 "%s xq_next=%d: B from A's image differs from B from xq_quantize (max %.3g)" % (path, xq_next, np.abs(ob1 - ob2).max()))
    W.done()


# ---- fused QKV with RoPE and the cache writes
QKV_CASES = [
    # (types, hidden, head_dim, n_heads, n_kv)
    (("Q4_K", "Q4_K", "Q6_K"), 4096, 128, 32, 8),
    (("Q5_K", "Q5_K", "Q6_K"), 4096, 128, 32, 8),
    (("Q8_0", "Q8_0", "Q8_0"), 4096, 128, 32, 8),
    (("Q4_K", "Q4_K", "Q6_K"), 2048, 64, 32, 4),
    (("Q5_K", "Q5_K", "Q6_K"), 2048, 64, 32, 4),
    (("Q8_0", "Q8_0", "Q8_0"), 2048, 64, 32, 4),
    (("Q8_0", "Q8_0", "Q8_0"), 896, 64, 14, 2),     # VALU: RoPE and cache epilogues on mv_kernel
    (("Q4_0", "Q4_0", "Q4_0"), 896, 64, 14, 2),
]


@pytest.mark.parametrize("types,hidden,hd,nh,nkv", QKV_CASES)
def test_fused_qkv_rope(gpu, pkg, orc, types, hidden, hd, nh, nkv):
    qkv_case(gpu, orc, types, hidden, hd, nh, nkv)


def qkv_case(gpu, orc, types, hidden, hd, nh, nkv, tag=""):
    """The fused QKV launch with and without biases at pos 0, 1 and last; `tag` leads every WORST line."""
    W = Worst()
    max_seq, base, scale = 40, 500000.0, 1.0
    fam = mr.kernel_family(types[0], hidden)
    rng = np.random.default_rng(hidden + nh)
    rows = (nh * hd, nkv * hd, nkv * hd)
    ws = [mr.weights(types[s], "full", hidden, rows[s], 10 + s) for s in range(3)]
    nw = (1 + 0.2 * rng.standard_normal(hidden)).astype(np.float32)
    for with_bias in (False, True):
        biases = [rng.standard_normal(r).astype(np.float32) if with_bias else None for r in rows]
        for pi, pos in enumerate((0, 1, max_seq - 1)):
            x = mr.activation(mr.ACT_KINDS[pi * 2 + with_bias], hidden, pos + 7)
            kc = np.full((nkv, max_seq, hd), NAN_BITS, np.uint32).view(np.float32)
            vc = kc.copy()
            q, k2, v2 = gpu.op_qkv_rope([mr.TYPE[t] for t in types], ws, biases, x, nw, EPS, hd, nh, nkv, kc, vc, pos, base, scale)
            q_b, k2b, v2b = gpu.op_qkv_rope([mr.TYPE[t] for t in types], ws, biases, x, nw, EPS, hd, nh, nkv, kc, vc, pos, base, scale)
            what = "%s/%s/%s %d%s" % (types + (hidden, " bias" if with_bias else ""))
            W.expect(all(np.array_equal(p.view(np.uint32), r.view(np.uint32)) for p, r in ((q, q_b), (k2, k2b), (v2, v2b))),
                     "%s pos %d: not deterministic" % (what, pos))
            c, s = mr.rope_cs(orc, pos, hd, base, scale)
            refs = [_ref(types[i], ws[i], hidden, rows[i], x, fam, nw=nw, bias=biases[i]) for i in range(3)]
            yq, eq = mr.rope(*refs[0], c, s, hd)
            yk, ek = mr.rope(*refs[1], c, s, hd)
            W.check("%s%s qkv ROPE_Q %s" % (tag, fam, what), q, yq, eq, "pos %d" % pos)
            W.check("%s%s qkv ROPE_K %s" % (tag, fam, what), k2[:, pos, :].reshape(-1), yk, ek, "pos %d" % pos)
            W.check("%s%s qkv V_CACHE %s" % (tag, fam, what), v2[:, pos, :].reshape(-1), refs[2][0], refs[2][1], "pos %d" % pos)
            others = np.ones(max_seq, bool)
            others[pos] = False
            W.expect(np.all(k2[:, others].view(np.uint32) == NAN_BITS) and np.all(v2[:, others].view(np.uint32) == NAN_BITS),
                     "%s pos %d: a cache row other than pos changed" % (what, pos))
    W.done()


# ---- MoE: MOE_SWIGLU (2 and 4 passes) and MOE_DOWN (first / middle / last group), device router
def _moe_ref(tg, gate, up, td, down, E, H, F, x, nw, sel, w):
    fam_g, fam_d = mr.kernel_family(tg, H), mr.kernel_family(td, F)
    gb, db = gate.size // E, down.size // E
    ys, es = [], []
    for e in sel:
        g, eg = _ref(tg, gate[e * gb:(e + 1) * gb], H, F, x, fam_g, nw=nw)
        u, eu = _ref(tg, up[e * gb:(e + 1) * gb], H, F, x, fam_g, nw=nw)
        act, eact = mr.swiglu(g, eg, u, eu)
        y, ey = _ref(td, down[e * db:(e + 1) * db], F, H, act, fam_d, xerr=eact)
        ys.append(y)
        es.append(ey)
    return mr.moe_down(ys, es, w, x)


MOE_CASES = [
    # (gate/up type, down type, experts, hidden, ffn)
    ("Q4_K", "Q6_K", 8, 1024, 512),
    ("Q8_0", "Q8_0", 6, 512, 256),
    ("Q8_0", "Q8_0", 6, 896, 320),      # gate / up on mv_kernel
]


@pytest.mark.parametrize("tg,td,E,H,F", MOE_CASES)
def test_moe_experts(gpu, pkg, orc, tg, td, E, H, F):
    W = Worst()
    rng = np.random.default_rng(E + H)
    gate, up = mr.weights(tg, "full", H, F * E, 1), mr.weights(tg, "full", H, F * E, 2)
    down = mr.weights(td, "full", F, H * E, 3)
    nw = (1 + 0.2 * rng.standard_normal(H)).astype(np.float32)
    for topk in (1, 2, 3, 4, 5):
        sel = rng.permutation(np.arange(2, E))[:topk].astype(np.int32) if topk <= E - 2 else rng.permutation(E)[:topk].astype(np.int32)
        w = rng.dirichlet(np.ones(topk)).astype(np.float32)
        x = mr.activation(mr.ACT_KINDS[topk % 6], H, topk)
        got, s_used, w_used = gpu.op_moe_experts(mr.TYPE[tg], gate, up, mr.TYPE[td], down, E, H, F, topk, x, nw, EPS, sel=sel, sel_w=w)
        got2, _, _ = gpu.op_moe_experts(mr.TYPE[tg], gate, up, mr.TYPE[td], down, E, H, F, topk, x, nw, EPS, sel=sel, sel_w=w)
        W.expect(np.array_equal(got.view(np.uint32), got2.view(np.uint32)), "moe %s top-%d: not deterministic" % (tg, topk))
        W.expect(np.array_equal(s_used, sel) and np.array_equal(w_used, w), "moe top-%d: selection not used as given" % topk)
        y, e = _moe_ref(tg, gate, up, td, down, E, H, F, x, nw, sel, w)
        W.check("moe %s/%s top-%d" % (tg, td, topk), got, y, e, "sel %s" % list(sel))
    # the device router: selection, tie order, weights
    wr = (0.05 * rng.standard_normal((E, H))).astype(np.float32)
    wr[3] = wr[1]                                  # experts 1 and 3 tie exactly
    for topk in (1, 2, 4):
        for trial in range(3):
            x = mr.activation("normal", H, 50 + trial)
            if trial == 0:                         # make the tied pair the top two
                xn = x.astype(np.float64) * mr.inv_rms(x, EPS) * nw
                wr_t = wr.copy()
                wr_t[[1, 3]] += (40.0 * np.sign(xn) / H).astype(np.float32)
            else:
                wr_t = wr
            got, s_used, w_used = gpu.op_moe_experts(mr.TYPE[tg], gate, up, mr.TYPE[td], down, E, H, F, topk, x, nw, EPS, router=wr_t)
            sel, wref, logits, lerr = mr.router(x, nw, EPS, wr_t, topk)
            srt = np.sort(logits)[::-1]
            gap_ok = topk >= E or srt[topk - 1] - srt[topk] > 2 * lerr.max()
            if gap_ok:
                W.expect(np.array_equal(s_used, sel), "router top-%d trial %d: selected %s, float64 %s" % (topk, trial, list(s_used), list(sel)))
                W.check("router weights top-%d" % topk, w_used, wref, 8 * mr.U + 2 * lerr.max() + 0 * wref)
            if trial == 0 and topk >= 2:
                W.expect(list(s_used[:2]) == [1, 3], "router tie: selected %s, want [1, 3] first" % list(s_used))
            y, e = _moe_ref(tg, gate, up, td, down, E, H, F, x, nw, s_used, w_used)
            W.check("moe %s/%s device router" % (tg, td), got, y, e, "top-%d" % topk)
    W.done()
