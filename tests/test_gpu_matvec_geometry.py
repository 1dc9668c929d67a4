"""The single-sequence matrix-core mat-vec at every workgroup geometry its planner emits (tests/matvec_ref.py: mvq_geometry), launch
by launch against the float64 restatement and the bound of tests/matvec_ref.py — no new tolerance.

tests/test_gpu_matvec.py runs k = 256, 2048, 4096, 5632, 14336 and 28672: one k-slice and eight row groups, eight even slices, eight
uneven slices that all have a block.  Here: 2, 3 and 4 slices with 4 and 2 row groups, 5, 6 and 7 slices (320, 384 and 448-thread
workgroups), eight uneven slices with one, two and three waves that have no block, several tiles per row group, a workgroup's
tiles capped at one row per thread (more workgroups than CUs), and the partial counts k / 16 of the norm prologue's gather below 64
and above 256.  One pytest case per class; the classes whole models already run come first, the ones nothing ran last.  Every case
prints `WORST <class> ...`, checks that two runs give the same bits and collects its failures before asserting.

The shape lists and the inputs are functions of this module: tests/test_matvec_geometry_ref.py (no GPU) checks that the lists cover
every class and that results wrong in the ways a geometry goes wrong exceed the bound on these very inputs."""
import numpy as np
import pytest

import matvec_multi_ref as mm
import matvec_ref as mr
from test_gpu_matvec import EPS, Worst, _ref, chain_case, qkv_case

pytestmark = pytest.mark.gpu

# (class, k): the smallest k of the class first, then deeper slices.  Order: classes test_gpu_matvec.py also runs; classes that ran
# only inside whole models; classes nothing ran.
PLAIN = [
    ("(1,8)", (256,)),
    ("(8,1) even", (2048,)),
    ("(8,1) uneven busy", (5632, 18944)),
    ("(2,4)", (512,)),
    ("(3,2)", (768,)),
    ("(4,2)", (1024,)),
    ("(6,1)", (1536, 13824)),
    ("(8,1) uneven idle2", (2816,)),
    ("(5,1)", (1280, 2560, 5120)),
    ("(7,1)", (1792, 3584, 7168)),
    ("(8,1) uneven idle1", (3328,)),
    ("(8,1) uneven idle3", (2304,)),
]
PLAIN_N = (1, 17, 130)


def plain_items(ci: int, ks):
    """The launches of class number ci: (format, k, n, activation kind, seed).  Every format at the smallest k, one (rotating) at the
    others; the activation kinds rotate, and all six run at (smallest k, n = 17) in the class's own format."""
    items, i = [], ci
    for ki, k in enumerate(ks):
        for n in PLAIN_N:
            for tname in mr.FUSED if ki == 0 else (mr.FUSED[(ci + ki) % len(mr.FUSED)],):
                every = ki == 0 and n == 17 and tname == mr.FUSED[ci % len(mr.FUSED)]
                for act in mr.ACT_KINDS if every else (mr.ACT_KINDS[i % len(mr.ACT_KINDS)],):
                    i += 1
                    items.append((tname, k, n, act, 7000 + 100 * i + ci))
    return items


def norm_weight(k: int, seed: int) -> np.ndarray:
    return (1 + 0.2 * np.random.default_rng(seed).standard_normal(k)).astype(np.float32)


def plain_inputs(item):
    """(raw, x, nw) of one plain_items entry."""
    tname, k, n, act, seed = item
    return mr.weights(tname, "full", k, n, seed), mr.activation(act, k, seed + 1), norm_weight(k, seed + 2)


@pytest.mark.parametrize("ci", range(len(PLAIN)), ids=[c for c, _ in PLAIN])
def test_plain_and_norm(gpu, pkg, orc, ci):
    cls, ks = PLAIN[ci]
    W = Worst()
    for item in plain_items(ci, ks):
        tname, k, n, act, _ = item
        assert mr.mvq_class(k) == cls
        raw, x, nw = plain_inputs(item)
        t = mr.TYPE[tname]
        what = "%s k=%d n=%d %s" % (tname, k, n, act)
        got, got2 = gpu.op_vec_mat(t, raw, x, n), gpu.op_vec_mat(t, raw, x, n)
        y, e = _ref(tname, raw, k, n, x, "mfma")
        W.check("%s plain" % cls, got, y, e, what)
        gotn, gotn2 = gpu.op_norm_vec_mat(t, raw, x, nw, EPS, n), gpu.op_norm_vec_mat(t, raw, x, nw, EPS, n)
        y, e = _ref(tname, raw, k, n, x, "mfma", nw=nw)
        W.check("%s norm" % cls, gotn, y, e, what)
        W.expect(np.array_equal(got.view(np.uint32), got2.view(np.uint32)) and np.array_equal(gotn.view(np.uint32), gotn2.view(np.uint32)),
                 "%s %s: not deterministic" % (cls, what))
    W.done()


# ---- wide launches: several tiles per row group, a short last workgroup, a ragged last tile, R capped at rmax
WIDE = [
    # (class, k, n, Rg, R, n_wg, tiles of the last workgroup)
    ("(2,4) Rg=2", 512, 16400, 2, 8, 129, 1),
    ("(3,2) Rg=2", 768, 8208, 2, 4, 129, 1),
    ("(4,2) Rg=2", 1024, 8208, 2, 4, 129, 1),
    ("(5,1) Rg=2", 1280, 4113, 2, 2, 129, 2),            # an odd number of waves; the last tile has one row
    ("(7,1) Rg=2", 1792, 4113, 2, 2, 129, 2),
    ("(5,1) Rg=2 short last", 1280, 4097, 2, 2, 129, 1),   # ... and the last workgroup one tile
    ("(7,1) Rg=2 short last", 1792, 4097, 2, 2, 129, 1),
    ("(5,1) R=rmax", 1280, 81936, 20, 20, 257, 1),       # more workgroups than CUs
    ("(1,8) R=rmax", 256, 151936, 4, 32, 297, 24),
]
WIDE_FMT = "Q4_K"


def wide_rows(k: int, n: int) -> np.ndarray:
    """matvec_multi_ref.sample_rows plus the first and the last tile of the last two workgroups."""
    g = mr.mvq_geometry(k, n)
    tiles = -(-n // 16)
    edge = []
    for wg in (g["n_wg"] - 2, g["n_wg"] - 1):
        for tile in (wg * g["R"], min(wg * g["R"] + g["R"], tiles) - 1):
            edge.append(np.arange(16 * tile, min(16 * tile + 16, n)))
    return np.unique(np.concatenate([mm.sample_rows(n, 192, k)] + edge))


def wide_inputs(k: int, n: int):
    return mr.weights(WIDE_FMT, "full", k, n, k + n), mr.activation("outlier", k, k + n + 1), norm_weight(k, k + n + 2)


@pytest.mark.parametrize("cls,k,n,Rg,R,n_wg,last", WIDE, ids=[w[0] for w in WIDE])
def test_wide(gpu, pkg, orc, cls, k, n, Rg, R, n_wg, last):
    g = mr.mvq_geometry(k, n)
    assert (g["Rg"], g["R"], g["n_wg"], g["last"]) == (Rg, R, n_wg, last) and cls.startswith("(%d,%d)" % (g["T"], g["G"]))
    W = Worst()
    raw, x, nw = wide_inputs(k, n)
    rows = wide_rows(k, n)
    t = mr.TYPE[WIDE_FMT]
    for path, w in (("plain", None), ("norm", nw)):
        run = (lambda: gpu.op_vec_mat(t, raw, x, n)) if w is None else (lambda: gpu.op_norm_vec_mat(t, raw, x, w, EPS, n))
        got, got2 = run(), run()
        Y, E = mm.linear(WIDE_FMT, raw, k, n, x[None], nw=w, rows=rows, eps=EPS)
        W.check("%s wide %s" % (cls, path), got[rows], Y[0], E[0], "k=%d n=%d" % (k, n))
        W.expect(np.all(np.isfinite(got)), "%s %s: a row outside the sample is not finite" % (cls, path))
        W.expect(np.array_equal(got.view(np.uint32), got2.view(np.uint32)), "%s %s: not deterministic" % (cls, path))
    W.done()


# ---- epilogues and the XQ hand-off: A [na, k] feeding B [nb, na]
CHAIN = [
    # (type A, k, n_a, type B, n_b): classes of A > B
    ("Q4_K", 1280, 1792, "Q5_K", 48),      # (5,1) > (7,1)
    ("Q6_K", 1792, 2304, "Q8_0", 40),      # (7,1) > idle3
    ("Q5_K", 768, 3328, "Q4_0", 32),       # (3,2) > idle1
    ("Q8_0", 3584, 2560, "Q6_K", 64),      # (7,1) > (5,1)
]


@pytest.mark.parametrize("ta,k,na,tb,nb", CHAIN, ids=["%d-%d" % (c[1], c[2]) for c in CHAIN])
def test_epilogues_and_xq_chain(gpu, pkg, orc, ta, k, na, tb, nb):
    chain_case(gpu, ta, k, na, tb, nb, tag="%s > %s: " % (mr.mvq_class(k), mr.mvq_class(na)))


# ---- fused QKV with RoPE and the cache rows
QKV = [
    # (hidden, head_dim, n_heads, n_kv)
    (1792, 128, 14, 2),
    (1280, 128, 10, 10),
    (3328, 64, 8, 2),
    (768, 128, 6, 2),        # two and four row groups in a fused launch: a segment's tiles per row group come from its own rows
    (512, 64, 8, 2),
]
QKV_MIXES = (("Q4_K", "Q4_K", "Q6_K"), ("Q8_0", "Q8_0", "Q8_0"))


@pytest.mark.parametrize("types", QKV_MIXES, ids=["Q4_K-Q4_K-Q6_K", "Q8_0"])
@pytest.mark.parametrize("hidden,hd,nh,nkv", QKV, ids=[str(q[0]) for q in QKV])
def test_fused_qkv_rope(gpu, pkg, orc, types, hidden, hd, nh, nkv):
    qkv_case(gpu, orc, types, hidden, hd, nh, nkv, tag="%s: " % mr.mvq_class(hidden))


# ---- MoE: gate / up at k = H, down at k = F
MOE = [
    # (gate/up type, down type, experts, hidden, ffn)
    ("Q8_0", "Q8_0", 4, 768, 1280),        # (3,2) and (5,1)
    ("Q4_K", "Q6_K", 4, 1792, 2304),       # (7,1) and idle3
]


@pytest.mark.parametrize("tg,td,E,H,F", MOE, ids=["%d-%d" % (m[3], m[4]) for m in MOE])
def test_moe_experts(gpu, pkg, orc, tg, td, E, H, F):
    W = Worst()
    cls = "%s / %s" % (mr.mvq_class(H), mr.mvq_class(F))
    rng = np.random.default_rng(E + H)
    gate, up = mr.weights(tg, "full", H, F * E, 1), mr.weights(tg, "full", H, F * E, 2)
    down = mr.weights(td, "full", F, H * E, 3)
    ex = mm.Experts(tg, gate, up, td, down, E, H, F)
    nw = norm_weight(H, H)
    wr = (0.05 * rng.standard_normal((E, H))).astype(np.float32)
    args = (mr.TYPE[tg], gate, up, mr.TYPE[td], down, E, H, F)
    for topk in (1, 2, 3):
        x = mr.activation(mr.ACT_KINDS[topk % 6], H, topk)
        sel = rng.permutation(E)[:topk].astype(np.int32)
        w = rng.dirichlet(np.ones(topk)).astype(np.float32)
        for how, kw in (("given", dict(sel=sel, sel_w=w)), ("router", dict(router=wr))):
            got, s_used, w_used = gpu.op_moe_experts(*args, topk, x, nw, EPS, **kw)
            got2, s2, w2 = gpu.op_moe_experts(*args, topk, x, nw, EPS, **kw)
            what = "moe %s top-%d %s" % (cls, topk, how)
            W.expect(np.array_equal(got.view(np.uint32), got2.view(np.uint32)) and np.array_equal(s_used, s2), what + ": not deterministic")
            if how == "given":
                W.expect(np.array_equal(s_used, sel) and np.array_equal(w_used, w), what + ": selection not used as given")
            else:
                rsel, rw, logits, lerr = mr.router(x, nw, EPS, wr, topk)
                srt = np.sort(logits)[::-1]
                if srt[topk - 1] - srt[topk] > 2 * lerr.max():
                    W.expect(np.array_equal(s_used, rsel), what + ": selected %s, float64 %s" % (list(s_used), list(rsel)))
            y, e = mm.moe(ex, x, [x] * topk, nw, s_used, w_used, eps=EPS)
            W.check("%s moe %s/%s %s" % (cls, tg, td, how), got, y, e, "top-%d sel %s" % (topk, list(s_used)))
    W.done()
