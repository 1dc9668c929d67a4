"""Every multi-sequence mat-vec launch (matvec_batch.hip: mvqb, mvqb2 split / SEQ and their epilogue; the grouped MoE kernels of
misc.hip) through the step's own assembly (launch_mvb -> build_mv_group -> mvqb_launch) on the engine's own batch scratch.

Each launch is checked three ways: (i) per sequence against the float64 restatement within matvec_ref's bound, (ii) bit for bit
against the single-sequence entry point on the same vector (outputs, XQ image bytes, sums of squares), (iii) a second call gives the
same bits.  Where a launch leaves an XQ image, its elements, chunk sums and sums of squares are also held to float64 of the launch's
own f32 output (matvec_multi_ref.image_ref).  The scratch is poisoned first (0x7FC0BEEF), so rows of sequences the call does not have, rows past n and cache rows other
than (slot[s], pos[s]) must still hold the pattern.  tests/test_matvec_multi_ref.py shows on the CPU, on the inputs used here, that
these checks catch the ways such a kernel goes wrong.  Each test prints `WORST <path>: err / bound`."""
import numpy as np
import pytest

import matvec_multi_ref as mm
import matvec_ref as mr
from test_gpu_matvec import Worst
from test_gpu_prefill_ref import MOE_FORMATS

pytestmark = pytest.mark.gpu

EPS = 1e-5
SPLIT, SEQ, MVQB = "mvqb2 split", "mvqb2 seq", "mvqb"


def _bits(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(_bits(a), _bits(b)))


def _records(img):
    """(payload, tail) of XQ images: a 1280-byte record holds 1152 bytes the producers write (limbs, chunk sums, chunk scales); no
    kernel writes or reads the last 128, so there a poisoned image keeps the pattern."""
    rec = np.ascontiguousarray(img).reshape(-1, 1280)
    return np.ascontiguousarray(rec[:, :1152]), np.ascontiguousarray(rec[:, 1152:])


def _same_image(a, b):
    return _same(_records(a)[0], _records(b)[0])


def _check_image(W, path, image, ssq, out, nw, what):
    """An image (and sums of squares) against float64 of the launch's own f32 output: independent of any GPU converter."""
    x, xs = mm.xq_decode(image, out.size)
    (v, ev), (sums, es), (sq, eq) = mm.image_ref(out, nw)
    W.check(path, x, v, ev, what + " elements")
    W.check(path, xs, sums, es, what + " chunk sums")
    if ssq is not None:
        W.check(path, ssq, sq, eq, what + " sums of squares")


def _norm_w(k, seed):
    return (1 + 0.2 * np.random.default_rng(seed).standard_normal(k)).astype(np.float32)


class Linear:
    """One launch shape with its weights, 16 sequences' inputs, the float64 reference and the single-sequence results, computed once
    and shared by the sequence counts of a test."""

    def __init__(self, gpu, tname, k, n, *, role="store", xq_next=0, seed=0, norm=True, bias=False, n_rows=192):
        rng = np.random.default_rng(seed + k + n)
        self.gpu, self.tname, self.t, self.k, self.n, self.role, self.xq_next = gpu, tname, mr.TYPE[tname], k, n, role, xq_next
        self.raw = mr.weights(tname, "full", k, n, seed + 1)
        self.raw_up = mr.weights(tname, "full", k, n, seed + 2) if role == "swiglu" else None
        self.X = mm.activations(k, 16, seed + 3)
        self.nw = _norm_w(k, seed + 4) if norm else None
        self.bias = rng.standard_normal(n).astype(np.float32) if bias else None
        self.resid = (3 * rng.standard_normal((16, n))).astype(np.float32) if role == "resid" else None
        self.next_nw = _norm_w(n, seed + 5) if xq_next == 2 else None
        self.rows = mm.sample_rows(n, n_rows, seed)
        Y, E = mm.linear(tname, self.raw, k, n, self.X, nw=self.nw, bias=self.bias, rows=self.rows, eps=EPS)
        if role == "swiglu":
            U, EU = mm.linear(tname, self.raw_up, k, n, self.X, nw=self.nw, rows=self.rows, eps=EPS)
            Y, E = mr.swiglu(Y, E, U, EU)
        elif role == "resid":
            Y, E = mr.resid(Y, E, self.resid[:, self.rows])
        self.Y, self.E = Y, E
        self.single = {}

    def kw(self, s=None):
        rs = None if self.resid is None else (self.resid[s] if s is not None else None)
        return dict(w_up=self.raw_up, bias=self.bias, norm_w=self.nw, eps=EPS, resid=rs, xq_next=self.xq_next, next_nw=self.next_nw)

    def one(self, s):
        if s not in self.single:
            self.single[s] = self.gpu.op_linear_image(self.t, self.raw, self.k, self.n, self.X[s], **self.kw(s))
        return self.single[s]

    def check(self, W, n_seq, max_batch, structure, path):
        kw = self.kw()
        kw["resid"] = None if self.resid is None else self.resid[:n_seq]
        r = self.gpu.op_linear_multi(self.t, self.raw, self.k, self.n, self.X[:n_seq], max_batch=max_batch, **kw)
        r2 = self.gpu.op_linear_multi(self.t, self.raw, self.k, self.n, self.X[:n_seq], max_batch=max_batch, **kw)
        tag = "%s k=%d n=%d B=%d" % (path, self.k, self.n, n_seq)
        W.expect(r["structure"] == structure, "%s: ran as %s %s, want %s" % (tag, r["structure"], r["counts"], structure))
        W.expect(all(_same(r[f], r2[f]) for f in ("out", "image", "ssq")), "%s: a second call gives other bits" % tag)
        W.expect(r["used"] == (self.xq_next != 0), "%s: image left = %s" % (tag, r["used"]))
        for s in range(n_seq):
            W.check(path, r["out"][s][self.rows], self.Y[s], self.E[s], "k=%d n=%d B=%d sequence %d" % (self.k, self.n, n_seq, s))
            o = self.one(s)
            W.expect(_same(r["out"][s], o["out"]), "%s sequence %d: output differs from the single-sequence launch (max %.3g)"
                     % (tag, s, float(np.abs(r["out"][s] - o["out"]).max())))
            if self.xq_next:
                W.expect(_same_image(r["image"][s], o["image"]), "%s sequence %d: XQ image differs from the single-sequence launch" % (tag, s))
                W.expect(mm.poisoned(_records(r["image"][s])[1].view(np.float32)).all(), "%s sequence %d: the records' unused tail was written" % (tag, s))
            if self.xq_next == 2:
                W.expect(_same(r["ssq"][s], o["ssq"]), "%s sequence %d: sums of squares differ from the single-sequence launch" % (tag, s))
            if self.xq_next:
                _check_image(W, path + " image", r["image"][s], r["ssq"][s] if self.xq_next == 2 else None, r["out"][s], self.next_nw,
                             "B=%d sequence %d" % (n_seq, s))
        W.expect(mm.poisoned(r["out"][n_seq:]).all(), "%s: output rows of sequences the call does not have changed" % tag)
        W.expect(mm.poisoned(r["pad"]).all(), "%s: floats past row n of a sequence changed" % tag)
        if r["image"] is not None:
            W.expect(mm.poisoned(r["image"][n_seq:].view(np.float32)).all() and mm.poisoned(r["ssq"][n_seq:]).all(),
                     "%s: image / sums of squares of sequences the call does not have changed" % tag)
            if self.xq_next != 2:
                W.expect(mm.poisoned(r["ssq"]).all(), "%s: sums of squares written without norm weights" % tag)
            if not self.xq_next:
                W.expect(mm.poisoned(r["image"].view(np.float32)).all(), "%s: image written unasked" % tag)


# ---- formats x sequence counts: k = 1024 (T = 4, G = 2), n = 272
@pytest.mark.parametrize("tname", mr.FUSED)
def test_formats_and_sequence_counts(gpu, tname):
    W = Worst()
    L = Linear(gpu, tname, 1024, 272, seed=100)
    for n_seq in (1, 2, 3, 4, 5, 8, 9, 16):
        L.check(W, n_seq, 16, MVQB if n_seq == 1 else SPLIT, "multi %s store" % tname)
    W.done()


# ---- k geometry: one slice (SEQ), two, empty slices, a short last slice, several chunks per slice
@pytest.mark.parametrize("tname", ["Q4_K", "Q6_K"])
@pytest.mark.parametrize("k,n", [(256, 48), (512, 64), (2816, 272), (5632, 96), (14336, 48)])
def test_k_geometry(gpu, tname, k, n):
    W = Worst()
    L = Linear(gpu, tname, k, n, seed=200)
    for n_seq in (3, 16):
        L.check(W, n_seq, 16, SEQ if k == 256 else SPLIT, "multi %s k-slices" % tname)
    W.done()


# ---- the SEQ grid with more than one slice: >= 160 workgroups of units
@pytest.mark.parametrize("k", [512, 2816])
def test_seq_grid_gate_up(gpu, k):
    W = Worst()
    L = Linear(gpu, "Q4_K", k, 10240, role="swiglu", xq_next=1, seed=300)
    for n_seq in (5, 16):
        L.check(W, n_seq, 16, SEQ, "multi Q4_K swiglu SEQ")
    W.done()


# ---- the output projection of a vocabulary that is no multiple of 16: the ragged last tile on both grids
@pytest.mark.parametrize("k,n,structure", [(1024, 130, SPLIT), (512, 20500, SEQ)])
def test_ragged_rows(gpu, k, n, structure):
    W = Worst()
    L = Linear(gpu, "Q6_K", k, n, seed=400)
    for n_seq in (5, 15, 16):             # (a store's rows lie whole tiles apart: what a sequence writes past row n lands in floats of nobody)
        L.check(W, n_seq, 16, structure, "multi Q6_K ragged store")
    W.done()


# ---- the epilogues as the step makes them
EPILOGUES = [
    # (name, type, k, n, role, xq_next, bias)
    ("wo", "Q4_K", 1024, 512, "resid", 2, True),
    ("down", "Q6_K", 2816, 512, "resid", 2, False),
    ("gate|up", "Q4_K", 512, 1024, "swiglu", 1, False),
    ("gate|up Q5_K", "Q5_K", 1024, 256, "swiglu", 1, False),
    ("down Q8_0", "Q8_0", 1024, 256, "resid", 2, False),
    ("wo Q4_0", "Q4_0", 512, 512, "resid", 2, True),
]


@pytest.mark.parametrize("name,tname,k,n,role,xq_next,bias", EPILOGUES)
def test_epilogues(gpu, name, tname, k, n, role, xq_next, bias):
    W = Worst()
    L = Linear(gpu, tname, k, n, role=role, xq_next=xq_next, seed=500, norm=role == "swiglu", bias=bias)
    for n_seq, max_batch in ((3, 4), (16, 16)):
        L.check(W, n_seq, max_batch, SPLIT, "multi %s %s" % (tname, name))
    W.done()


CHAINS = [
    # (A type, k, n_a, A role, xq_next, B type, n_b)
    ("Q4_K", 512, 1024, "swiglu", 1, "Q6_K", 48),
    ("Q6_K", 1024, 512, "resid", 2, "Q6_K", 130),
    ("Q8_0", 512, 512, "resid", 2, "Q8_0", 64),
]


@pytest.mark.parametrize("ta,k,na,role,xq_next,tb,nb", CHAINS)
def test_xq_chain(gpu, ta, k, na, role, xq_next, tb, nb):
    """B from the images A's epilogue left equals B after a fresh conversion of A's output, for every sequence, bitwise."""
    W = Worst()
    A = Linear(gpu, ta, k, na, role=role, xq_next=xq_next, seed=600, norm=role == "swiglu")
    wb = mr.weights(tb, "full", na, nb, 7)
    ab, ob = mr.decode(tb, wb, na, nb)
    bnw = A.next_nw if xq_next == 2 else None
    for n_seq in (3, 16):
        kw = A.kw()
        kw["resid"] = None if A.resid is None else A.resid[:n_seq]
        args = (A.t, A.raw, k, na, A.X[:n_seq], mr.TYPE[tb], wb, nb)
        kw = dict(w_a_up=kw["w_up"], bias_a=kw["bias"], norm_w=kw["norm_w"], eps=EPS, resid=kw["resid"], xq_next=xq_next, next_nw=kw["next_nw"])
        oa, ob1, ob2, used = gpu.op_linear_chain_multi(*args, **kw)
        oa_b, ob1_b, _, _ = gpu.op_linear_chain_multi(*args, **kw)
        tag = "chain %s %s -> %s B=%d" % (ta, role, tb, n_seq)
        W.expect(used, "%s: A left no images" % tag)
        W.expect(_same(oa, oa_b) and _same(ob1, ob1_b), "%s: a second call gives other bits" % tag)
        W.expect(_same(ob1, ob2), "%s: B from A's images differs from B after re-quantization (max %.3g)" % (tag, float(np.abs(ob1 - ob2).max())))
        for s in range(n_seq):
            W.check("multi chain A %s %s" % (ta, role), oa[s][A.rows], A.Y[s], A.E[s], "B=%d sequence %d" % (n_seq, s))
            yb, eb = mr.matvec(ab, ob, oa[s], nw=bnw, eps=EPS, family="mfma")     # B reads A's f32 output as the kernel left it
            W.check("multi chain B %s fed by %s" % (tb, role), ob1[s], yb, eb, "B=%d sequence %d" % (n_seq, s))
            kws = dict(kw, resid=None if A.resid is None else A.resid[s])
            sa, sb, _, _ = gpu.op_linear_chain(A.t, A.raw, k, na, A.X[s], mr.TYPE[tb], wb, nb, **kws)
            W.expect(_same(oa[s], sa) and _same(ob1[s], sb), "%s sequence %d: differs from the single-sequence chain" % (tag, s))
    W.done()


# ---- fused QKV: RoPE at every sequence's own position, K / V rows into its own cache slot
QKV_SHAPES = [(hd, 8, nkv, hidden) for hd in (64, 128) for nkv in (2, 8) for hidden in (512, 1024)]   # head_dim, heads, kv heads, hidden
QKV_MIXES = [("Q4_K", "Q4_K", "Q6_K"), ("Q5_K", "Q5_K", "Q6_K"), ("Q8_0", "Q8_0", "Q8_0"), ("Q4_K", "Q8_0", "Q4_0")]
MAX_SEQ, ROPE_BASE, ROPE_SCALE = 40, 500000.0, 1.0


class Qkv:
    def __init__(self, orc, types, hd, nh, nkv, hidden, with_bias):
        rng = np.random.default_rng(hidden + hd + nkv)
        self.types, self.hd, self.nh, self.nkv, self.hidden = types, hd, nh, nkv, hidden
        self.rows = (nh * hd, nkv * hd, nkv * hd)
        self.ws = [mr.weights(types[i], "full", hidden, self.rows[i], 10 + i) for i in range(3)]
        self.nw = _norm_w(hidden, 5)
        self.biases = [rng.standard_normal(r).astype(np.float32) if with_bias else None for r in self.rows]
        self.X = mm.activations(hidden, 16, 900)
        self.pos = mm.positions(16, MAX_SEQ)
        refs = [mm.linear(types[i], self.ws[i], hidden, self.rows[i], self.X, nw=self.nw, bias=self.biases[i], eps=EPS) for i in range(3)]
        self.pre = refs                                            # (before RoPE: what the CPU mutation tests rotate wrongly)
        self.q = mm.rope_rows(orc, *refs[0], self.pos, hd, ROPE_BASE, ROPE_SCALE)
        self.k = mm.rope_rows(orc, *refs[1], self.pos, hd, ROPE_BASE, ROPE_SCALE)
        self.v = refs[2]


@pytest.mark.parametrize("mix", range(len(QKV_MIXES)))
@pytest.mark.parametrize("shape", range(len(QKV_SHAPES)))
def test_fused_qkv(gpu, orc, shape, mix):
    fused_qkv_case(gpu, orc, shape, mix, 1)


def fused_qkv_case(gpu, orc, shape, mix, structure):
    """structure: the index in hip_backend.MV_STRUCTURES every launch must have run as (1, mvqb2 split, unless the process's environment
    forces another: tests/fresh_scenarios.py)"""
    W = Worst()
    hd, nh, nkv, hidden = QKV_SHAPES[shape]
    types = QKV_MIXES[mix]
    C = Qkv(orc, types, hd, nh, nkv, hidden, with_bias=(shape + mix) % 2 == 1)
    tys = [mr.TYPE[t] for t in types]
    split3 = mix == 3                                              # no common instantiation: three launches
    poison = np.full((nkv, MAX_SEQ, hd), mm.NAN_BITS, np.uint32).view(np.float32)
    single = {}
    for n_seq, n_slots in ((3, 8), (16, 16)):
        pos, slot = C.pos[:n_seq], mm.slots(n_seq, n_slots, 77 + n_seq)
        args = (tys, C.ws, C.biases, C.X[:n_seq], C.nw, EPS, hd, nh, nkv, MAX_SEQ, pos, slot, ROPE_BASE, ROPE_SCALE)
        r = gpu.op_qkv_rope_multi(*args, max_batch=n_slots)
        r2 = gpu.op_qkv_rope_multi(*args, max_batch=n_slots)
        st = gpu.op_qkv_rope_multi(*args, max_batch=n_slots, staged=True)
        tag = "qkv %s/%s/%s hd=%d kv=%d H=%d B=%d" % (types + (hd, nkv, hidden, n_seq))
        want_counts = [0, 0, 0]
        want_counts[structure] = 3 if split3 else 1
        W.expect(r["counts"] == want_counts, "%s: structures %s" % (tag, r["counts"]))
        W.expect(all(_same(r[f], r2[f]) for f in "qkv"), "%s: a second call gives other bits" % tag)
        path = "multi qkv %s/%s/%s" % types
        for s in range(n_seq):
            W.check(path + " ROPE_Q", r["q"][s], C.q[0][s], C.q[1][s], "%s sequence %d pos %d" % (tag, s, pos[s]))
        for f in cache_fails(r, pos, slot, C, tag):
            W.expect(False, f)
        W.expect(mm.poisoned(r["q"][n_seq:]).all(), "%s: q rows of sequences the call does not have changed" % tag)
        # the quantized caches' variant: the same rows, staged per sequence; the caches are not this launch's
        W.expect(_same(st["q"], r["q"]), "%s staged: q differs from the f32-cache launch" % tag)
        for s in range(n_seq):
            W.expect(_same(st["staged"][s, 0], np.ascontiguousarray(r["k"][slot[s], :, pos[s], :]).reshape(-1)) and
                     _same(st["staged"][s, 1], np.ascontiguousarray(r["v"][slot[s], :, pos[s], :]).reshape(-1)),
                     "%s staged: sequence %d's rows differ from its cache rows" % (tag, s))
        W.expect(mm.poisoned(st["staged"][n_seq:]).all(), "%s staged: rows of sequences the call does not have changed" % tag)
        for s in range(n_seq):                                      # bit for bit the single-sequence fused launch at pos[s]
            if s not in single:
                single[s] = gpu.op_qkv_rope(tys, C.ws, C.biases, C.X[s], C.nw, EPS, hd, nh, nkv, poison, poison, int(pos[s]), ROPE_BASE, ROPE_SCALE)
            q1, k1, v1 = single[s]
            W.expect(_same(r["q"][s], q1) and _same(r["k"][slot[s], :, pos[s], :], k1[:, pos[s], :]) and
                     _same(r["v"][slot[s], :, pos[s], :], v1[:, pos[s], :]), "%s sequence %d: differs from the single-sequence launch" % (tag, s))
    W.done()


def cache_fails(r, pos, slot, C, tag):
    return (mm.cache_failures(r["k"], pos, slot, C.k[0], C.k[1], tag + " ROPE_K") +
            mm.cache_failures(r["v"], pos, slot, C.v[0], C.v[1], tag + " V_CACHE"))


# ---- grouped MoE: H = 512, EI = 1024 (the smallest widths that plan to 8 waves)
MOE_H, MOE_EI = 512, 1024


def _moe_weights(tg, td, E, H, F):
    return mr.weights(tg, "full", H, F * E, 1), mr.weights(tg, "full", H, F * E, 2), mr.weights(td, "full", F, H * E, 3)


def _moe_check(W, gpu, tg, td, stacks, E, H, F, topk, X, nw, nnw, tag, *, sel=None, sel_w=None, router=None, max_batch=16, f64_seqs=None, rows=None):
    gate, up, down = stacks
    n_seq = len(X)
    args = (mr.TYPE[tg], gate, up, mr.TYPE[td], down, E, H, F, topk, X, nw, nnw, EPS)
    kw = dict(max_batch=max_batch, sel=sel, sel_w=sel_w, router=router)
    r = gpu.op_moe_multi(*args, **kw)
    r2 = gpu.op_moe_multi(*args, **kw)
    W.expect(r["counts"][0] == 0 and sum(r["counts"]) == 2, "%s: structures %s (gate|up and down, neither as mvqb)" % (tag, r["counts"]))
    W.expect(all(_same(r[f], r2[f]) for f in ("out", "image", "ssq", "cnt", "idx", "sel", "sel_w")), "%s: a second call gives other bits" % tag)
    if sel is not None:
        W.expect(np.array_equal(r["sel"], sel) and _same(r["sel_w"], sel_w), "%s: selection not used as given" % tag)
    for f in mm.group_failures(r["cnt"], r["idx"], r["sel"], E, max_batch * topk - 1):
        W.expect(False, "%s: %s" % (tag, f))
    ex = mm.Experts(tg, gate, up, td, down, E, H, F)
    for s in range(n_seq):
        if f64_seqs is None or s in f64_seqs:
            y, e = mm.moe(ex, X[s], [X[s]] * topk, nw, r["sel"][s], r["sel_w"][s], eps=EPS, rows=rows)
            W.check("multi moe %s/%s top-%d" % (tg, td, topk), r["out"][s] if rows is None else r["out"][s][rows], y, e, "%s sequence %d" % (tag, s))
        o, _, _ = gpu.op_moe_experts(mr.TYPE[tg], gate, up, mr.TYPE[td], down, E, H, F, topk, X[s], nw, EPS, sel=r["sel"][s], sel_w=r["sel_w"][s])
        W.expect(_same(r["out"][s], o), "%s sequence %d: differs from the single-sequence MoE (max %.3g)" % (tag, s, float(np.abs(r["out"][s] - o).max())))
    # the image and the sums of squares the combine launch left: what the engine's converter makes of the new rows
    for s in range(n_seq):
        _check_image(W, "multi moe combine image", r["image"][s], r["ssq"][s], r["out"][s], nnw, "%s sequence %d" % (tag, s))
    W.expect(_same_image(r["image"][:n_seq], r["image_requant"][:n_seq]) and _same(r["ssq"][:n_seq], r["ssq_requant"][:n_seq]),
             "%s: the combine launch's image / sums of squares differ from a conversion of its output" % tag)
    W.expect(mm.poisoned(r["out"][n_seq:]).all() and mm.poisoned(r["image"][n_seq:].view(np.float32)).all() and mm.poisoned(r["ssq"][n_seq:]).all(),
             "%s: rows of sequences the call does not have changed" % tag)
    return r


@pytest.mark.parametrize("n_seq", [3, 7, 16])
@pytest.mark.parametrize("E,topk", [(8, 2), (8, 4), (4, 1)])
def test_grouped_moe_given_selections(gpu, E, topk, n_seq):
    W = Worst()
    H, F = MOE_H, MOE_EI
    for ki, kind in enumerate(("random", "same", "single")):
        case = 3 * (3, 7, 16).index(n_seq) + ki                   # the format pairs take turns over the nine cases of an (E, top_k)
        tg, td = MOE_FORMATS[(case + E + topk) % len(MOE_FORMATS)]
        X = mm.activations(H, n_seq, 41 + case)
        sel, w = mm.selections(kind, n_seq, E, topk, 51 + case)
        cnt, _ = mm.group(sel, E)
        if kind == "same":
            assert np.count_nonzero(cnt) == topk and cnt.max() == n_seq
        if kind == "single":
            assert cnt[0] == 1
        _moe_check(W, gpu, tg, td, _moe_weights(tg, td, E, H, F), E, H, F, topk, X, _norm_w(H, 1), _norm_w(H, 2), "moe E=%d top-%d B=%d %s %s/%s"
                   % (E, topk, n_seq, kind, tg, td), sel=sel, sel_w=w, max_batch=16 if n_seq != 7 else 8)
    W.done()


def test_grouped_moe_device_router(gpu):
    """Every sequence routed by its own workgroup of the router launch; the logit gaps at the selection boundary are far above the bound
    of the kernel's f32 logits, so the float64 selection is THE selection."""
    W = Worst()
    E, topk, H, F, n_seq = 8, 2, MOE_H, MOE_EI, 7
    tg, td = "Q4_K", "Q6_K"
    stacks = _moe_weights(tg, td, E, H, F)
    X = mm.activations(H, n_seq, 61)
    nw, nnw = _norm_w(H, 1), _norm_w(H, 2)
    wr = (0.05 * np.random.default_rng(62).standard_normal((E, H))).astype(np.float32)
    # the tie: experts 1 and 3 share a row that every sequence scores highest
    xn = np.stack([X[s].astype(np.float64) * mr.inv_rms(X[s], EPS) * nw for s in range(n_seq)])
    wt = (1e-3 * wr).astype(np.float32)
    wt[1] = wt[3] = (xn / (xn * xn).sum(axis=1, keepdims=True)).sum(axis=0).astype(np.float32)
    for name, router in (("router", wr), ("router tie", wt)):
        want_sel, want_w = [], []
        for s in range(n_seq):
            sel, wref, logits, lerr = mr.router(X[s], nw, EPS, router, topk)
            srt = np.sort(logits)[::-1]
            gaps = srt[:topk] - srt[1:topk + 1]
            tied = name == "router tie"
            assert (gaps[1:] if tied else gaps).min() > 100 * lerr.max(), (name, s, gaps, lerr.max())     # no case may be skipped
            if tied:
                assert logits[1] == logits[3] and list(sel) == [1, 3]
            want_sel.append(sel)
            want_w.append((wref, lerr.max()))
        r = _moe_check(W, gpu, tg, td, stacks, E, H, F, topk, X, nw, nnw, "moe %s" % name, router=router, max_batch=8)
        for s in range(n_seq):
            W.expect(list(r["sel"][s]) == list(want_sel[s]), "%s sequence %d: selected %s, float64 %s" % (name, s, list(r["sel"][s]), list(want_sel[s])))
            W.check("multi %s weights" % name, r["sel_w"][s], want_w[s][0], 8 * mr.U + 2 * want_w[s][1] + 0 * want_w[s][0], "sequence %d" % s)
    W.done()


def test_grouped_moe_partial_buffer_sizing(gpu):
    """H = 2048 (8 slices), EI = 2048, 8 experts at max_batch sequences: the gate|up launch over all experts on the split grid needs
    E * T * 2 * EI partial sums per sequence.  The scratch is sized by lgh_batch_create's own rule."""
    W = Worst()
    E, topk, H, F, n_seq = 8, 2, 2048, 2048, 16
    tg, td = "Q4_K", "Q6_K"
    stacks = _moe_weights(tg, td, E, H, F)
    X = mm.activations(H, n_seq, 71)
    sel, w = mm.selections("random", n_seq, E, topk, 72)
    r = _moe_check(W, gpu, tg, td, stacks, E, H, F, topk, X, _norm_w(H, 1), _norm_w(H, 2), "moe sizing H=2048 EI=2048 E=8 B=16", sel=sel, sel_w=w,
                   f64_seqs=(1,), rows=mm.sample_rows(H, 64, 3))
    W.expect(r["counts"] == [0, 2, 0], "sizing: both expert launches on the split grid, got %s" % r["counts"])
    W.done()


# ---- shapes the 8-wave kernels do not take: a stated refusal, not a launch error
@pytest.mark.parametrize("k", [768, 1536, 2560, 5120])
def test_refused_k(gpu, pkg, k):
    raw = mr.weights("Q4_K", "full", k, 64, 1)
    with pytest.raises(pkg.BackendError) as ei:
        gpu.op_linear_multi(mr.TYPE["Q4_K"], raw, k, 64, mm.activations(k, 3, 1), norm_w=_norm_w(k, 2))
    assert ei.value.variant == "Unsupported", ei.value


def test_batch_create_refuses_a_hidden_size_without_an_8_wave_plan(pkg, gpu):
    cfg = pkg.make_config("test-dense", max_seq_len=32, hidden_size=1536, num_layers=1, num_heads=8, head_dim=64, vocab_size=256)
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q4_K"), 32)
    with pytest.raises(pkg.BackendError) as ei:
        eng.batch_create(4)
    assert ei.value.variant == "Unsupported" and "1536" in str(ei.value), ei.value
    logits = eng.forward(3)                                       # refused before any launch: the context still decodes
    assert np.isfinite(logits).all()
    eng.close()
