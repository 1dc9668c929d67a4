"""The multi-sequence mat-vec on the f32 matrix cores (matvec_batch_f32.hip: mvqf_kernel, taken under lgh_set_batch_policy's
LGH_BATCH_F32_MATRIX) through the step's own assembly, against the float64 restatement of tests/matvec_ref.py.

Bound.  matvec_ref.matvec's form  C * u * M * inv + A  (+ the bias and epilogue terms of mr.resid / mr.swiglu / mr.rope) with
m(i) = |v_i| — the kernel reads f32 activations, no XQ chunk scale enters — and C counted for this kernel: the weight's factors d * sc
and dmin * mn (1 each, relative to |a| and |o|) and its fma (1); the product x * nw (1); along k the MFMA accumulator, one product
and one addition per element in a chain of at most k (k); the sum over the k-slices (<= 8); the epilogue as c_mfma has it: inv (1),
bias (1) and inv's own error (k / 2048 + 16, <= 48 for k <= 65536).  Sum: k + 5 + 8 + 2 + 48 <= k + 64 = C(k).  mr.matvec's family
"orc" is this form with C = k + 32; the remaining 32 * u * M * inv is added here.  The poison checks are those of
tests/test_gpu_matvec_multi.py.  Each test prints `WORST <path>: err / bound`."""
import numpy as np
import pytest

import matvec_multi_ref as mm
import matvec_ref as mr
from test_gpu_matvec import Worst
from test_gpu_matvec_multi import EPS, MAX_SEQ, QKV_MIXES, QKV_SHAPES, ROPE_BASE, ROPE_SCALE, _check_image, _norm_w

pytestmark = pytest.mark.gpu

POLICY = 1 | 2 << 8                                                # LGH_BATCH_F32_MATRIX, minimum forced to 2 sequences


def f32_linear(tname, raw, k, n, X, nw=None, bias=None, rows=None):
    """(Y, E) [n_seq, rows] with C(k) = k + 64 and m(i) = |v_i|."""
    rows = np.arange(n) if rows is None else rows
    a, o = mr.decode(tname, mm.take_rows(raw, n, rows), k, rows.size)
    out = []
    for x in X:
        y, e = mr.matvec(a, o, x, nw=nw, eps=EPS, bias=None if bias is None else bias[rows], family="orc")
        v = np.abs(x.astype(np.float64) * (1.0 if nw is None else nw.astype(np.float64)))
        out.append((y, e + 32 * mr.U * ((np.abs(a) + np.abs(o)) @ v) * (1.0 if nw is None else mr.inv_rms(x, EPS))))
    return np.stack([y for y, _ in out]), np.stack([e for _, e in out])


class Case:
    def __init__(self, gpu, tname, k, n, *, role="store", xq_next=0, norm=True, bias=False, seed=0):
        rng = np.random.default_rng(seed + k + n)
        self.gpu, self.tname, self.k, self.n, self.xq_next = gpu, tname, k, n, xq_next
        self.raw, self.raw_up = mr.weights(tname, "full", k, n, seed + 1), mr.weights(tname, "full", k, n, seed + 2) if role == "swiglu" else None
        self.X, self.nw = mm.activations(k, 16, seed + 3), _norm_w(k, seed + 4) if norm else None
        self.bias = rng.standard_normal(n).astype(np.float32) if bias else None
        self.resid = (3 * rng.standard_normal((16, n))).astype(np.float32) if role == "resid" else None
        self.next_nw, self.rows = _norm_w(n, seed + 5) if xq_next == 2 else None, mm.sample_rows(n, 192, seed)
        self.Y, self.E = f32_linear(tname, self.raw, k, n, self.X, self.nw, self.bias, self.rows)
        if role == "swiglu":
            self.Y, self.E = mr.swiglu(self.Y, self.E, *f32_linear(tname, self.raw_up, k, n, self.X, self.nw, None, self.rows))
        elif role == "resid":
            self.Y, self.E = mr.resid(self.Y, self.E, self.resid[:, self.rows])

    def check(self, W, n_seq, path):
        r = self.gpu.op_linear_multi_ex(mr.TYPE[self.tname], self.raw, self.k, self.n, self.X[:n_seq], POLICY, w_up=self.raw_up, bias=self.bias,
                                        norm_w=self.nw, eps=EPS, resid=None if self.resid is None else self.resid[:n_seq], xq_next=self.xq_next,
                                        next_nw=self.next_nw)
        tag = "%s k=%d n=%d B=%d" % (path, self.k, self.n, n_seq)
        want = [1, 0, 0, 0] if n_seq == 1 else [0, 0, 0, 1]         # one sequence never takes the new kernel; every other launch does
        W.expect(r["counts"] == want, "%s: structures %s, want %s" % (tag, r["counts"], want))
        W.expect(r["used"] == (self.xq_next != 0), "%s: image left = %s" % (tag, r["used"]))
        for s in range(n_seq):
            W.check(path, r["out"][s][self.rows], self.Y[s], self.E[s], "%s sequence %d" % (tag, s))
            if self.xq_next:
                _check_image(W, path + " image", r["image"][s], r["ssq"][s] if self.xq_next == 2 else None, r["out"][s], self.next_nw, tag)
        img = r["image"] is not None                                # what must still hold the poison pattern
        keep = {"output rows of sequences beyond n_seq": r["out"][n_seq:], "floats past row n": r["pad"],
                "image of sequences beyond n_seq": r["image"][n_seq:].view(np.float32) if img else None, "ssq of sequences beyond n_seq": r["ssq"][n_seq:] if img else None,
                "ssq without norm weights": r["ssq"] if img and self.xq_next != 2 else None,
                "unasked image": r["image"].view(np.float32) if img and not self.xq_next else None}
        for what, a in keep.items():
            W.expect(a is None or mm.poisoned(a).all(), "%s: %s changed" % (tag, what))


@pytest.mark.parametrize("tname", mr.FUSED)
def test_formats_and_sequence_counts(gpu, tname):
    W, L = Worst(), Case(gpu, tname, 1024, 272, seed=100)
    for n_seq in (1, 5, 9, 16):
        L.check(W, n_seq, "mvqf %s store" % tname)
    W.done()


# one block (SEQ); two slices; uneven slices; several staged chunks per slice; the SEQ grid with several slices, a ragged last tile and
# a last workgroup with inactive units
@pytest.mark.parametrize("tname", ["Q4_K", "Q6_K"])
@pytest.mark.parametrize("k,n", [(256, 48), (512, 64), (2816, 272), (5632, 96), (512, 20500)])
def test_k_geometry(gpu, tname, k, n):
    W, L = Worst(), Case(gpu, tname, k, n, seed=200)
    for n_seq in (3, 16):
        L.check(W, n_seq, "mvqf %s k-slices" % tname)
    W.done()


@pytest.mark.parametrize("name,tname,k,n,role,xq_next,bias", [("gate|up", "Q4_K", 512, 1024, "swiglu", 1, False),
                                                              ("wo", "Q4_K", 1024, 512, "resid", 2, True),
                                                              ("down", "Q6_K", 1024, 512, "resid", 1, False)])
def test_epilogues(gpu, name, tname, k, n, role, xq_next, bias):
    W, L = Worst(), Case(gpu, tname, k, n, role=role, xq_next=xq_next, norm=role == "swiglu", bias=bias, seed=500)
    for n_seq in (3, 16):
        L.check(W, n_seq, "mvqf %s %s" % (tname, name))
    W.done()


@pytest.mark.parametrize("mix", [0, 1])
def test_fused_qkv(gpu, orc, mix):
    """RoPE at every sequence's own position, K / V rows into its own cache slot; every other cache row keeps the pattern."""
    W = Worst()
    (hd, nh, nkv, hidden), types = QKV_SHAPES[0], QKV_MIXES[mix]
    rows = (nh * hd, nkv * hd, nkv * hd)
    ws = [mr.weights(types[i], "full", hidden, rows[i], 10 + i) for i in range(3)]
    nw, X, allpos = _norm_w(hidden, 5), mm.activations(hidden, 16, 900), mm.positions(16, MAX_SEQ)
    biases = [np.random.default_rng(i).standard_normal(rows[i]).astype(np.float32) for i in range(3)]
    pre = [f32_linear(types[i], ws[i], hidden, rows[i], X, nw, biases[i]) for i in range(3)]
    for n_seq, n_slots in ((3, 8), (16, 16)):
        pos, slot = allpos[:n_seq], mm.slots(n_seq, n_slots, 77 + n_seq)
        r = gpu.op_qkv_rope_multi_ex([mr.TYPE[t] for t in types], ws, biases, X[:n_seq], nw, EPS, hd, nh, nkv, MAX_SEQ, pos, slot, ROPE_BASE, ROPE_SCALE,
                                     max_batch=n_slots, batch_policy=POLICY)
        tag = "mvqf qkv %s/%s/%s B=%d" % (types + (n_seq,))
        W.expect(r["counts"] == [0, 0, 0, 1], "%s: structures %s" % (tag, r["counts"]))
        q = mm.rope_rows(orc, pre[0][0][:n_seq], pre[0][1][:n_seq], pos, hd, ROPE_BASE, ROPE_SCALE)
        kk = mm.rope_rows(orc, pre[1][0][:n_seq], pre[1][1][:n_seq], pos, hd, ROPE_BASE, ROPE_SCALE)
        for s in range(n_seq):
            W.check("mvqf qkv ROPE_Q", r["q"][s], q[0][s], q[1][s], "%s sequence %d" % (tag, s))
        for f in mm.cache_failures(r["k"], pos, slot, kk[0], kk[1], tag + " ROPE_K") + mm.cache_failures(r["v"], pos, slot, *pre[2], tag + " V_CACHE"):
            W.expect(False, f)
        W.expect(mm.poisoned(r["q"][n_seq:]).all(), "%s: q rows of sequences the call does not have changed" % tag)
    W.done()


def test_engine_policy(pkg, gpu, orc):
    """A 2-layer dense model, hidden 1024, 6 sequences at ragged positions, 8 steps under the policy: the oracle's bound, greedy tokens,
    graph == no graph, policy 0 == the single-sequence engine again, and what the setter refuses."""
    cfg = pkg.make_config("test-dense", max_seq_len=64, hidden_size=1024, num_layers=2)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    B, steps = 6, 8
    hist = [[int(t) for t in np.random.default_rng(1000 + s).integers(0, cfg.vocab_size, size=1 + s + steps)] for s in range(B)]

    def run(flags):
        eng = pkg.HipGpuInference.from_model(model, 64, flags=flags)
        for word in (pkg.hip_backend.BATCH_F32_MATRIX, 1 << 5):     # before batch_create; then, after it, unknown bits
            with pytest.raises(pkg.BackendError) as ei:
                eng.set_batch_policy(word)
            assert ei.value.variant == "InvalidArgument", ei.value
            eng.batch_create(8)
        for s in range(B):                                          # ragged: slot s holds 1 + s tokens
            for t in hist[s][:1 + s]:
                eng.forward_multi([s], [t])
        eng.set_batch_policy(pkg.hip_backend.BATCH_F32_MATRIX | 5 << 8)   # from 5 sequences on
        before = gpu.mvqf_launches()
        out = [eng.forward_multi(list(range(B)), [hist[s][1 + s + t] for s in range(B)], greedy=True) for t in range(steps)]
        assert gpu.mvqf_launches() > before                         # (counted where the launch is enqueued: eagerly, or at the capture)
        return eng, out

    eng, out = run(0)
    eng_ng, out_ng = run(pkg.hip_backend.FLAG_NO_GRAPH)
    assert all(np.array_equal(l0.view(np.uint32), l1.view(np.uint32)) and np.array_equal(n0, n1) for (l0, n0), (l1, n1) in zip(out, out_ng))
    eng_ng.close()
    worst = 0.0
    for s in range(B):
        ref = orc.Model(cfg.as_dict())
        for nm, t, ne, data in model.tensors(keep=True):
            ref.add_tensor(nm, t, ne, data)
        ref.finalize()
        ref.forward(hist[s][:1 + s])
        for t in range(steps):
            want = ref.forward([hist[s][1 + s + t]])
            err, tol = float(np.abs(out[t][0][s] - want).max()), 2e-3 * float(np.abs(want).max()) + 2e-3
            worst = max(worst, err / tol)
            assert err <= tol, (s, t, err)
            top = np.sort(want)[-2:]
            if top[1] - top[0] > 4 * err:
                assert int(out[t][1][s]) == int(orc.argmax_last(want)), (s, t)
    print("WORST mvqf engine vs oracle (of 2e-3 max|logit| + 2e-3): %.3g" % worst)
    # policy 0: the same context is bit-identical to the single-sequence engine again
    eng.set_batch_policy(0)
    [eng.batch_reset(s) for s in range(B)]
    single = pkg.HipGpuInference.from_model(model, 64, attn_direct=255)
    got = [eng.forward_multi(list(range(B)), [hist[s][t] for s in range(B)])[0] for t in range(3)]
    for s in range(B):
        single.reset()
        for t in range(3):
            assert np.array_equal(got[t][s].view(np.uint32), single.forward(hist[s][t]).view(np.uint32)), (s, t)
    single.close()
    eng.close()
