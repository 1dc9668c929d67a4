"""The 56-block static plans of the matrix-core mat-vec (down, k = 14336: csrc/matvec_mfma.hip, mvqs_body) request each x record
right in front of the weight tile that first uses it and wait for it with a counted vmcnt.  A count that is too large would let a
wave read a record before it has landed, so every launch here is compared bitwise with the generic kernel (mvq_kernel, which
requests all records first), held to the float64 bound of tests/matvec_ref.py, and run twice.

Shapes (residual epilogue, XQ image times the next norm's weights and sums of squares out): n = 16 (one workgroup, one tile), 17 (a
second workgroup, ragged), 48, 4096 (256 workgroups of one tile: the decode graph's launch) and 4112 = 257 tiles, for which mvq_plan
takes two tiles per workgroup (Rg = 2; the last workgroup has one): records are requested once and read again by the second tile.
Inputs: `normal`; zero except the LAST record of the vector; zero except the last record of EVERY wave's k-slice (blocks 6, 13, ...,
55) — the records that are requested last, behind the refill tiles."""
import contextlib

import numpy as np
import pytest

import matvec_ref as mr

pytestmark = pytest.mark.gpu

K, NBLK, NBW = 14336, 56, 7
N_MAX = 4112
SIZES = (16, 17, 48, 4096, N_MAX)
POISON = 0xA5   # lgh_op_linear_image fills the image and the sums of squares with it before the launch


def inputs():
    base = mr.activation("normal", K, 91)
    last = np.zeros(K, np.float32)
    last[-256:] = base[-256:]
    per_wave = np.zeros(K, np.float32)
    for w in range(8):
        b = w * NBW + NBW - 1
        per_wave[b * 256:(b + 1) * 256] = base[b * 256:(b + 1) * 256]
    return {"normal": base, "last record": last, "last record of every wave": per_wave}


@pytest.fixture(scope="module", params=["Q4_K", "Q6_K"])
def case(request):
    """Weights of N_MAX rows (smaller shapes take the first rows) and, per input, the float64 result and bound of every row."""
    tname = request.param
    raw = mr.weights(tname, "full", K, N_MAX, 7 + len(tname))
    rb = raw.size // N_MAX
    xs = inputs()
    ys = {name: ([], []) for name in xs}
    for r0 in range(0, N_MAX, 512):
        m = min(512, N_MAX - r0)
        a, o = mr.decode(tname, raw[r0 * rb:(r0 + m) * rb], K, m, None, "mfma")
        for name, x in xs.items():
            y, e = mr.matvec(a, o, x, family="mfma")
            ys[name][0].append(y)
            ys[name][1].append(e)
    ref = {name: (np.concatenate(y), np.concatenate(e)) for name, (y, e) in ys.items()}
    rng = np.random.default_rng(5)
    res = (3 * rng.standard_normal(N_MAX)).astype(np.float32)
    nnw = (1 + 0.2 * rng.standard_normal(N_MAX)).astype(np.float32)
    return tname, raw, rb, xs, ref, res, nnw


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


def unwritten_image_bytes(n):
    """Bytes of the image's limb and per-chunk areas that belong to elements at or past n (xq.h's record layout)."""
    nrec = (n + 255) // 256
    mask = np.zeros((nrec, 1280), bool)
    el = np.arange(256)
    for r in range(nrec):
        gone = el[(r * 256 + el) >= n]
        for i in range(4):
            mask[r, ((gone // 32) * 4 + i) * 32 + gone % 32] = True
    return mask.reshape(-1)


@pytest.mark.parametrize("n", SIZES)
def test_down_plan_streams_x(gpu, case, n):
    tname, raw, rb, xs, ref, res, nnw = case
    geo = mr.mvq_geometry(K, n)
    assert (geo["T"], geo["G"], geo["nbw"]) == (8, 1, NBW) and geo["Rg"] == (2 if n == N_MAX else 1), geo
    w = raw[:n * rb]
    fails = []
    for name, x in xs.items():
        kw = dict(resid=res[:n], xq_next=2, next_nw=nnw[:n])
        s = gpu.op_linear_image(mr.TYPE[tname], w, K, n, x, **kw)
        s2 = gpu.op_linear_image(mr.TYPE[tname], w, K, n, x, **kw)
        with generic(gpu):
            g = gpu.op_linear_image(mr.TYPE[tname], w, K, n, x, **kw)
        assert (s["static"], s2["static"], g["static"]) == (1, 1, 0), "which kernel ran: %s" % ((s["static"], s2["static"], g["static"]),)
        tag = "%s n=%d %s" % (tname, n, name)
        y, e = mr.resid(ref[name][0][:n], ref[name][1][:n], res[:n])
        for what, r in (("static", s), ("generic", g)):
            got = np.asarray(r["out"], np.float64)
            ratio = np.abs(got - y) / e
            ratio[~np.isfinite(got)] = np.inf
            print("WORST %s %s: %.3g" % (tag, what, ratio.max()))
            if not ratio.max() <= 1.0:
                fails.append("%s: %s kernel against float64: ratio %.3g" % (tag, what, ratio.max()))
        for key in ("out", "image", "ssq"):
            if not same(s[key], s2[key]):
                fails.append("%s: %s differs between two calls" % (tag, key))
            if not same(s[key], g[key]):
                fails.append("%s: %s differs from the generic kernel's" % (tag, key))
        if n % 16 == 0 and s["image"] is None:
            fails.append("%s: no XQ image left" % tag)
        if s["image"] is not None and n % 256:
            keep = unwritten_image_bytes(n)
            if not np.all(s["image"][keep] == POISON):
                fails.append("%s: %d image bytes past row n changed" % (tag, int(np.sum(s["image"][keep] != POISON))))
    assert not fails, "\n".join(fails)
