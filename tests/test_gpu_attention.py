"""Every engine attention kernel against the float64 restatement (tests/attention_ref.py), through the per-path entry points
(lgh_op_attention_decode / _kv8 / _tq / _prefill), which run the engine's own launch sequences with the position in the
device word.

Paths and kernels:  f32 split + merge  attn_partial_kernel<D,G,4> (max_seq < 2048) / <D,G,8> (max_seq >= 2048) + attn_combine_kernel;
f32 direct  attn_partial_kernel<D,G,16,false,true>;  any shape  attn_decode_any_kernel;  int8 / FP8  attn_partial_q8_kernel<D,G,4,FMT>;
TurboQuant  attn_tq_partial_kernel<D,G,BITS,QJL> + attn_tq_combine_kernel<D>;  prompt pass  attn_pf_mfma_kernel<D,8>.

Every cache row past the visible range holds NaN (f32 NaN, the FP8 byte 0x7F, an int8 row with a NaN scale, a QJL row with a NaN
norm), and so does the row the kv8 / TurboQuant launch is about to write: a read of any of them shows as NaN in the output.
Each test prints its worst error as a fraction of the bound, per path."""
import numpy as np
import pytest

import attention_ref as ar

pytestmark = pytest.mark.gpu

SHAPES = [(d, g) for d in (64, 128) for g in (1, 2, 4, 8)]
ANY_SHAPES = [(96, 7), (80, 3), (96, 3), (80, 7)]
N_KV = 2
# (max_seq, pos): around 64 rows (one row per lane; the smallest threshold the flags can set, attn_direct=1), the last context the
# default engine gives the head kernel (kDirectAttnDefaultKv = 256 rows: pos 255) and the first it gives split + merge (pos 256), a long
# context, and max_seq >= 2048 (8 waves).  (The case index seeds the case's data: new cases go at the end.)
DECODE_POS = [(1024, p) for p in (0, 1, 63, 64, 65, 1000)] + [(4096, 1000), (4096, 4095)] + [(1024, 255), (1024, 256)]
BYTE_POS = [(1024, p) for p in (0, 1, 63, 64, 65, 1000)] + [(4096, 4095)]
SPLITS = (1, 7, 32)   # the engine's default is min(32, 256 / n_kv); 32 splits at pos 0 / 1 is more splits than rows
PF_POS0 = (0, 5, 16, 2000)
PF_M = (1, 15, 16, 17, 100, 128)


class Worst:
    """Worst error / bound per path, and every case over the bound."""

    def __init__(self, name):
        self.name, self.ratio, self.fails = name, {}, []

    def add(self, path, ratio, case):
        self.ratio[path] = max(self.ratio.get(path, 0.0), ratio)
        if not ratio <= 1.0:
            self.fails.append(f"{path} {case}: err / bound = {ratio:.3g}")

    def check(self):
        for path, r in sorted(self.ratio.items()):
            print(f"WORST {self.name} {path}: err / bound = {r:.4f}")
        assert not self.fails, "\n".join(self.fails[:20])


def _dominant_row(rng, qg, d, scale, others_max):
    """A key whose score beats every other visible row of the group's queries qg [G, d] by >= 20 (other weights < 2.1e-9)."""
    u = qg.sum(axis=0)
    u = u / np.linalg.norm(u)
    c = float((qg.astype(np.float64) @ u).min())
    assert c > 0.5
    return (u * (22.0 + others_max) / (scale * c)).astype(np.float32)


def _queries(rng, kind, n_heads, g, d):
    q = rng.standard_normal((n_heads, d)).astype(np.float32)
    if kind == "dominant":   # a group's queries share a direction, so one key can dominate for all of them
        base = rng.standard_normal((n_heads // g, 1, d))
        q = (np.repeat(base, g, axis=1).reshape(n_heads, d) + 0.3 * q).astype(np.float32)
    if kind == "hot":        # scores in the hundreds: the online softmax's rescaling
        q *= 30.0
    return q


def _f32_case(rng, kind, g, d, max_seq, pos):
    """q [N_KV G, d], K / V [N_KV, max_seq, d] f32: rows 0..pos visible, NaN after."""
    n = pos + 1
    q = _queries(rng, kind, N_KV * g, g, d)
    k = np.full((N_KV, max_seq, d), np.nan, np.float32)
    v = np.full((N_KV, max_seq, d), np.nan, np.float32)
    k[:, :n] = rng.standard_normal((N_KV, n, d))
    v[:, :n] = rng.standard_normal((N_KV, n, d))
    scale = 1.0 / np.sqrt(d)
    if kind == "equal":      # every key the same: the output is the exact mean of V
        k[:, :n] = rng.standard_normal((N_KV, 1, d))
    if kind == "dominant":   # kv head 0: the last visible row dominates; kv head 1: row 0
        for h, j in ((0, pos), (1, 0)):
            qg = q[h * g:(h + 1) * g]
            others = float((qg.astype(np.float64) @ k[h, :n].astype(np.float64).T).max()) * scale
            k[h, j] = _dominant_row(rng, qg, d, scale, abs(others))
    return q, k, v, scale


@pytest.mark.parametrize("d,g", SHAPES)
def test_decode_f32_paths(gpu, d, g):
    """Split + merge (4 and 8 waves), direct, the any-shape kernel and lgh_op_attention_cached on the same inputs, each within the
    bound against the float64 reference."""
    W = Worst(f"decode_f32 d={d} g={g}")
    for ci, (max_seq, pos) in enumerate(DECODE_POS):
        for kind in ("normal", "dominant", "equal", "hot"):
            rng = np.random.default_rng([d, g, ci, len(kind)])
            q, k, v, scale = _f32_case(rng, kind, g, d, max_seq, pos)
            n = pos + 1
            ref = ar.decode(q, k, v, scale, n)
            S, vmax = ar.magnitude(q, k, scale, n), float(np.abs(v[:, :n]).max())
            case = f"kind={kind} max_seq={max_seq} pos={pos}"
            waves = 8 if max_seq >= 2048 else 4
            for s in SPLITS:
                got = gpu.op_attention_decode(gpu.ATTN_SPLIT, q, k, v, scale, pos, s)
                W.add(f"split{waves}", ar.worst_ratio(got, ref, S, vmax, n), f"{case} splits={s}")
            got = gpu.op_attention_cached(q, k, v, scale, n, SPLITS[ci % 3])   # kv_len_fixed: 4 waves (kv_len < 2048)
            W.add("attention_cached", ar.worst_ratio(got, ref, S, vmax, n), case)
            W.add("direct", ar.worst_ratio(gpu.op_attention_decode(gpu.ATTN_DIRECT, q, k, v, scale, pos), ref, S, vmax, n), case)
            W.add("any", ar.worst_ratio(gpu.op_attention_decode(gpu.ATTN_ANY, q, k, v, scale, pos), ref, S, vmax, n), case)
    W.check()


@pytest.mark.parametrize("d,g", ANY_SHAPES)
def test_decode_any_shape(gpu, pkg, d, g):
    """attn_decode_any_kernel at the head sizes / group sizes the templated kernels do not cover; those paths refuse them."""
    W = Worst(f"decode_any d={d} g={g}")
    for ci, (max_seq, pos) in enumerate(DECODE_POS):
        for kind in ("normal", "dominant", "equal", "hot"):
            rng = np.random.default_rng([d, g, ci, len(kind), 1])
            q, k, v, scale = _f32_case(rng, kind, g, d, max_seq, pos)
            n = pos + 1
            ref = ar.decode(q, k, v, scale, n)
            S, vmax = ar.magnitude(q, k, scale, n), float(np.abs(v[:, :n]).max())
            got = gpu.op_attention_decode(gpu.ATTN_ANY, q, k, v, scale, pos)
            W.add("any", ar.worst_ratio(got, ref, S, vmax, n), f"kind={kind} max_seq={max_seq} pos={pos}")
    for path in (gpu.ATTN_SPLIT, gpu.ATTN_DIRECT):
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_attention_decode(path, q, k, v, scale, 3, 4)
        assert ei.value.variant == "Unsupported"
    W.check()


# ---- int8 / FP8 caches
def _kv8_encode(orc, kv_type, x):
    """The oracle's encoding of one row: (bytes uint8 [d], scale)."""
    if kv_type == 1:
        b, sc = orc.kv_quantize_int8(x)
        return b.view(np.uint8), np.float32(sc)
    fmt = {2: orc.FP8_E4M3, 3: orc.FP8_E5M2}[kv_type]
    return np.array([orc.kv_quantize_fp8(fmt, float(e)) for e in x], np.uint8), np.float32(1.0)


@pytest.mark.parametrize("d,g", SHAPES)
@pytest.mark.parametrize("kv_type", [1, 2, 3], ids=["int8", "fp8_e4m3", "fp8_e5m2"])
def test_decode_kv8(gpu, orc, kv_type, d, g):
    """attn_partial_q8_kernel: rows 0..pos-1 read from the byte cache, row pos quantized from k_new / v_new, stored bit-exactly as
    the oracle encodes it and attended through its stored values; every other row is left as it was."""
    W = Worst(f"kv8 type={kv_type} d={d} g={g}")
    table = ar.fp8_table(orc, kv_type) if kv_type != 1 else None
    finite = np.flatnonzero(np.isfinite(table) & (np.abs(table) <= 4.0)) if table is not None else None
    values = (lambda b, s: ar.int8_values(b, s)) if kv_type == 1 else (lambda b, s: table[b])
    for ci, (max_seq, pos) in enumerate(BYTE_POS):
        for ki, kind in enumerate(("normal", "dominant", "hot")):
            rng = np.random.default_rng([kv_type, d, g, ci, ki])
            q = _queries(rng, kind, N_KV * g, g, d)
            scale = 1.0 / np.sqrt(d)
            if kv_type == 1:
                kb = rng.integers(-127, 128, (N_KV, max_seq, d)).astype(np.int8).view(np.uint8)
                vb = rng.integers(-127, 128, (N_KV, max_seq, d)).astype(np.int8).view(np.uint8)
                ks = rng.uniform(0.005, 0.03, (N_KV, max_seq)).astype(np.float32)
                vs = rng.uniform(0.005, 0.03, (N_KV, max_seq)).astype(np.float32)
                ks[:, pos:] = np.nan   # int8 rows past the cached ones (and the row about to be written): NaN scale
                vs[:, pos:] = np.nan
            else:
                kb = rng.choice(finite, (N_KV, max_seq, d)).astype(np.uint8)
                vb = rng.choice(finite, (N_KV, max_seq, d)).astype(np.uint8)
                kb[:, pos:] = 0x7F     # the FP8 NaN byte
                vb[:, pos:] = 0x7F
                ks = vs = None
            k_new = rng.standard_normal((N_KV, d)).astype(np.float32)
            v_new = rng.standard_normal((N_KV, d)).astype(np.float32)
            if kind == "dominant":   # kv head 0: the new row dominates; kv head 1: the last cached row
                k_new[0] = _dominant_row(rng, q[:g], d, scale, 40.0)
                if pos > 0:
                    b, s = _kv8_encode(orc, kv_type, _dominant_row(rng, q[g:2 * g], d, scale, 40.0))
                    kb[1, pos - 1] = b
                    if kv_type == 1:
                        ks[1, pos - 1] = s
            # what the cache must hold after the call
            kb_x, vb_x = kb.copy(), vb.copy()
            ks_x = ks.copy() if kv_type == 1 else None
            vs_x = vs.copy() if kv_type == 1 else None
            for h in range(N_KV):
                kb_x[h, pos], s = _kv8_encode(orc, kv_type, k_new[h])
                if kv_type == 1:
                    ks_x[h, pos] = s
                vb_x[h, pos], s = _kv8_encode(orc, kv_type, v_new[h])
                if kv_type == 1:
                    vs_x[h, pos] = s
            n = pos + 1
            kv_vals = values(kb_x[:, :n], ks_x[:, :n] if kv_type == 1 else None)
            vv_vals = values(vb_x[:, :n], vs_x[:, :n] if kv_type == 1 else None)
            s_split = SPLITS[(ci + ki) % 3]
            out, kb_g, vb_g, ks_g, vs_g = gpu.op_attention_kv8(kv_type, q, kb, vb, ks, vs, k_new, v_new, scale, pos, s_split)
            case = f"kind={kind} max_seq={max_seq} pos={pos} splits={s_split}"
            np.testing.assert_array_equal(kb_g, kb_x, err_msg=f"K bytes {case}")
            np.testing.assert_array_equal(vb_g, vb_x, err_msg=f"V bytes {case}")
            if kv_type == 1:
                np.testing.assert_array_equal(ks_g.view(np.uint32), ks_x.view(np.uint32), err_msg=f"K scales {case}")
                np.testing.assert_array_equal(vs_g.view(np.uint32), vs_x.view(np.uint32), err_msg=f"V scales {case}")
            ref = ar.decode(q, kv_vals, vv_vals, scale, n)
            S, vmax = ar.magnitude(q, kv_vals, scale, n), float(np.abs(vv_vals).max())
            W.add("q8", ar.worst_ratio(out, ref, S, vmax, n), case)
    W.check()


# ---- TurboQuant caches
@pytest.mark.parametrize("d,g", SHAPES)
@pytest.mark.parametrize("kv_type", [4, 5, 6, 7], ids=["tq2", "tq3", "tq2_qjl", "tq3_qjl"])
def test_decode_tq(gpu, orc, kv_type, d, g):
    """attn_tq_partial_kernel + attn_tq_combine_kernel: row pos compressed from k_new / v_new exactly as the oracle compresses it
    (codes, QJL bits and norm), every other row unchanged, and the output within the bound of the float64 attention over the
    rows' values R^-1(centroid[code]) (+ the QJL correction of the scores)."""
    bits = 2 if kv_type in (4, 6) else 3
    qjl = kv_type in (6, 7)
    rb = d // 4 if bits == 2 else d // 8 * 3
    xw = d // 32 + 1
    W = Worst(f"tq type={kv_type} d={d} g={g}")
    for ci, (max_seq, pos) in enumerate(BYTE_POS):
        for ki, kind in enumerate(("normal", "dominant", "hot")):
            rng = np.random.default_rng([kv_type, d, g, ci, ki, 2])
            q = _queries(rng, kind, N_KV * g, g, d)
            scale = 1.0 / np.sqrt(d)
            signs = np.where(rng.random((N_KV, 2, d)) < 0.5, -1.0, 1.0).astype(np.float32)
            S = rng.standard_normal((N_KV, d, d)).astype(np.float32) if qjl else None
            kc = rng.integers(0, 256, (N_KV, max_seq, rb)).astype(np.uint8)
            vc = rng.integers(0, 256, (N_KV, max_seq, rb)).astype(np.uint8)
            kx = None
            if qjl:
                kx = rng.integers(0, 2 ** 32, (N_KV, max_seq, xw), dtype=np.uint64).astype(np.uint32)
                nrm = (0.3 * np.abs(rng.standard_normal((N_KV, max_seq)))).astype(np.float32)
                nrm[:, pos:] = np.nan  # rows never visible, and the row about to be written: NaN norm
                kx[:, :, xw - 1] = nrm.view(np.uint32)
            k_new = rng.standard_normal((N_KV, d)).astype(np.float32)
            v_new = rng.standard_normal((N_KV, d)).astype(np.float32)
            if kind == "dominant":
                for h in range(N_KV):
                    k_new[h] = _dominant_row(rng, q[h * g:(h + 1) * g], d, scale, 40.0)
            kc_x, vc_x = kc.copy(), vc.copy()
            kx_x = kx.copy() if qjl else None
            for h in range(N_KV):
                if qjl:
                    codes, qb, norm = orc.tq_compress_qjl(k_new[h], bits, signs[h, 0], S[h])
                    kc_x[h, pos] = codes
                    kx_x[h, pos] = np.concatenate([qb.view(np.uint32), np.float32([norm]).view(np.uint32)])
                else:
                    kc_x[h, pos] = orc.tq_compress(k_new[h], bits, signs[h, 0])
                vc_x[h, pos] = orc.tq_compress(v_new[h], bits, signs[h, 1])
            s_split = SPLITS[(ci + ki) % 3]
            out, kc_g, vc_g, kx_g = gpu.op_attention_tq(kv_type, q, kc, vc, kx, k_new, v_new, signs, S, scale, pos, s_split)
            case = f"kind={kind} max_seq={max_seq} pos={pos} splits={s_split}"
            np.testing.assert_array_equal(kc_g, kc_x, err_msg=f"K codes {case}")
            np.testing.assert_array_equal(vc_g, vc_x, err_msg=f"V codes {case}")
            if qjl:
                np.testing.assert_array_equal(kx_g, kx_x, err_msg=f"QJL rows {case}")
            n = pos + 1
            ref, s_mag, vmax = ar.tq_decode(orc, q, kc_x, vc_x, bits, signs, scale, n, kx_x, S)
            W.add("tq_qjl" if qjl else "tq", ar.worst_ratio(out, ref, s_mag, vmax, n), case)
    W.check()


# ---- the prompt pass
def _pf_kv(d, g):
    """kv heads so that n_heads * d is a multiple of 256 (the XH layout's slab width), and at least two of them."""
    return 2 * max(1, 256 // (d * g))


@pytest.mark.parametrize("d,g", SHAPES)
def test_prefill(gpu, d, g):
    """attn_pf_mfma_kernel: token t of the block sees rows <= pos0 + t; its f16 output within the f32 bound plus one f16 rounding."""
    prefill_case(gpu, d, g)


def prefill_case(gpu, d, g, keep=None):
    """(the test above; returns the output of the case keep = (pos0, m, kind), for tests/fresh_scenarios.py)"""
    kept = None
    n_kv = _pf_kv(d, g)
    nh = n_kv * g
    max_seq = 2176
    W = Worst(f"prefill d={d} g={g}")
    for pos0 in PF_POS0:
        for m in PF_M:
            kinds = ("normal", "dominant", "equal", "hot") if m in (17, 128) else ("normal",)
            for ki, kind in enumerate(kinds):
                rng = np.random.default_rng([d, g, pos0, m, ki, 3])
                n = pos0 + m
                scale = 1.0 / np.sqrt(d)
                q = np.stack([_queries(rng, kind, nh, g, d) for _ in range(m)]) if kind != "dominant" else None
                if kind == "dominant":   # every token's group shares one direction; row pos0 (the block's first) dominates
                    base = rng.standard_normal((n_kv, 1, 1, d))
                    q = (np.repeat(base, g, axis=1).reshape(1, nh, d) + 0.3 * rng.standard_normal((m, nh, d))).astype(np.float32)
                k = np.full((n_kv, max_seq, d), np.nan, np.float32)
                v = np.full((n_kv, max_seq, d), np.nan, np.float32)
                k[:, :n] = rng.standard_normal((n_kv, n, d))
                v[:, :n] = rng.standard_normal((n_kv, n, d))
                if kind == "equal":
                    k[:, :n] = rng.standard_normal((n_kv, 1, d))
                if kind == "dominant":
                    for h in range(n_kv):
                        qg = q[:, h * g:(h + 1) * g].reshape(-1, d)
                        others = float(np.abs(qg.astype(np.float64) @ k[h, :n].astype(np.float64).T).max()) * scale
                        k[h, pos0] = _dominant_row(rng, qg, d, scale, others)
                ref = ar.prefill(q, k, v, scale, pos0, m).reshape(m, nh * d)
                S, vmax = ar.magnitude(q, k, scale, n), float(np.abs(v[:, :n]).max())
                got = gpu.op_attention_prefill(q, k, v, scale, pos0)
                W.add("pf_mfma", ar.worst_ratio(got, ref, S, vmax, n, f16=True), f"kind={kind} pos0={pos0} m={m}")
                if keep == (pos0, m, kind):
                    kept = got
    W.check()
    return kept


def test_entry_points_refuse(gpu, pkg):
    """Shapes a path has no kernel for, and blocks the prompt pass cannot hold, are refused (never served by another kernel)."""
    rng = np.random.default_rng(5)
    q = rng.standard_normal((7 * 2, 96)).astype(np.float32)
    k = rng.standard_normal((2, 64, 96)).astype(np.float32)
    for path in (gpu.ATTN_SPLIT, gpu.ATTN_DIRECT):
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_attention_decode(path, q, k, k, 0.1, 3, 4)
        assert ei.value.variant == "Unsupported"
    b = np.zeros((2, 64, 96), np.uint8)
    sc = np.ones((2, 64), np.float32)
    x = np.zeros((2, 96), np.float32)
    with pytest.raises(pkg.BackendError) as ei:
        gpu.op_attention_kv8(1, q, b, b, sc, sc, x, x, 0.1, 3, 4)
    assert ei.value.variant == "Unsupported"
    with pytest.raises(pkg.BackendError) as ei:
        gpu.op_attention_tq(4, q, b, b, None, x, x, np.ones((2, 2, 96), np.float32), None, 0.1, 3, 4)
    assert ei.value.variant == "Unsupported"
    kc = rng.standard_normal((1, 256, 128)).astype(np.float32)
    for qq, pos0, why in ((np.zeros((129, 2, 128), np.float32), 0, "m > 128"), (np.zeros((4, 1, 128), np.float32), 0, "n_heads d % 256"),
                          (np.zeros((4, 2, 128), np.float32), 253, "past max_seq")):
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_attention_prefill(qq, kc, kc, 0.1, pos0)
        assert ei.value.variant == "InvalidArgument", why
