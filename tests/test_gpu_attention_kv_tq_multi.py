"""attn_tq_partial_kernel<D,G,BITS,QJL,MULTI> + attn_tq_combine_kernel<D,MULTI> through lgh_op_attention_tq_multi: the multi-sequence
decode step's attention over TurboQuant cache slots, against the float64 restatement (tests/attention_ref.py through
tests/attention_tq_multi_ref.py) and, bit for bit, against the single-sequence launch (lgh_op_attention_tq) on each slot alone.

One launch mixes sequences whose positions put them on different paths of the kernel's loop (only the staged row; fewer rows than
workgroups; the first batch of kAhead passes exactly full; one row into the second batch, whose rows come from memory inside the
loop; the last row of a slot), on slots that are not the identity with at least one slot unused; everything a sequence must not
read is poisoned (attention_tq_multi_ref.make_case).  Each test prints its worst error as a fraction of the bound.

test_attention_images: wo's input as every attention entry point's last launch leaves it (the XQ image of its output), against that
launch's own f32 output."""
import numpy as np
import pytest

import attention_kv8_multi_ref as m8
import attention_ref as ar
import attention_tq_multi_ref as mr
import matvec_multi_ref as mm

pytestmark = pytest.mark.gpu

SHAPES = [(d, g) for d in (64, 128) for g in (1, 4, 8)]
POISON = 0x7FC0BEEF


def _run(gpu, case, n_splits, **kw):
    return gpu.op_attention_tq_multi(case["kv_type"], case["q"], case["kc"], case["vc"], case["kx"], case["k_new"], case["v_new"], case["signs"],
                                     case["S"], case["scale"], case["pos"], case["slot"], n_splits, **kw)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(gpu, orc, case, n_splits, label):
    """Every assertion of one launch; -> the worst err / bound of its sequences."""
    kt, qjl = case["kv_type"], case["qjl"]
    out, kc_g, vc_g, kx_g = _run(gpu, case, n_splits)
    kc_x, vc_x, kx_x = after = mr.after_call(orc, case)
    # 1. rows pos[s] of slots slot[s] as the oracle compresses the staged rows, every other byte and word of every slot unchanged
    np.testing.assert_array_equal(kc_g, kc_x, err_msg=f"K codes {label}")
    np.testing.assert_array_equal(vc_g, vc_x, err_msg=f"V codes {label}")
    if qjl:
        np.testing.assert_array_equal(kx_g, kx_x, err_msg=f"QJL rows {label}")
    worst = 0.0
    for s, (sl, p) in enumerate(zip(case["slot"], case["pos"])):
        # 2. within the bound of the float64 attention over the slot's rows after the call
        ref, S, vmax, n = mr.sequence_reference(orc, case, after, s)
        r = ar.worst_ratio(out[s], ref, S, vmax, n)
        print(f"  {label} sequence {s} (slot {sl}, pos {p}): err / bound = {r:.4f}")
        assert r <= 1.0, f"{label} sequence {s} (slot {sl}, pos {p}): err / bound = {r:.3g}"
        worst = max(worst, r)
        # 3. the single-sequence launch on that slot alone: the same bits
        one = gpu.op_attention_tq(kt, case["q"][s], case["kc"][sl], case["vc"][sl], case["kx"][sl] if qjl else None, case["k_new"][s],
                                  case["v_new"][s], case["signs"], case["S"], case["scale"], p, n_splits)[0]
        assert np.array_equal(out[s].view(np.uint32), one.view(np.uint32)), f"{label} sequence {s} (slot {sl}, pos {p}) differs from the single launch"
    # 4. a second run: the same bits
    again = _run(gpu, case, n_splits)
    for a, b, what in zip((out, kc_g, vc_g, kx_g), again, ("out", "K codes", "V codes", "QJL rows")):
        if a is not None:
            assert np.array_equal(_bits(a), _bits(b)), f"{label}: {what} differ between two runs"
    return worst


@pytest.mark.parametrize("d,g", SHAPES)
@pytest.mark.parametrize("kv_type", mr.KV_TYPES, ids=mr.KV_IDS)
def test_decode_tq_multi(gpu, orc, kv_type, d, g):
    """n_seq 1 and 3 on 5 slots of 512 rows, two split counts, every position class of attention_tq_multi_ref.positions in some
    launch of each (attention_tq_multi_ref.launches), the last row of a slot on the highest slot."""
    worst = 0.0
    for si, n_splits in enumerate(mr.SPLITS):
        for li, (slot, pos, kind) in enumerate(mr.launches(d, n_splits)):
            rng = np.random.default_rng([kv_type, d, g, si, li])
            case = mr.make_case(orc, rng, kv_type, d, g, 5, slot, pos, mr.MAX_SEQ, kind)
            worst = max(worst, _check(gpu, orc, case, n_splits, f"type={kv_type} d={d} g={g} splits={n_splits} slot={slot} pos={pos} {kind}"))
    print(f"WORST tq_multi type={kv_type} d={d} g={g}: err / bound = {worst:.4f}")


@pytest.mark.parametrize("kv_type,d,g,n_splits", [(4, 128, 4, 3), (5, 64, 8, 2), (6, 128, 1, 2), (7, 64, 4, 3)], ids=mr.KV_IDS)
def test_decode_tq_multi_16_sequences(gpu, orc, kv_type, d, g, n_splits):
    """16 sequences on 16 slots (a permutation that is not the identity), the seven position classes spread over them, the last row of
    a slot on slot 15 among others."""
    P = mr.positions(d, n_splits)
    slot = [(5 * s + 3) % 16 for s in range(16)]
    pos = [P[(s + s // 7) % 7] for s in range(16)]
    pos[slot.index(15)] = P[6]
    assert sorted(set(pos)) == P and sorted(slot) == list(range(16)) and any(sl != s for s, sl in enumerate(slot))
    rng = np.random.default_rng([kv_type, d, g, 16])
    case = mr.make_case(orc, rng, kv_type, d, g, 16, slot, pos, mr.MAX_SEQ)
    worst = _check(gpu, orc, case, n_splits, f"type={kv_type} d={d} g={g} splits={n_splits} 16 sequences")
    print(f"WORST tq_multi16 type={kv_type} d={d} g={g}: err / bound = {worst:.4f}")


def test_tq_multi_refusals(pkg, gpu, orc):
    """Unsupported: a cache type that is not TurboQuant, a shape without a kernel (never another kernel).  InvalidArgument: a position
    at max_seq_len or below 0, a slot at n_slots, a slot listed twice, n_seq outside 1..16, a sign that is not +1 / -1."""
    rng = np.random.default_rng(5)

    def call(kv_type=5, d=64, g=4, n_slots=5, slot=(3, 0), pos=(7, 2), max_seq=32, as_type=None, pos_arg=None, slot_arg=None, sign=None):
        case = mr.make_case(orc, rng, kv_type, d, g, n_slots, slot, pos, max_seq)
        case["kv_type"] = kv_type if as_type is None else as_type
        case["pos"] = case["pos"] if pos_arg is None else list(pos_arg)
        case["slot"] = case["slot"] if slot_arg is None else list(slot_arg)
        if sign is not None:
            case["signs"][1, 1, 5] = sign
        return _run(gpu, case, 4)

    call()                                                     # (the well-formed calls pass)
    call(kv_type=6)
    for kw, variant in ((dict(as_type=0), "Unsupported"), (dict(as_type=1), "Unsupported"), (dict(as_type=8), "Unsupported"),
                        (dict(d=96), "Unsupported"), (dict(g=3), "Unsupported"),
                        (dict(pos_arg=(7, 32)), "InvalidArgument"), (dict(pos_arg=(-1, 2)), "InvalidArgument"),
                        (dict(slot_arg=(3, 5)), "InvalidArgument"), (dict(slot_arg=(3, 3)), "InvalidArgument"),
                        (dict(n_slots=17, slot=tuple(range(17)), pos=(1,) * 17), "InvalidArgument"),
                        (dict(slot=(), pos=()), "InvalidArgument"), (dict(sign=0.5), "InvalidArgument")):
        with pytest.raises(pkg.BackendError) as ei:
            call(**kw)
        assert ei.value.variant == variant, (kw, ei.value.variant)


# ---- wo's input as the attention launches leave it
def _check_image(img, out, what):
    """An image against float64 of the launch's own f32 output (elements and chunk sums; the merges write no sums of squares)."""
    o = np.asarray(out, np.float32).reshape(-1)
    x, xs = mm.xq_decode(img, o.size)
    (v, ev), (sums, es), _ = mm.image_ref(o)
    ex, exs = np.abs(x - v), np.abs(xs - sums)
    assert np.isfinite(x).all() and (ex <= ev).all(), f"{what} elements: worst err / bound = {float((ex / ev).max()):.3g}"
    assert np.isfinite(xs).all() and (exs <= es).all(), f"{what} chunk sums: worst err / bound = {float((exs / es).max()):.3g}"


def _check_multi_images(imgs, out, what):
    """n_seq + 1 images: sequence s's at index s (no other sequence's output fits it), the one behind the last still the poison."""
    n_seq = out.shape[0]
    assert imgs.shape[0] == n_seq + 1
    for s in range(n_seq):
        _check_image(imgs[s], out[s], f"{what} sequence {s}")
        x, _ = mm.xq_decode(imgs[s], out[s].size)
        for o in range(n_seq):
            if o != s:   # (the outputs differ by far more than an image's half step: a swapped pair cannot pass the check above)
                ev = mm.image_ref(out[o].reshape(-1))[0][1]
                assert (np.abs(x - out[o].reshape(-1).astype(np.float64)) > 1e3 * ev).any(), f"{what}: outputs {s} and {o} do not differ"
    assert (np.ascontiguousarray(imgs[n_seq]).view(np.uint32) == POISON).all(), f"{what}: the image behind the last sequence was written"


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: the output changes with the image"


@pytest.mark.parametrize("d,g", [(64, 1), (128, 4)])
def test_attention_images(gpu, orc, d, g):
    """Every attention entry point with image=True: the f32 output keeps its bits, the image holds that output (matvec_multi_ref.image_ref),
    the multi-sequence launches put sequence s's image at index s and leave the one behind the last alone.  (64, 1): n_heads * d = 128,
    half a record."""
    n_splits, max_seq = 3, 256
    slot, pos = [3, 0, 4], [1, 200, 40]
    tq_type, kv8_type = (5, 1) if d == 64 else (6, 2)
    rng = np.random.default_rng([d, g, 77])
    # f32 caches: 5 slots, rows past a sequence's position NaN
    n_heads = mr.N_KV * g
    q = rng.standard_normal((3, n_heads, d)).astype(np.float32)
    kf = np.full((5, mr.N_KV, max_seq, d), np.nan, np.float32)
    vf = np.full((5, mr.N_KV, max_seq, d), np.nan, np.float32)
    for sl, p in zip(slot, pos):
        kf[sl, :, :p + 1] = rng.standard_normal((mr.N_KV, p + 1, d))
        vf[sl, :, :p + 1] = rng.standard_normal((mr.N_KV, p + 1, d))
    scale = float(1.0 / np.sqrt(d))
    for s, (sl, p) in enumerate(zip(slot, pos)):
        for path, name in ((gpu.ATTN_SPLIT, "decode split"), (gpu.ATTN_DIRECT, "decode direct")):
            out, img = gpu.op_attention_decode(path, q[s], kf[sl], vf[sl], scale, p, n_splits, image=True)
            _same(out, gpu.op_attention_decode(path, q[s], kf[sl], vf[sl], scale, p, n_splits), f"{name} pos={p}")
            _check_image(img, out, f"{name} pos={p}")
    out, imgs = gpu.op_attention_decode_multi(q, kf, vf, scale, pos, slot, n_splits, image=True)
    _same(out, gpu.op_attention_decode_multi(q, kf, vf, scale, pos, slot, n_splits), "decode_multi")
    _check_multi_images(imgs, out, "decode_multi")
    # byte caches
    c8 = m8.make_case(orc, rng, kv8_type, d, g, 5, slot, pos, max_seq)
    args = (kv8_type, c8["q"], c8["kb"], c8["vb"], c8["ks"], c8["vs"], c8["k_new"], c8["v_new"], c8["scale"], pos, slot, n_splits)
    res = gpu.op_attention_kv8_multi(*args, image=True)
    plain = gpu.op_attention_kv8_multi(*args)
    assert len(res) == len(plain) + 1
    for a, b in zip(res, plain):
        if a is not None:
            _same(a, b, "kv8_multi")
    _check_multi_images(res[-1], res[0], "kv8_multi")
    for s, (sl, p) in enumerate(zip(slot, pos)):
        i8 = kv8_type == 1
        args = (kv8_type, c8["q"][s], c8["kb"][sl], c8["vb"][sl], c8["ks"][sl] if i8 else None, c8["vs"][sl] if i8 else None, c8["k_new"][s],
                c8["v_new"][s], c8["scale"], p, n_splits)
        res = gpu.op_attention_kv8(*args, image=True)
        _same(res[0], gpu.op_attention_kv8(*args)[0], f"kv8 pos={p}")
        _check_image(res[-1], res[0], f"kv8 pos={p}")
    # TurboQuant caches
    ct = mr.make_case(orc, rng, tq_type, d, g, 5, slot, pos, max_seq)
    res = _run(gpu, ct, n_splits, image=True)
    plain = _run(gpu, ct, n_splits)
    assert len(res) == len(plain) + 1
    for a, b in zip(res, plain):
        if a is not None:
            _same(a, b, "tq_multi")
    _check_multi_images(res[-1], res[0], "tq_multi")
    for s, (sl, p) in enumerate(zip(slot, pos)):
        args = (tq_type, ct["q"][s], ct["kc"][sl], ct["vc"][sl], ct["kx"][sl] if ct["qjl"] else None, ct["k_new"][s], ct["v_new"][s], ct["signs"],
                ct["S"], ct["scale"], p, n_splits)
        res = gpu.op_attention_tq(*args, image=True)
        _same(res[0], gpu.op_attention_tq(*args)[0], f"tq pos={p}")
        _check_image(res[-1], res[0], f"tq pos={p}")


def test_any_shape_path_has_no_image(pkg, gpu):
    """lgh_op_attention_decode path 2 (any head size / group size) writes f32 only: asked for an image it answers InvalidArgument."""
    rng = np.random.default_rng(3)
    q = rng.standard_normal((6, 96)).astype(np.float32)
    k = rng.standard_normal((2, 16, 96)).astype(np.float32)
    gpu.op_attention_decode(gpu.ATTN_ANY, q, k, k, 0.1, 7)
    with pytest.raises(pkg.BackendError) as ei:
        gpu.op_attention_decode(gpu.ATTN_ANY, q, k, k, 0.1, 7, image=True)
    assert ei.value.variant == "InvalidArgument"
