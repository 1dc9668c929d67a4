"""attn_partial_q8_kernel<D,G,4,FMT,MULTI> + attn_combine_kernel<MULTI> through lgh_op_attention_kv8_multi: the multi-sequence decode
step's attention over int8 / FP8 cache slots, against the float64 restatement (tests/attention_ref.py through
tests/attention_kv8_multi_ref.py) and, bit for bit, against the single-sequence launch (lgh_op_attention_kv8) on each slot alone.

One launch mixes sequences whose positions put them on different paths of the kernel's loop (only the staged row; fewer rows than
workgroups; one or several batches of kAhead passes), on slots that are not the identity with at least one slot unused; everything
a sequence must not read is poisoned (attention_kv8_multi_ref.make_case).  Each test prints its worst error as a fraction of the
bound."""
import numpy as np
import pytest

import attention_ref as ar
import attention_kv8_multi_ref as mr

pytestmark = pytest.mark.gpu

SHAPES = [(d, g) for d in (64, 128) for g in (1, 4, 8)]
KV_TYPES = [1, 2, 3]
KV_IDS = ["int8", "fp8_e4m3", "fp8_e5m2"]
MAX_SEQ = 384
SPLITS = (2, 5)


def _run(gpu, case, n_splits):
    return gpu.op_attention_kv8_multi(case["kv_type"], case["q"], case["kb"], case["vb"], case["ks"], case["vs"], case["k_new"], case["v_new"],
                                      case["scale"], case["pos"], case["slot"], n_splits)


def _check(gpu, orc, case, n_splits, label):
    """Every assertion of one launch; -> the worst err / bound of its sequences."""
    kt = case["kv_type"]
    out, kb_g, vb_g, ks_g, vs_g = _run(gpu, case, n_splits)
    kb_x, vb_x, ks_x, vs_x = after = mr.after_call(orc, case)
    # rows pos[s] of slots slot[s] as the oracle encodes the staged rows, every other byte and scale of every slot unchanged
    np.testing.assert_array_equal(kb_g, kb_x, err_msg=f"K bytes {label}")
    np.testing.assert_array_equal(vb_g, vb_x, err_msg=f"V bytes {label}")
    if kt == 1:
        np.testing.assert_array_equal(ks_g.view(np.uint32), ks_x.view(np.uint32), err_msg=f"K scales {label}")
        np.testing.assert_array_equal(vs_g.view(np.uint32), vs_x.view(np.uint32), err_msg=f"V scales {label}")
    worst = 0.0
    for s, (sl, p) in enumerate(zip(case["slot"], case["pos"])):
        ref, S, vmax, n = mr.sequence_reference(orc, case, after, s)
        r = ar.worst_ratio(out[s], ref, S, vmax, n)
        assert r <= 1.0, f"{label} sequence {s} (slot {sl}, pos {p}): err / bound = {r:.3g}"
        worst = max(worst, r)
        # the single-sequence launch on that slot alone: the same bits
        one = gpu.op_attention_kv8(kt, case["q"][s], case["kb"][sl], case["vb"][sl], case["ks"][sl] if kt == 1 else None,
                                   case["vs"][sl] if kt == 1 else None, case["k_new"][s], case["v_new"][s], case["scale"], p, n_splits)[0]
        assert np.array_equal(out[s].view(np.uint32), one.view(np.uint32)), f"{label} sequence {s} (slot {sl}, pos {p}) differs from the single launch"
    again = _run(gpu, case, n_splits)
    for a, b, what in zip((out, kb_g, vb_g, ks_g, vs_g), again, ("out", "K bytes", "V bytes", "K scales", "V scales")):
        if a is not None:
            assert np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint8), b.view(np.uint32 if b.dtype == np.float32 else np.uint8)), \
                f"{label}: {what} differ between two runs"
    return worst


@pytest.mark.parametrize("d,g", SHAPES)
@pytest.mark.parametrize("kv_type", KV_TYPES, ids=KV_IDS)
def test_decode_kv8_multi(gpu, orc, kv_type, d, g):
    """n_seq 1 and 3 on 5 slots, two split counts, every position class of attention_kv8_multi_ref.positions in some launch."""
    worst = 0.0
    for si, n_splits in enumerate(SPLITS):
        P = mr.positions(d, n_splits)
        launches = [([3, 0, 4], [P[0], P[4], P[2]], "normal"), ([1, 4, 2], [P[3], P[1], P[5]], "hot"),
                    ([2], [P[4]], "hot"), ([4], [P[0]], "normal"), ([3], [P[5]], "normal")]
        for li, (slot, pos, kind) in enumerate(launches):
            rng = np.random.default_rng([kv_type, d, g, si, li])
            case = mr.make_case(orc, rng, kv_type, d, g, 5, slot, pos, MAX_SEQ, kind)
            worst = max(worst, _check(gpu, orc, case, n_splits, f"type={kv_type} d={d} g={g} splits={n_splits} slot={slot} pos={pos} {kind}"))
    print(f"WORST kv8_multi type={kv_type} d={d} g={g}: err / bound = {worst:.4f}")


@pytest.mark.parametrize("kv_type,d,g,n_splits", [(1, 128, 4, 8), (2, 64, 8, 5), (3, 128, 1, 2)], ids=KV_IDS)
def test_decode_kv8_multi_16_sequences(gpu, orc, kv_type, d, g, n_splits):
    """16 sequences on 16 slots (a permutation that is not the identity), the six position classes spread over them."""
    P = mr.positions(d, n_splits)
    slot = [(5 * s + 3) % 16 for s in range(16)]
    pos = [P[(s + s // 6) % 6] for s in range(16)]
    rng = np.random.default_rng([kv_type, d, g, 16])
    case = mr.make_case(orc, rng, kv_type, d, g, 16, slot, pos, MAX_SEQ)
    worst = _check(gpu, orc, case, n_splits, f"type={kv_type} d={d} g={g} splits={n_splits} 16 sequences")
    print(f"WORST kv8_multi16 type={kv_type} d={d} g={g}: err / bound = {worst:.4f}")


def test_kv8_multi_refusals(pkg, gpu, orc):
    """Unsupported: a cache type outside int8 / FP8, a shape without a kernel (never another kernel).  InvalidArgument: a position at
    max_seq_len, a slot at n_slots, a slot listed twice, n_seq outside 1..16."""
    rng = np.random.default_rng(5)

    def call(kv_type=1, d=64, g=4, n_slots=5, slot=(3, 0), pos=(7, 2), max_seq=32, as_type=None, pos_arg=None, slot_arg=None):
        case = mr.make_case(orc, rng, kv_type, d, g, n_slots, slot, pos, max_seq)
        case["kv_type"] = kv_type if as_type is None else as_type
        case["pos"] = case["pos"] if pos_arg is None else list(pos_arg)
        case["slot"] = case["slot"] if slot_arg is None else list(slot_arg)
        return _run(gpu, case, 4)

    call()                                                     # (the well-formed call passes)
    for kw, variant in ((dict(as_type=0), "Unsupported"), (dict(as_type=4), "Unsupported"), (dict(as_type=8), "Unsupported"),
                        (dict(d=96), "Unsupported"), (dict(g=3), "Unsupported"), (dict(d=256, g=1), "Unsupported"),
                        (dict(pos_arg=(7, 32)), "InvalidArgument"), (dict(pos_arg=(-1, 2)), "InvalidArgument"),
                        (dict(slot_arg=(3, 5)), "InvalidArgument"), (dict(slot_arg=(3, 3)), "InvalidArgument"),
                        (dict(n_slots=17, slot=tuple(range(17)), pos=(1,) * 17), "InvalidArgument"),
                        (dict(slot=(), pos=()), "InvalidArgument")):
        with pytest.raises(pkg.BackendError) as ei:
            call(**kw)
        assert ei.value.variant == variant, (kw, ei.value.variant)
