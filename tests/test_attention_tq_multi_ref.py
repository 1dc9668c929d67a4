"""The per-sequence reference of the multi-sequence TurboQuant attention tests (tests/attention_tq_multi_ref.py), on the CPU: it is
attention_ref.tq_decode on the slot a sequence names, and the bound the GPU test applies (attention_ref.bound, unchanged) sees the
mistakes a multi-sequence kernel can make that a single-sequence one cannot, each by a factor of at least FACTOR."""
import numpy as np
import pytest

import attention_ref as ar
import attention_tq_multi_ref as mr

FACTOR = 5.0
SHAPES = [(64, 1), (128, 4)]


def test_positions_fit():
    """All seven position classes are distinct rows of a MAX_SEQ-row slot, for both head sizes and both split counts; 2 * stride - 1
    is the last position whose rows all lie in a workgroup's first batch (two passes), 2 * stride the first that leaves it."""
    for d in (64, 128):
        for n_splits in mr.SPLITS:
            st = mr.stride_of(d, n_splits)
            assert st == n_splits * 4 * (1024 // d)
            P = mr.positions(d, n_splits, mr.MAX_SEQ)
            assert P == [0, 1, st - 1, st, 2 * st - 1, 2 * st, mr.MAX_SEQ - 1] and len(set(P)) == 7 and max(P) == mr.MAX_SEQ - 1
            seen = sorted(p for slot, pos, _ in mr.launches(d, n_splits) for p in pos)
            assert sorted(set(seen)) == P                             # every class in some launch
            assert all(max(slot) == slot[pos.index(P[6])] for slot, pos, _ in mr.launches(d, n_splits) if P[6] in pos)


@pytest.mark.parametrize("kv_type", mr.KV_TYPES, ids=mr.KV_IDS)
def test_reference_is_tq_decode_on_the_named_slot(orc, kv_type):
    d, g, n_splits = 128, 4, 3
    P = mr.positions(d, n_splits)
    rng = np.random.default_rng([kv_type, d, g])
    case = mr.make_case(orc, rng, kv_type, d, g, 5, [3, 0, 4], [P[3], P[5], P[6]], mr.MAX_SEQ)
    bits, qjl, signs = case["bits"], case["qjl"], case["signs"]
    after = kc, vc, kx = mr.after_call(orc, case)
    for s, (sl, p) in enumerate(zip(case["slot"], case["pos"])):
        ref, S, vmax, n = mr.sequence_reference(orc, case, after, s)
        assert n == p + 1 and np.isfinite(ref).all()          # no NaN norm entered
        # the slot alone, as the single-sequence test builds it: stored rows, then the oracle's compression of the staged rows at p
        k1, v1 = case["kc"][sl].copy(), case["vc"][sl].copy()
        x1 = case["kx"][sl].copy() if qjl else None
        for h in range(case["n_kv"]):
            if qjl:
                codes, qb, norm = orc.tq_compress_qjl(case["k_new"][s, h], bits, signs[h, 0], case["S"][h])
                k1[h, p] = codes
                x1[h, p] = np.concatenate([qb.view(np.uint32), np.float32([norm]).view(np.uint32)])
            else:
                k1[h, p] = orc.tq_compress(case["k_new"][s, h], bits, signs[h, 0])
            v1[h, p] = orc.tq_compress(case["v_new"][s, h], bits, signs[h, 1])
        want, s_mag, vm = ar.tq_decode(orc, case["q"][s], k1, v1, bits, signs, case["scale"], n, x1, case["S"])
        np.testing.assert_array_equal(ref, want)
        assert S == s_mag and vmax == vm
        # the poison is what the module says: V rows of top centroids from the stale row on, NaN norms (QJL)
        assert (case["vc"][sl, :, p:] == 0xFF).all() and (case["vc"][sl, :, :p] != 0xFF).any()
        top = ar.tq_values(orc, case["vc"][sl, 0, p], bits, d, signs[0, 1])
        cen = float(orc.tq_codebook(d, bits)[0].max())
        assert abs(abs(top[0]) - cen * np.sqrt(d)) < 1e-6 and np.abs(top[1:]).max() < 1e-6
        assert abs(cen * np.sqrt(d) - (1.51 if bits == 2 else 2.15)) < 0.01
        if qjl:
            assert np.isnan(ar.qjl_norms(case["kx"][sl, :, p:], d)).all() and np.isfinite(ar.qjl_norms(kx[sl, :, :p + 1], d)).all()
    unnamed = [sl for sl in range(5) if sl not in case["slot"]]
    assert unnamed and all((case["vc"][sl] == 0xFF).all() for sl in unnamed)
    # every byte and word outside the written rows is the input's; the written rows changed
    written = np.zeros(kc.shape[:3], bool)
    for sl, p in zip(case["slot"], case["pos"]):
        written[sl, :, p] = True
    np.testing.assert_array_equal(kc[~written], case["kc"][~written])
    np.testing.assert_array_equal(vc[~written], case["vc"][~written])
    assert (vc[written] != 0xFF).any()
    if qjl:
        np.testing.assert_array_equal(kx[~written], case["kx"][~written])


def _mistakes(orc, case, after, rolled, s):
    """(name, K side only, the reference with the mistake planted) for sequence s."""
    n_seq, p, sl = len(case["slot"]), case["pos"][s], case["slot"][s]
    others = [o for o in range(n_seq) if o != s]
    ref = lambda **kw: mr.sequence_reference(orc, case, kw.pop("after", after), s, **kw)[0]
    for o in others:
        # another sequence's slot, read up to this sequence's position (rows from that slot's own position on are poisoned)
        yield f"slot of sequence {o}", False, ref(slot=case["slot"][o])
        yield f"query of sequence {o}", True, ref(q=case["q"][o])
        if case["qjl"]:   # K codes of the right slot, QJL rows of another: x_stride or the kx offset wrong
            yield f"QJL rows of sequence {o}'s slot", True, ref(x_slot=case["slot"][o])
    if others:
        yield "k_new / v_new of another sequence", False, ref(after=rolled)
    if sl != s:
        yield "slot = s", False, ref(slot=s)
    if p + 1 < case["max_seq"]:          # (the last row of a slot has no row behind it in the slot)
        yield "one row too many", False, ref(pos=p + 1)
    if p >= 1:
        yield "one row too few", False, ref(pos=p - 1)
    yield "the stale row at pos", False, ref(after=mr.before_call(case))
    yield "the neighbouring kv head's signs", False, ref(signs=np.roll(case["signs"], 1, axis=0))


@pytest.mark.parametrize("d,g", SHAPES)
@pytest.mark.parametrize("kv_type", mr.KV_TYPES, ids=mr.KV_IDS)
def test_planted_mistakes_exceed_the_bound(orc, kv_type, d, g):
    """`normal` cases at every position class for both split counts (the GPU test's launches): each planted mistake moves the
    reference by at least FACTOR = 5 bounds.  Exempt, exactly: mistakes that change only K (another sequence's query, another slot's
    QJL rows) at pos = 0, where the one visible row's weight is 1 whatever its score: there they move nothing at all.
    Smallest factor over all of these cases: 13.9 (tq3_qjl, d = 64, g = 1: another slot's QJL rows at position 384); one row too
    few, the weakest on the types without QJL, is 19.5 at position 511 (tq3, d = 128, g = 4).  With staged rows of N(0, 1) alone
    that one measured 2.9 (tq2_qjl) to 10 — hence make_case's staged rows.  (Staged K rows alone from another sequence, V rows
    right, change one score of pos + 1 and are not planted here: the GPU test sees that one exactly, in the stored row.)"""
    smallest = (np.inf, None)
    for si, n_splits in enumerate(mr.SPLITS):
        for li, (slot, pos, _) in enumerate(mr.launches(d, n_splits)):
            rng = np.random.default_rng([kv_type, d, g, si, li, 1])
            case = mr.make_case(orc, rng, kv_type, d, g, 5, slot, pos, mr.MAX_SEQ, "normal")
            after = mr.after_call(orc, case)
            rolled = mr.after_call(orc, case, np.roll(case["k_new"], 1, axis=0), np.roll(case["v_new"], 1, axis=0))
            for s in range(len(slot)):
                ref, S, vmax, n = mr.sequence_reference(orc, case, after, s)
                assert ar.worst_ratio(ref.astype(np.float32), ref, S, vmax, n) <= 1.0      # (an f32 rounding of the truth passes)
                for name, k_only, bad in _mistakes(orc, case, after, rolled, s):
                    r = ar.worst_ratio(bad, ref, S, vmax, n)
                    if k_only and pos[s] == 0:
                        assert r == 0.0, (name, slot, pos, s, r)       # (nothing to see: the exemption is exact)
                        continue
                    assert r >= FACTOR, (name, slot, pos, s, r)
                    if r < smallest[0]:
                        smallest = (r, f"{name} slot={slot} pos={pos} s={s} splits={n_splits}")
    print(f"SMALLEST planted factor type={kv_type} d={d} g={g}: {smallest[0]:.1f} ({smallest[1]})")
