"""The per-sequence reference of the multi-sequence byte-cache attention tests (tests/attention_kv8_multi_ref.py), on the CPU: it is
attention_ref.decode on the slot a sequence names, and the bound the GPU test applies sees the mistakes a multi-sequence kernel can
make that a single-sequence one cannot — another sequence's slot, a position off by one, another sequence's staged row."""
import numpy as np
import pytest

import attention_ref as ar
import attention_kv8_multi_ref as mr


def _case(orc, kv_type, d=128, g=4):
    rng = np.random.default_rng([kv_type, d, g])
    n_splits = 5
    st = mr.stride_of(d, n_splits)
    return mr.make_case(orc, rng, kv_type, d, g, 5, [3, 0, 4], [st, 4 * st + 1, 300], 384)


@pytest.mark.parametrize("kv_type", [1, 2, 3], ids=["int8", "fp8_e4m3", "fp8_e5m2"])
def test_reference_is_decode_on_the_named_slot(orc, kv_type):
    case = _case(orc, kv_type)
    after = mr.after_call(orc, case)
    kb, vb, ks, vs = after
    for s, (sl, p) in enumerate(zip(case["slot"], case["pos"])):
        ref, S, vmax, n = mr.sequence_reference(orc, case, after, s)
        assert n == p + 1 and np.isfinite(ref).all()          # no poisoned row entered
        # the slot alone, as the single-sequence test builds it: stored rows 0..p-1, then the oracle's encoding of the staged row
        K = np.empty((case["n_kv"], n, case["d"]))
        V = np.empty_like(K)
        for h in range(case["n_kv"]):
            K[h, :p] = mr.values(orc, kv_type, case["kb"][sl, h, :p], case["ks"][sl, h, :p] if kv_type == 1 else None)
            V[h, :p] = mr.values(orc, kv_type, case["vb"][sl, h, :p], case["vs"][sl, h, :p] if kv_type == 1 else None)
            b, sc = mr.encode_row(orc, kv_type, case["k_new"][s, h])
            K[h, p] = mr.values(orc, kv_type, b, sc)
            b, sc = mr.encode_row(orc, kv_type, case["v_new"][s, h])
            V[h, p] = mr.values(orc, kv_type, b, sc)
        np.testing.assert_array_equal(ref, ar.decode(case["q"][s], K, V, case["scale"], n))
        assert S == ar.magnitude(case["q"][s], K, case["scale"], n) and vmax == float(np.abs(V).max())
    # every byte and scale outside the written rows is the input's
    written = np.zeros(kb.shape[:3], bool)
    for sl, p in zip(case["slot"], case["pos"]):
        written[sl, :, p] = True
    np.testing.assert_array_equal(kb[~written], case["kb"][~written])
    np.testing.assert_array_equal(vb[~written], case["vb"][~written])
    if kv_type == 1:
        np.testing.assert_array_equal(ks[~written].view(np.uint32), case["ks"][~written].view(np.uint32))
        assert np.isfinite(ks[written]).all() and np.isfinite(vs[written]).all()
    else:
        assert (kb[written] != case["kb"][written]).any()


@pytest.mark.parametrize("kv_type", [1, 2, 3], ids=["int8", "fp8_e4m3", "fp8_e5m2"])
def test_planted_mistakes_exceed_the_bound(orc, kv_type):
    case = _case(orc, kv_type)
    after = mr.after_call(orc, case)
    n_seq = len(case["slot"])
    rolled = mr.after_call(orc, case, np.roll(case["k_new"], 1, axis=0), np.roll(case["v_new"], 1, axis=0))
    for s in range(n_seq):
        ref, S, vmax, n = mr.sequence_reference(orc, case, after, s)
        assert ar.worst_ratio(ref.astype(np.float32), ref, S, vmax, n) <= 1.0      # (an f32 rounding of the truth passes)
        other = (s + 1) % n_seq
        # another sequence's slot, read up to this sequence's position (rows past that slot's own position are poisoned) or up to its own
        for p in (case["pos"][s], case["pos"][other]):
            bad = mr.sequence_reference(orc, case, after, s, slot=case["slot"][other], pos=p)[0]
            assert ar.worst_ratio(bad, ref, S, vmax, n) > 1.0, ("slot", s, p)
        # a position off by one: the staged row dropped, or the poisoned row behind it read
        for p in (case["pos"][s] - 1, case["pos"][s] + 1):
            bad = mr.sequence_reference(orc, case, after, s, pos=p)[0]
            assert ar.worst_ratio(bad, ref, S, vmax, n) > 1.0, ("pos", s, p)
        # the staged row of the wrong sequence
        bad = mr.sequence_reference(orc, case, rolled, s)[0]
        assert ar.worst_ratio(bad, ref, S, vmax, n) > 1.0, ("staged", s)
