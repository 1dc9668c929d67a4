"""tests/step_ref.py on the CPU: on the inputs tests/test_gpu_step_launches.py uses, each likely mistake of a launch — applied to the
reference's own output — lands outside the check the GPU test applies (ratio > 1, or different bits where the check is exact), and the
unmutated output passes it.  So those inputs can tell the kernels from their mistakes."""
import numpy as np
import pytest

import matvec_multi_ref as mm
import matvec_ref as mr
import step_ref as sr


def _tables(pkg, orc, tname, hidden):
    return sr.table(tname, hidden, orc, pkg.synth.fill_tensor)


@pytest.mark.parametrize("tname", sr.EMBED_TYPES)
def test_embedding_mistakes_are_caught(pkg, orc, tname):
    for hidden in sr.embed_hiddens(tname):
        raw = _tables(pkg, orc, tname, hidden)
        assert raw.size == orc.nbytes_for(sr.TYPE[tname], sr.VOCAB * hidden)
        nw = sr.norm_weight(hidden, 3)
        rows = {t: sr.embed_row(orc, tname, raw, hidden, t) for t in range(sr.VOCAB)}
        whole = orc.dequantize(sr.TYPE[tname], raw, sr.VOCAB * hidden).reshape(sr.VOCAB, hidden)
        for t in sr.EMBED_TOKENS:
            row = rows[t]
            assert np.all(np.isfinite(row)) and np.any(row != 0)
            assert np.array_equal(sr.bits(row), sr.bits(whole[t]))                       # a row's bytes dequantize as the table's do
            # the row of token + 1 (and of every other token): different bits
            for other in range(sr.VOCAB):
                assert other == t or not np.array_equal(sr.bits(rows[other]), sr.bits(row)), (t, other)
            if hidden % 256:
                continue
            (v, _), (sums, _), (sq, _) = mm.image_ref(row, nw)
            assert max(sr.decoded_ratios(v, sums, sq, row, nw)) <= 1.0
            # the image built with v instead of v * norm_w; of the neighbouring row; ssq of v * norm_w instead of v
            (v0, _), (sums0, _), _ = mm.image_ref(row, None)
            assert sr.decoded_ratios(v0, sums, sq, row, nw)[0] > 1 and sr.decoded_ratios(v, sums0, sq, row, nw)[1] > 1
            (v1, _), (sums1, _), (sq1, _) = mm.image_ref(rows[(t + 1) % sr.VOCAB], nw)
            assert all(r > 1 for r in sr.decoded_ratios(v1, sums1, sq1, row, nw))
            wrong_sq = ((row.astype(np.float64) * nw) ** 2).reshape(-1, 16).sum(axis=1)
            assert sr.decoded_ratios(v, sums, wrong_sq, row, nw)[2] > 1
            # what was never written (FILL) is outside every bound
            junk = np.full(hidden * 4, sr.FILL, np.uint8).view(np.float32)
            assert all(r > 1 for r in sr.decoded_ratios(junk, junk[:hidden // 16], junk[:hidden // 16], row, nw))


def test_sequence_strides_are_told_apart(pkg, orc):
    """Images lie xq_bytes(hidden) apart either way; the partials lie hidden / 16 + 64 apart, and a launch that put sequence s's at
    s * (hidden / 16) shows from sequence 1 on."""
    hidden, tname = 512, "Q4_K"
    raw = _tables(pkg, orc, tname, hidden)
    nw = sr.norm_weight(hidden, 3)
    toks = [0, 17, 17, sr.VOCAB - 1]
    rows = [sr.embed_row(orc, tname, raw, hidden, t) for t in toks]
    refs = [mm.image_ref(r, nw) for r in rows]
    per_seq = [r[2][0] for r in refs]
    good = sr.pack_ssq(per_seq, hidden // 16 + 64, len(toks) + 1)
    bad = sr.pack_ssq(per_seq, hidden // 16, len(toks) + 1)
    for s in range(len(toks)):
        v, sums = refs[s][0][0], refs[s][1][0]
        assert sr.decoded_ratios(v, sums, good[s], rows[s], nw)[2] <= 1.0
        assert s == 0 or sr.decoded_ratios(v, sums, bad[s], rows[s], nw)[2] > 1
    assert sr.filled(good[len(toks)]) and sr.filled(good[:, hidden // 16:])
    assert not sr.filled(bad[:len(toks), hidden // 16:])            # ... and it wrote where no sequence's partials belong


QKV_ALL = [(c, False) for c in sr.QKV_UNFUSED] + [(c, True) for c in sr.QKV_FUSED]


@pytest.mark.parametrize("hd,nh,nkv", sr.QKV_SHAPES)
@pytest.mark.parametrize("case,fused", QKV_ALL)
def test_qkv_mistakes_are_caught(pkg, orc, case, fused, hd, nh, nkv):
    types, neox, with_bias = case
    ws, nw, biases, rows = sr.qkv_inputs(types, hd, nh, nkv, with_bias, orc)
    for pi, pos in enumerate(sr.QKV_POS):
        x = sr.qkv_x(pi, with_bias, pos)
        (q, eq), (k, ek), (v, ev) = sr.qkv_ref(orc, types, ws, nw, biases, rows, x, pos, hd, neox)
        assert mm.ratio(q, q, eq) == 0.0 and np.all(eq > 0) and np.all(ek > 0) and np.all(ev > 0)
        # the other pairing (at position 0 every rotation is the identity: nothing to tell apart there)
        (q2, _), (k2, _), _ = sr.qkv_ref(orc, types, ws, nw, biases, rows, x, pos, hd, not neox)
        if pos:
            assert mm.ratio(q2, q, eq) > 1 and mm.ratio(k2, k, ek) > 1, (types, pos)
        else:
            assert np.array_equal(q2, q)
        # the bias added after the rotation
        if with_bias and pos:
            (q3, _), (k3, _), _ = sr.qkv_ref(orc, types, ws, nw, biases, rows, x, pos, hd, neox, bias_after_rope=True)
            assert mm.ratio(q3, q, eq) > 1 and mm.ratio(k3, k, ek) > 1
        # the K row rotated for position pos + 1, and stored one row further
        _, (k4, _), _ = sr.qkv_ref(orc, types, ws, nw, biases, rows, x, pos, hd, neox, pos_shift=1)
        assert mm.ratio(k4, k, ek) > 1
        cache = sr.nan_cache(nkv, hd)
        cache[:, pos, :] = k.reshape(nkv, hd)
        assert sr.cache_failures(cache, pos, k, ek, "K") == []
        if pos + 1 < sr.MAX_SEQ:
            moved = sr.nan_cache(nkv, hd)
            moved[:, pos + 1, :] = k.reshape(nkv, hd)
            assert len(sr.cache_failures(moved, pos, k, ek, "K")) == 2
        # K and V swapped, a head's rows swapped
        assert mm.ratio(v, k, ek) > 1
        assert mm.ratio(np.roll(k.reshape(nkv, hd), 1, axis=0).reshape(-1), k, ek) > 1


@pytest.mark.parametrize("tg,tu", sr.GATEUP_CASES)
def test_gateup_mistakes_are_caught(pkg, orc, tg, tu):
    wg, wu, nw = sr.gateup_inputs(tg, tu, orc)
    for ai, act in enumerate(mr.ACT_KINDS):
        x = mr.activation(act, sr.FFN_HIDDEN, 40 + ai)
        y, e = sr.gateup_ref(orc, tg, wg, tu, wu, nw, x)
        assert np.all(np.isfinite(y)) and np.all(e > 0)
        # gate and up exchanged; silu_mul reading the gate's output, or the up's, on both sides
        y2, _ = sr.gateup_ref(orc, tu, wu, tg, wg, nw, x)
        assert mm.ratio(y2, y, e) > 1
        fam_parts = [sr.gateup_ref(orc, t, w, t, w, nw, x) for t, w in ((tg, wg), (tu, wu))]
        assert mm.ratio(fam_parts[0][0], y, e) > 1 and mm.ratio(fam_parts[1][0], y, e) > 1


@pytest.mark.parametrize("n", sr.ARGMAX_N)
def test_argmax_cases_are_ties_and_first_maximal_differs(orc, n):
    rows = sr.argmax_rows(n, n)
    names = [name for name, _, _ in rows]
    assert len(set(names)) == len(names) == 9
    for name, row, is_tie in rows:
        assert not np.any(np.isnan(row))
        want = sr.argmax_last(row)
        assert want == orc.argmax_last(row), (n, name)
        assert is_tie == (int(np.sum(row == row.max())) > 1), (n, name)
        assert row[want] == row.max() and not np.any(row[want + 1:] == row.max())
        if is_tie:
            assert sr.argmax_first(row) != want, (n, name)           # the first-maximal rule gives another token
    ties = {name for name, _, t in rows if t}
    if n >= 16384:
        assert ties == set(names) - {"last index alone"}
        byname = {name: row for name, row, _ in rows}
        wg = lambda i: (i // 256) % 64
        i = np.nonzero(byname["two lanes of one workgroup"] == sr.PEAK)[0]
        assert len(i) == 2 and wg(i[0]) == wg(i[1]) and i[0] // 256 == i[1] // 256
        i = np.nonzero(byname["two workgroups"] == sr.PEAK)[0]
        assert len({wg(j) for j in i}) == 3
        if n > 5 + 16384:
            i = np.nonzero(byname["one thread twice"] == sr.PEAK)[0]
            assert list(i) == [5, 5 + 16384]                         # one thread of one workgroup, two trips of its loop
    assert sr.argmax_last(np.full(n, -np.inf, np.float32)) == n - 1
    # sequences of a batch have their maxima at different indices: an arg-max that reads another sequence's row or parts shows
    for n_seq in (3, 16):
        for batch in sr.argmax_batches(n, n_seq, n):
            assert batch.shape == (n_seq, n)
            toks = [sr.argmax_last(r) for r in batch]
            assert n == 1 or len(set(toks)) > 1
