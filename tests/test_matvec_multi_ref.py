"""CPU tests of tests/matvec_multi_ref.py: the grouping restatement, and mutation tests — on the inputs tests/test_gpu_matvec_multi.py
uses (its own case classes, built here without a GPU), results that are wrong in the ways a multi-sequence kernel goes wrong must
exceed the bound the GPU tests apply.  A condition on the chosen inputs, not a measurement: every mutation has to be caught."""
import numpy as np
import pytest

import matvec_multi_ref as mm
import matvec_ref as mr
from test_gpu_matvec_multi import EPS, MAX_SEQ, MOE_EI, MOE_H, QKV_MIXES, QKV_SHAPES, ROPE_BASE, ROPE_SCALE, Linear, Qkv, _moe_weights, _norm_w
from test_gpu_prefill_ref import MOE_FORMATS


# ---- the grouping restatement and the inputs
def test_group_lists_pairs_per_expert_ascending():
    sel = np.array([[3, 1], [1, 0], [3, 2]], np.int32)
    cnt, lists = mm.group(sel, 5)
    assert list(cnt) == [1, 2, 1, 2, 0]
    assert lists == [[3], [1, 2], [5], [0, 4], []]
    for kind in ("random", "same", "single"):
        for E, topk, n_seq in ((8, 2, 16), (8, 4, 7), (4, 1, 3)):
            sel, w = mm.selections(kind, n_seq, E, topk, 5)
            cnt, lists = mm.group(sel, E)
            assert cnt.sum() == n_seq * topk and cnt.max() <= n_seq                 # an expert's list holds at most one pair per sequence
            assert all(len(set(row)) == topk for row in sel.tolist())
            assert sorted(v for l in lists for v in l) == list(range(n_seq * topk))
            for e, l in enumerate(lists):
                assert l == sorted(l) and all(sel.reshape(-1)[v] == e for v in l)
            np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=1e-6)
            if topk > 1:
                assert np.all(np.abs(w[:, 0] - w[:, 1]) > 0.05)


def test_group_failures_sees_wrong_tables():
    sel, _ = mm.selections("single", 7, 8, 2, 9)
    cnt, lists = mm.group(sel, 8)
    sentinel = 8 * 2 - 1
    idx = np.full((64, 16), sentinel, np.int32)
    for e, l in enumerate(lists):
        idx[e, :len(l)] = l
    cnt64 = np.full(64, 0x55, np.int32)
    cnt64[:8] = cnt
    assert mm.group_failures(cnt64, idx, sel, 8, sentinel) == []
    e = int(np.argmax(cnt))
    swapped = idx.copy()
    swapped[e, [0, 1]] = swapped[e, [1, 0]]                       # sequences not ascending
    off = cnt64.copy()
    off[0] = 0                                                    # the lone pair's expert counted empty
    over = idx.copy()
    over[0, 1] = 0                                                # an entry written past the count
    late = cnt64.copy()
    late[8] = 0                                                   # a count written past the experts
    for c, i in ((cnt64, swapped), (off, idx), (cnt64, over), (late, idx)):
        assert mm.group_failures(c, i, sel, 8, sentinel)


def test_inputs_are_what_the_tests_need():
    for n_seq, n_slots in ((3, 8), (16, 16)):
        s = mm.slots(n_seq, n_slots, 77 + n_seq)
        assert len(set(s.tolist())) == n_seq and s.max() < n_slots and not np.any(s == np.arange(n_seq))
        p = mm.positions(n_seq, MAX_SEQ)
        assert {0, 1, MAX_SEQ - 1} <= set(p.tolist()) and p.max() < MAX_SEQ and p.min() >= 0
    assert {"zeros", "outlier"} <= set(mm.SEQ_KINDS[:3]) and set(mm.SEQ_KINDS) == set(mr.ACT_KINDS)
    assert [mm.k_slices(k) for k in (256, 512, 1024, 2816, 5632, 14336)] == [(1, 1), (2, 1), (4, 1), (8, 2), (8, 3), (8, 7)]
    rows = mm.sample_rows(20500, 192, 0)
    assert rows[0] == 0 and rows[-1] == 20499 and len(set(rows.tolist())) == rows.size <= 192


def _xq_encode(v32):
    """xq_store_chunk (csrc/xq.h) restated: the image of an f32 vector whose length is a multiple of 256."""
    v32 = np.asarray(v32, np.float32)
    rec = np.zeros((v32.size // 256, 1280), np.uint8)
    for c, ch in enumerate(v32.reshape(-1, 16)):
        blk, j = c >> 4, c & 15
        e = int((np.abs(ch).max().view(np.uint32) >> 23) & 0xFF)
        e = min(max(e, 30), 250)
        I = np.rint(ch.astype(np.float64) * 2.0 ** (156 - e)).astype(np.int64)           # v / s * 2^30, s = 2^(e - 126)
        w = ((I + 0x00808080) ^ 0x00808080) & 0xFFFFFFFF
        for q in range(4):                                            # digit q (0 least significant) -> row i = 3 - q of group g
            off = ((j >> 1) * 4 + (3 - q)) * 32 + (j & 1) * 16
            rec[blk, off:off + 16] = ((w >> (8 * q)) & 0xFF).astype(np.uint8)
        slot = (j & 3) * 4 + (j >> 2)
        rec[blk, 1024 + 4 * slot:1028 + 4 * slot] = np.frombuffer(np.float32(ch.astype(np.float64).sum()).tobytes(), np.uint8)
        rec[blk, 1088 + 4 * slot:1092 + 4 * slot] = np.frombuffer(np.float32(2.0 ** (e - 156)).tobytes(), np.uint8)
    return rec.reshape(-1)


def test_xq_decode_reads_what_the_producers_write():
    for kind in mr.ACT_KINDS:
        out = mr.activation(kind, 512, 3)
        nw = (1 + 0.2 * np.random.default_rng(4).standard_normal(512)).astype(np.float32)
        x, xs = mm.xq_decode(_xq_encode(out * nw), 512)
        (v, ev), (sums, es), _ = mm.image_ref(out, nw)
        assert mm.ratio(x, v, ev) <= 1.0 and mm.ratio(xs, sums, es) <= 1.0, kind
        assert mm.ratio(np.roll(x, 1), v, ev) > 1.0                  # an element in its neighbour's place
        worse = x + np.where(np.arange(512) == 37, 2.0 ** -20 * mr.chunk_max(v), 0.0)
        assert mm.ratio(worse, v, ev) > 1.0                           # one element a thousand steps of its chunk's scale off


# ---- mutations the float64 check must catch
def _caught(got, ref, err):
    return mm.ratio(got, ref, err) > 1.0


def test_mutation_a_sequence_computed_from_its_odd_partners_input():
    L = Linear(None, "Q4_K", 1024, 272, seed=100)
    for n_seq in (2, 5):
        for s in range(n_seq):
            p = s ^ 1                                             # the other sequence of the pair; past the last one: the zero block
            xp = L.X[p] if p < n_seq else np.zeros(L.k, np.float32)
            y, _ = mm.linear(L.tname, L.raw, L.k, L.n, xp[None], nw=L.nw, rows=L.rows, eps=EPS)
            assert _caught(y[0], L.Y[s], L.E[s]), (n_seq, s)
            assert not _caught(L.Y[s], L.Y[s], L.E[s])


def test_mutation_b_one_staged_chunk_of_a_slice_dropped():
    L = Linear(None, "Q4_K", 14336, 48, seed=200)
    T, nbw = mm.k_slices(L.k)
    assert (T, nbw) == (8, 7)
    for s, chunk in ((7, (2, 3)), (15, (6,)), (2, (7 * 7 + 4, 7 * 7 + 5))):      # a chunk of 2 / the slice's last chunk of 1 / in the last slice
        keep = [b for b in range(L.k // 256) if b not in chunk]
        y = mm.linear_blocks(L.tname, L.raw, L.k, L.n, L.X[s], keep, nw=L.nw, rows=L.rows, eps=EPS)
        assert _caught(y, L.Y[s], L.E[s]), (s, chunk)


def test_mutation_g_seq_running_sum_restarted_at_a_slice_boundary():
    L = Linear(None, "Q6_K", 512, 20500, seed=400)
    for s in range(15):
        y = mm.linear_blocks(L.tname, L.raw, L.k, L.n, L.X[s], [1], nw=L.nw, rows=L.rows, eps=EPS)   # T = 2: only the last slice's sum
        assert _caught(y, L.Y[s], L.E[s]), s
    G = Linear(None, "Q4_K", 2816, 10240, role="swiglu", xq_next=1, seed=300)
    T, nbw = mm.k_slices(G.k)
    last = list(range(5 * nbw, 11))                               # slices 6 and 7 hold no block: slice 5's one block is the last sum
    assert last == [10]
    for s in (0, 1, 2, 4, 15):
        g = mm.linear_blocks(G.tname, G.raw, G.k, G.n, G.X[s], last, nw=G.nw, rows=G.rows, eps=EPS)
        u = mm.linear_blocks(G.tname, G.raw_up, G.k, G.n, G.X[s], last, nw=G.nw, rows=G.rows, eps=EPS)
        y, _ = mr.swiglu(g, 0 * g, u, 0 * u)
        assert _caught(y, G.Y[s], G.E[s]), s


@pytest.fixture(scope="module")
def qkv(orc):
    hd, nh, nkv, hidden = QKV_SHAPES[0]
    return Qkv(orc, QKV_MIXES[0], hd, nh, nkv, hidden, with_bias=False)


def test_mutation_c_rope_at_sequence_0s_position(orc, qkv):
    n_seq = 16
    same_pos = np.full(n_seq, qkv.pos[0], np.int32)
    for pre, good in ((qkv.pre[0], qkv.q), (qkv.pre[1], qkv.k)):
        bad, _ = mm.rope_rows(orc, pre[0][:n_seq], pre[1][:n_seq], same_pos, qkv.hd, ROPE_BASE, ROPE_SCALE)
        for s in range(1, n_seq):
            assert _caught(bad[s], good[0][s], good[1][s]), s
        assert not _caught(bad[0], good[0][0], good[1][0])


def test_mutation_d_rows_written_to_slot_s_instead_of_slot_of_s(qkv):
    for n_seq, n_slots in ((3, 8), (16, 16)):
        pos, slot = qkv.pos[:n_seq], mm.slots(n_seq, n_slots, 77 + n_seq)

        def cache(where):
            c = np.full((n_slots, qkv.nkv, MAX_SEQ, qkv.hd), mm.NAN_BITS, np.uint32).view(np.float32).copy()
            for s in range(n_seq):
                c[where[s], :, pos[s], :] = qkv.k[0][s].reshape(qkv.nkv, qkv.hd)
            return c

        assert mm.cache_failures(cache(slot), pos, slot, qkv.k[0], qkv.k[1], "k") == []
        fails = mm.cache_failures(cache(np.arange(n_seq)), pos, slot, qkv.k[0], qkv.k[1], "k")
        assert len(fails) == n_seq + 1, fails                     # every sequence's own row still poisoned, and rows elsewhere changed
        extra = cache(slot)
        extra[slot[0], 0, (pos[0] + 1) % MAX_SEQ, 0] = 0.0        # one element of a row that is nobody's
        assert len(mm.cache_failures(extra, pos, slot, qkv.k[0], qkv.k[1], "k")) >= 1


@pytest.fixture(scope="module")
def moe_case():
    E, topk, n_seq = 8, 2, 3                                      # the GPU test's first case of (E, top_k) = (8, 2)
    tg, td = MOE_FORMATS[(0 + E + topk) % len(MOE_FORMATS)]
    gate, up, down = _moe_weights(tg, td, E, MOE_H, MOE_EI)
    X = mm.activations(MOE_H, n_seq, 41)
    sel, w = mm.selections("random", n_seq, E, topk, 51)
    ex = mm.Experts(tg, gate, up, td, down, E, MOE_H, MOE_EI)
    nw = _norm_w(MOE_H, 1)
    good = [mm.moe(ex, X[s], [X[s]] * topk, nw, sel[s], w[s], eps=EPS) for s in range(n_seq)]
    return ex, X, nw, sel, w, topk, good


def test_mutation_e_a_pair_reads_input_v_instead_of_v_over_top_k(moe_case):
    ex, X, nw, sel, w, topk, good = moe_case
    n_seq = len(X)
    for s in range(n_seq):
        src = [(s * topk + p) % n_seq for p in range(topk)]       # (past the sequences' vectors lies the next buffer: any other vector)
        assert src != [s] * topk
        y, _ = mm.moe(ex, X[s], [X[v] for v in src], nw, sel[s], w[s], eps=EPS)
        assert _caught(y, *good[s]), s


def test_mutation_f_slot_weights_of_a_sequence_swapped(moe_case):
    ex, X, nw, sel, w, topk, good = moe_case
    for s in range(len(X)):
        y, _ = mm.moe(ex, X[s], [X[s]] * topk, nw, sel[s], w[s][::-1], eps=EPS)
        assert _caught(y, *good[s]), s
        y, _ = mm.moe(ex, X[s], [X[s]] * topk, nw, sel[s][::-1], w[s][::-1], eps=EPS)    # (the same pairs in the other order: the same sum)
        assert not _caught(y, *good[s]), s
