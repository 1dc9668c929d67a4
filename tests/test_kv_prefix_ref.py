"""The numpy restatement of the prompt cache's packed layout (tests/kv_prefix_ref.py) against hand-written cases, and the packed size
against layers * kv heads * rows * (2 * (row + scale) + qjl) for every cache format.  CPU only: lgh_kv_cache_layout needs no device."""
import types

import numpy as np
import pytest

import kv_prefix_ref as ref


def _lay(row, scale=0, qjl=0):
    return types.SimpleNamespace(row_bytes=row, scale_bytes=scale, qjl_bytes=qjl)


def test_pack_orders_layer_kind_head_row_by_hand():
    """2 layers, 2 slots, 2 kv heads, max_seq 3, 2-byte rows and 1-byte scales, no QJL: every byte written out."""
    lay = _lay(2, 1)
    caches = ref.random_caches(np.random.default_rng(0), lay, 2, 2, 2, 3, fill=0)
    v = 1
    for layer in caches:                       # number every byte of slot 1 in memory order, slot 0 stays 0
        for t in layer:
            if t is not None:
                t[1] = np.arange(v, v + t[1].size, dtype=np.uint8).reshape(t[1].shape)
                v += t[1].size
    assert caches[0][4] is None and caches[1][4] is None
    # layer 0: K = 1..12 as [head][pos][2], V = 13..24, kscale = 25..30 as [head][pos], vscale = 31..36; layer 1 goes on from 37
    want = [1, 2, 3, 4, 7, 8, 9, 10,           # K: head 0 rows 0, 1; head 1 rows 0, 1
            13, 14, 15, 16, 19, 20, 21, 22,    # V
            25, 26, 28, 29,                    # K scales
            31, 32, 34, 35,                    # V scales
            37, 38, 39, 40, 43, 44, 45, 46,
            49, 50, 51, 52, 55, 56, 57, 58,
            61, 62, 64, 65,
            67, 68, 70, 71]
    got = ref.pack(caches, 1, 2)
    assert got.tolist() == want
    assert got.size == ref.packed_size(lay, 2, 2, 2)
    assert not ref.pack(caches, 0, 3).any()


def test_unpack_writes_only_the_rows_of_the_slot_by_hand():
    lay = _lay(2, 0, 3)                        # rows and QJL words, no scales
    caches = ref.random_caches(np.random.default_rng(0), lay, 1, 2, 2, 3, fill=0xEE)
    packed = np.arange(1, 1 + ref.packed_size(lay, 1, 2, 2), dtype=np.uint8)     # 1 .. 28
    out = ref.unpack(caches, 0, 2, packed)
    k, v, ks, vs, kx = out[0]
    assert ks is None and vs is None
    assert k[0].tolist() == [[[1, 2], [3, 4], [0xEE, 0xEE]], [[5, 6], [7, 8], [0xEE, 0xEE]]]
    assert v[0].tolist() == [[[9, 10], [11, 12], [0xEE, 0xEE]], [[13, 14], [15, 16], [0xEE, 0xEE]]]
    assert kx[0].tolist() == [[[17, 18, 19], [20, 21, 22], [0xEE] * 3], [[23, 24, 25], [26, 27, 28], [0xEE] * 3]]
    for t in (k, v, kx):
        assert (t[1] == 0xEE).all()
    assert (caches[0][0] == 0xEE).all()        # the input is not changed
    # fewer rows than the prefix was packed with: the segment stride stays the prefix's
    out1 = ref.unpack(caches, 1, 1, packed, n_stride=2)
    assert out1[0][0][1].tolist() == [[[1, 2], [0xEE, 0xEE], [0xEE, 0xEE]], [[5, 6], [0xEE, 0xEE], [0xEE, 0xEE]]]
    assert out1[0][4][1, 1, 0].tolist() == [23, 24, 25]


def test_pack_then_unpack_round_trips():
    lay = _lay(24, 4, 12)
    rng = np.random.default_rng(5)
    src = ref.random_caches(rng, lay, 3, 3, 2, 37)
    dst = ref.random_caches(rng, lay, 3, 3, 2, 37)
    p = ref.pack(src, 1, 36)
    out = ref.unpack(dst, 2, 36, p)
    assert np.array_equal(ref.pack(out, 2, 36), p)
    for lo, ld in zip(out, dst):
        for a, b in zip(lo, ld):
            assert np.array_equal(a[:2], b[:2]) and np.array_equal(a[2, :, 36:], b[2, :, 36:])


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("kv", range(8))
def test_packed_size_follows_the_layout_of_every_format(pkg, kv, d):
    n_layers, n_slots, n_kv, max_seq, n = 3, 2, 2, 37, 5
    lay = pkg.hip_backend.kv_cache_layout(kv, n_kv, max_seq, d)
    caches = ref.random_caches(np.random.default_rng(kv), lay, n_layers, n_slots, n_kv, max_seq)
    row = {0: 4 * d, 1: d, 2: d, 3: d, 4: d // 4, 5: d // 8 * 3, 6: d // 4, 7: d // 8 * 3}[kv]
    scale, qjl = (4 if kv == 1 else 0), (d // 8 + 4 if kv in (6, 7) else 0)
    assert ref.pos_bytes(lay) == [row, row, scale, scale, qjl]
    want = n_layers * n_kv * n * (2 * (row + scale) + qjl)
    assert ref.packed_size(lay, n_layers, n_kv, n) == want
    assert ref.pack(caches, 1, n).size == want
    for layer in caches:                       # the tensors are as large as the layout says a slot's are
        sizes = [0 if t is None else t[0].size for t in layer]
        assert sizes == [lay.k_bytes, lay.v_bytes, lay.k_scale_bytes, lay.v_scale_bytes, lay.k_qjl_bytes]
