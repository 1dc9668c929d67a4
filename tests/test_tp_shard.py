"""lgh_tp_shard on the CPU (no device needed): the one implementation of the tensor-parallel slicing.  For every format the engine
keeps in its matrix-core tile layouts, and F32: dequantize(shard) is bit for bit the matching slice of dequantize(whole) (oracle
dequantize), the shards of one tensor are disjoint and together cover every block, and what cannot be sliced is refused with the
stated status and nothing written."""
import ctypes as C

import numpy as np
import pytest

import tp_ref

TYPES = ("Q4_K", "Q5_K", "Q6_K", "Q8_0", "Q4_0", "F32")
# (axis, rows, k, ranks): k-shards of 2 and 3 blocks of 256 per rank (and 2 per rank of 4 ranks); row shards of [96 x 512]; rows that
# no rank count divides: whole 16-row tiles, the remainder to the last rank (output.weight's rule)
SHAPES = [(1, 48, 1536, 2), (1, 48, 1536, 3), (1, 48, 2048, 4), (0, 96, 512, 2), (0, 96, 512, 3), (0, 96, 512, 4), (0, 100, 512, 3), (0, 1000, 256, 4)]


def _tensor(pkg, tname, rows, k, seed):
    return pkg.synth.fill_tensor("blk.0.tp_%s_%d.weight" % (tname, seed), tp_ref.TYPE[tname], rows * k, k)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("axis,rows,k,n", SHAPES)
def test_shards_dequantize_to_the_slices_and_cover_every_block(pkg, orc, tname, axis, rows, k, n):
    hb, t = pkg.hip_backend, tp_ref.TYPE[tname]
    bs, bb = tp_ref.BLOCK[tname]
    raw = _tensor(pkg, tname, rows, k, rows + k)
    assert raw.size == rows * k // bs * bb
    dense = orc.dequantize(t, raw, rows * k).reshape(rows, k)
    blocks = raw.reshape(rows * k // bs, bb)
    hits = np.zeros(len(blocks), np.int64)
    total = 0
    for rank in range(n):
        shard = hb.tp_shard(t, (k, rows), axis, rank, n, raw)
        want = tp_ref.shard_elems(dense, axis, rank, n)
        assert shard.size == want.size // bs * bb
        got = orc.dequantize(t, shard, want.size).reshape(want.shape)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (tname, axis, rank, n)
        total += shard.size
        # the shard's blocks, in order, are the blocks of its rows / block columns in GGUF order
        if axis == 0:
            r0, r1 = tp_ref.row_range(rows, rank, n)
            ids = np.arange(r0 * (k // bs), r1 * (k // bs))
        else:
            per = k // bs // n
            ids = (np.arange(rows)[:, None] * (k // bs) + rank * per + np.arange(per)[None, :]).reshape(-1)
        assert np.array_equal(shard.reshape(-1, bb), blocks[ids])
        hits[ids] += 1
    assert total == raw.size and np.all(hits == 1)          # disjoint, and every block is somewhere


def test_whole_tensor_for_one_rank_and_vector_rows(pkg):
    hb = pkg.hip_backend
    raw = _tensor(pkg, "Q6_K", 32, 512, 5)
    for axis in (0, 1):
        assert np.array_equal(hb.tp_shard(tp_ref.TYPE["Q6_K"], (512, 32), axis, 0, 1, raw), raw)
    bias = np.arange(96, dtype=np.float32)                   # a bias: 96 rows of one element
    for r in range(3):
        got = hb.tp_shard(0, (1, 96), 0, r, 3, bias.view(np.uint8)).view(np.float32)
        assert np.array_equal(got, bias[32 * r:32 * r + 32])


def _raw_call(pkg, t, ne, axis, rank, n, raw, dst):
    ne4 = (C.c_uint64 * 4)(*(list(ne) + [0] * (4 - len(ne))))
    written = C.c_size_t(12345)
    st = pkg.hip_backend.load_library().lgh_tp_shard(t, ne4, axis, rank, n, raw.ctypes.data, raw.nbytes, dst.ctypes.data, dst.nbytes, C.byref(written))
    return st, written.value


def test_refusals_write_nothing(pkg):
    BE = pkg.BackendError
    t = tp_ref.TYPE["Q4_K"]
    raw = _tensor(pkg, "Q4_K", 48, 1536, 1)
    dst = np.full(raw.size, 0xC3, np.uint8)

    def refused(variant, *a, **kw):
        st, written = _raw_call(pkg, *a, **kw)
        assert st != 0 and BE(st, "").variant == variant, (a[1:5], st)
        assert written == 0 and np.all(dst == 0xC3)

    refused("Unsupported", t, (1536, 48), 1, 0, 4, raw, dst)              # 6 blocks of 256 over 4 ranks
    refused("Unsupported", t, (1536, 48), 1, 3, 4, raw, dst)
    q8 = _tensor(pkg, "Q8_0", 48, 1536, 2)                                 # whole 32-element blocks per rank are not enough
    refused("Unsupported", tp_ref.TYPE["Q8_0"], (1536, 48), 1, 0, 4, q8, dst)
    for axis in (0, 1):
        refused("InvalidArgument", t, (1536, 48), axis, 2, 2, raw, dst)    # rank >= n
        refused("InvalidArgument", t, (1536, 48), axis, 0, 9, raw, dst)    # more than 8 ranks
        refused("InvalidArgument", t, (1536, 48), axis, 0, 2, raw, dst[:raw.size // 2 - 1])   # dst one byte short
    refused("InvalidArgument", t, (1536, 48), 2, 0, 2, raw, dst)           # no such axis
    refused("ShapeMismatch", t, (1536, 48), 0, 0, 2, raw[:-144], dst)      # src does not hold the tensor
    refused("Unsupported", t, (256, 16), 0, 1, 3, raw[:16 * 144], dst)     # 16 rows: one tile, three ranks
    # a dst of exactly the shard's size is enough, and nothing past `written` changes
    st, written = _raw_call(pkg, t, (1536, 48), 1, 1, 2, raw, dst[:raw.size // 2])
    assert st == 0 and written == raw.size // 2 and np.all(dst[raw.size // 2:] == 0xC3)
