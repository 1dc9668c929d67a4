"""numpy restatement of the device prompt cache's packed layout (csrc/kv_prefix.hip), over the sizes lgh_kv_cache_layout reports.

A layer's cache is five tensors in KvKind order — K rows, V rows, K scales, V scales, K QJL words — each
[n_slots, n_kv, max_seq, bytes per position] uint8, or None where the format has none.  A prefix of n rows of one slot is
[layer][kind the format has][kv head][n][bytes per position], no padding."""
import numpy as np


def pos_bytes(lay):
    """Bytes per (kv head, position) of the five tensors, from an lgh_kv_layout."""
    return [lay.row_bytes, lay.row_bytes, lay.scale_bytes, lay.scale_bytes, lay.qjl_bytes]


def packed_size(lay, n_layers, n_kv, n):
    return n_layers * n_kv * n * (2 * (lay.row_bytes + lay.scale_bytes) + lay.qjl_bytes)


def random_caches(rng, lay, n_layers, n_slots, n_kv, max_seq, fill=None):
    """Per layer the five tensors, random bytes (or every byte `fill`)."""
    def one(pb):
        if not pb:
            return None
        shape = (n_slots, n_kv, max_seq, pb)
        return rng.integers(0, 256, size=shape, dtype=np.uint8) if fill is None else np.full(shape, fill, np.uint8)
    return [[one(pb) for pb in pos_bytes(lay)] for _ in range(n_layers)]


def pack(caches, slot, n):
    """Rows [0, n) of `slot`, packed."""
    parts = [t[slot, :, :n, :].reshape(-1) for layer in caches for t in layer if t is not None]
    return np.concatenate(parts)


def unpack(caches, slot, n, packed, n_stride=None):
    """Copies of `caches` with rows [0, n) of `slot` taken from a prefix packed with n_stride (default n) rows."""
    n_stride = n if n_stride is None else n_stride
    out = [[None if t is None else t.copy() for t in layer] for layer in caches]
    off = 0
    for layer in out:
        for t in layer:
            if t is None:
                continue
            n_kv, pb = t.shape[1], t.shape[3]
            seg = np.asarray(packed[off:off + n_kv * n_stride * pb]).reshape(n_kv, n_stride, pb)
            t[slot, :, :n, :] = seg[:, :n, :]
            off += n_kv * n_stride * pb
    assert off == len(packed)
    return out
