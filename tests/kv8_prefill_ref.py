"""A float64 restatement of a block of prompt tokens over a byte KV cache (int8 + row scales, FP8 E4M3, FP8 E5M2): QuantizedKVCache's
row write followed by its attention for every token of the block (kv_quantized.rs:143-300), which is `attention_ref.prefill` over
the values the stored bytes stand for.  Every row takes part through its bytes, a token's own row included.  Shared by
tests/test_kv8_prefill_ref.py (against the oracle, on the CPU) and tests/test_gpu_kv8_prefill.py (the arbiter of the batched path's
kernels)."""
from __future__ import annotations

import numpy as np

import attention_kv8_multi_ref as mr
import attention_ref as ar

KV_INT8, KV_FP8_E4M3, KV_FP8_E5M2 = mr.KV_INT8, mr.KV_FP8_E4M3, mr.KV_FP8_E5M2
FORMATS = (KV_INT8, KV_FP8_E4M3, KV_FP8_E5M2)
NAMES = {KV_INT8: "int8", KV_FP8_E4M3: "e4m3", KV_FP8_E5M2: "e5m2"}


def encode_rows(orc, kv_type: int, rows):
    """rows [n_kv, n, d] f32 -> (bytes uint8 [n_kv, n, d], scales f32 [n_kv, n]; 1 for the FP8 formats): the oracle's encoding of
    every row."""
    rows = np.asarray(rows, np.float32)
    b = np.zeros(rows.shape, np.uint8)
    sc = np.ones(rows.shape[:2], np.float32)
    for h in range(rows.shape[0]):
        for r in range(rows.shape[1]):
            b[h, r], sc[h, r] = mr.encode_row(orc, kv_type, rows[h, r])
    return b, sc


def values(orc, kv_type: int, b, scales, n: int) -> np.ndarray:
    """float64 [n_kv, n, d]: what rows 0..n-1 of the stored bytes (and, int8, scales) stand for."""
    return mr.values(orc, kv_type, np.asarray(b)[:, :n], None if scales is None else np.asarray(scales)[:, :n])


def block(orc, kv_type: int, q, kb, vb, ks, vs, scale: float, pos0: int, m: int) -> np.ndarray:
    """The reference: out [m, n_heads, d] float64 of the block's tokens; q [m, n_heads, d]; bytes [n_kv, rows, d], scales [n_kv, rows]."""
    n = pos0 + m
    return ar.prefill(q, values(orc, kv_type, kb, ks, n), values(orc, kv_type, vb, vs, n), scale, pos0, m)


def magnitudes(orc, kv_type: int, q, kb, vb, ks, vs, scale: float, n: int):
    """(S, vmax) of attention_ref.bound over every token of the block and rows 0..n-1."""
    K, V = values(orc, kv_type, kb, ks, n), values(orc, kv_type, vb, vs, n)
    return ar.magnitude(q, K, scale, n), float(np.abs(V).max())


def set_oracle_format(orc, ref, kv_type: int) -> None:
    """The oracle model's cache in the given byte format."""
    if kv_type == KV_INT8:
        ref.set_kv_int8()
    else:
        ref.set_kv_fp8({KV_FP8_E4M3: orc.FP8_E4M3, KV_FP8_E5M2: orc.FP8_E5M2}[kv_type])
