"""Cases and the per-sequence float64 reference for the multi-sequence attention over int8 / FP8 cache slots
(lgh_op_attention_kv8_multi; tests/test_gpu_attention_kv8_multi.py), on top of tests/attention_ref.py.

One launch serves n_seq sequences.  Sequence s reads rows 0..pos[s]-1 of cache slot slot[s], quantizes its own staged rows
k_new[s] / v_new[s] into row pos[s] of that slot and attends to rows 0..pos[s] through their stored values.  So its reference is
attention_ref.decode over the values that slot's bytes stand for AFTER the call, rows 0..pos[s] — nothing of any other slot,
position or staged row enters it.

A case poisons everything a sequence must not read: every row at or past pos[s] of its slot (the row the launch writes included)
and every row of a slot no sequence names — the FP8 NaN byte 0x7F, or an int8 row with a NaN scale, as test_decode_kv8 does for
one sequence.  A read of any of them shows as NaN in the output."""
from __future__ import annotations

import numpy as np

import attention_ref as ar

N_KV = 2
KV_INT8, KV_FP8_E4M3, KV_FP8_E5M2 = 1, 2, 3
_TABLES: dict = {}


def encode_row(orc, kv_type: int, x):
    """The oracle's encoding of one row: (bytes uint8 [d], scale f32; 1 for the FP8 formats)."""
    if kv_type == KV_INT8:
        b, sc = orc.kv_quantize_int8(np.ascontiguousarray(x, np.float32))
        return b.view(np.uint8), np.float32(sc)
    fmt = {KV_FP8_E4M3: orc.FP8_E4M3, KV_FP8_E5M2: orc.FP8_E5M2}[kv_type]
    return np.array([orc.kv_quantize_fp8(fmt, float(e)) for e in x], np.uint8), np.float32(1.0)


def _table(orc, kv_type: int) -> np.ndarray:
    if kv_type not in _TABLES:
        _TABLES[kv_type] = ar.fp8_table(orc, kv_type)
    return _TABLES[kv_type]


def values(orc, kv_type: int, b, scales) -> np.ndarray:
    """float64 values the kernel reads from stored bytes b [..., d] (and, int8, scales [...])."""
    return ar.int8_values(b, scales) if kv_type == KV_INT8 else _table(orc, kv_type)[np.asarray(b)]


def stride_of(d: int, n_splits: int) -> int:
    """Rows one pass of all workgroups of a kv head covers: n_splits x 4 waves x (256 / d) rows per wave-instruction.  A split's loop
    requests 4 such passes per batch, so a sequence with pos > 4 * stride enters the second batch and one with pos <= 4 * stride does not."""
    return n_splits * 4 * (256 // d)


def positions(d: int, n_splits: int):
    """The positions worth mixing in one launch: only the staged row; one cached row; one short of a pass / exactly a pass; just into
    the second batch; a few passes more."""
    st = stride_of(d, n_splits)
    return [0, 1, st - 1, st, 4 * st + 1, 300]


def make_case(orc, rng, kv_type: int, d: int, g: int, n_slots: int, slot, pos, max_seq: int, kind: str = "normal", n_kv: int = N_KV) -> dict:
    """Inputs of one launch.  kind "hot": scores in the hundreds (the online softmax's rescaling)."""
    slot, pos = [int(x) for x in slot], [int(x) for x in pos]
    n_seq = len(slot)
    assert len(pos) == n_seq and len(set(slot)) == n_seq and all(0 <= s < n_slots for s in slot) and all(0 <= p < max_seq for p in pos)
    q = rng.standard_normal((n_seq, n_kv * g, d)).astype(np.float32)
    if kind == "hot":
        q *= 30.0
    shape = (n_slots, n_kv, max_seq, d)
    if kv_type == KV_INT8:
        kb = rng.integers(-127, 128, shape).astype(np.int8).view(np.uint8)
        vb = rng.integers(-127, 128, shape).astype(np.int8).view(np.uint8)
        ks = rng.uniform(0.005, 0.03, shape[:3]).astype(np.float32)
        vs = rng.uniform(0.005, 0.03, shape[:3]).astype(np.float32)
    else:
        t = _table(orc, kv_type)
        finite = np.flatnonzero(np.isfinite(t) & (np.abs(t) <= 4.0))
        kb = rng.choice(finite, shape).astype(np.uint8)
        vb = rng.choice(finite, shape).astype(np.uint8)
        ks = vs = None
    first_poisoned = [0] * n_slots             # a slot no sequence names: every row
    for s in range(n_seq):
        first_poisoned[slot[s]] = pos[s]
    for sl in range(n_slots):
        if kv_type == KV_INT8:
            ks[sl, :, first_poisoned[sl]:] = np.nan
            vs[sl, :, first_poisoned[sl]:] = np.nan
        else:
            kb[sl, :, first_poisoned[sl]:] = 0x7F
            vb[sl, :, first_poisoned[sl]:] = 0x7F
    k_new = rng.standard_normal((n_seq, n_kv, d)).astype(np.float32)
    v_new = rng.standard_normal((n_seq, n_kv, d)).astype(np.float32)
    return dict(kv_type=kv_type, d=d, g=g, n_kv=n_kv, n_slots=n_slots, max_seq=max_seq, slot=slot, pos=pos, q=q, kb=kb, vb=vb, ks=ks, vs=vs,
                k_new=k_new, v_new=v_new, scale=float(1.0 / np.sqrt(d)))


def after_call(orc, case: dict, k_new=None, v_new=None):
    """What the caches must hold after the launch: row pos[s] of slot slot[s] as the oracle encodes k_new[s] / v_new[s] (scale
    included), everything else as it was.  -> (kb, vb, ks, vs); ks / vs None for FP8."""
    kt = case["kv_type"]
    k_new = case["k_new"] if k_new is None else k_new
    v_new = case["v_new"] if v_new is None else v_new
    kb, vb = case["kb"].copy(), case["vb"].copy()
    ks = case["ks"].copy() if kt == KV_INT8 else None
    vs = case["vs"].copy() if kt == KV_INT8 else None
    for s, (sl, p) in enumerate(zip(case["slot"], case["pos"])):
        for h in range(case["n_kv"]):
            kb[sl, h, p], sc = encode_row(orc, kt, k_new[s, h])
            if kt == KV_INT8:
                ks[sl, h, p] = sc
            vb[sl, h, p], sc = encode_row(orc, kt, v_new[s, h])
            if kt == KV_INT8:
                vs[sl, h, p] = sc
    return kb, vb, ks, vs


def sequence_reference(orc, case: dict, after, s: int, slot=None, pos=None):
    """Sequence s's reference from the caches `after` the call: attention_ref.decode of q[s] over rows 0..pos[s] of slot slot[s].
    -> (out [n_heads, d] float64, S, max|V|, n) — the last three are what attention_ref.worst_ratio takes.  `slot` / `pos` override
    the sequence's own (for planting a mistake)."""
    kt = case["kv_type"]
    sl = case["slot"][s] if slot is None else slot
    n = (case["pos"][s] if pos is None else pos) + 1
    kb, vb, ks, vs = after
    K = values(orc, kt, kb[sl, :, :n], ks[sl, :, :n] if kt == KV_INT8 else None)
    V = values(orc, kt, vb[sl, :, :n], vs[sl, :, :n] if kt == KV_INT8 else None)
    q = case["q"][s]
    return ar.decode(q, K, V, case["scale"], n), ar.magnitude(q, K, case["scale"], n), float(np.abs(V).max()), n
