"""Cases and the per-sequence float64 reference for the multi-sequence attention over TurboQuant cache slots
(lgh_op_attention_tq_multi; tests/test_gpu_attention_kv_tq_multi.py), on top of tests/attention_ref.py.

One launch serves n_seq sequences.  Sequence s reads rows 0..pos[s]-1 of cache slot slot[s], compresses its own staged rows
k_new[s] / v_new[s] into row pos[s] of that slot (codes; for the QJL types also the sign words and the residual norm of K) and
attends to rows 0..pos[s] through what they hold.  So its reference is attention_ref.tq_decode over that slot's rows AFTER the call,
rows 0..pos[s] — nothing of any other slot, position, staged row, query or kv head's signs enters it.

A case poisons everything a sequence must not read: every row at or past pos[s] of its slot (the row the launch writes included)
and every row of a slot no sequence names.  A code row has no NaN, so a poisoned V row is all 0xFF: every rotated coordinate at the
top centroid, which stands for sqrt(d) * centroid = 2.15 (3 bits) / 1.51 (2 bits) at coordinate 0 of the row, about 20 times a
normal element; for the QJL types a poisoned row also carries a NaN norm, as test_decode_tq's do, and shows as NaN."""
from __future__ import annotations

import numpy as np

import attention_ref as ar

N_KV = 2
KV_TQ2, KV_TQ3, KV_TQ2_QJL, KV_TQ3_QJL = 4, 5, 6, 7
KV_TYPES = [KV_TQ2, KV_TQ3, KV_TQ2_QJL, KV_TQ3_QJL]
KV_IDS = ["tq2", "tq3", "tq2_qjl", "tq3_qjl"]
MAX_SEQ = 512
SPLITS = (2, 3)


def bits_of(kv_type: int) -> int:
    return 2 if kv_type in (KV_TQ2, KV_TQ2_QJL) else 3


def is_qjl(kv_type: int) -> bool:
    return kv_type in (KV_TQ2_QJL, KV_TQ3_QJL)


def row_bytes(bits: int, d: int) -> int:
    return d // 4 if bits == 2 else d // 8 * 3


def stride_of(d: int, n_splits: int) -> int:
    """Rows one pass of all workgroups of a kv head covers: n_splits x 4 waves x (1024 / d) rows per wave-instruction (16 coordinates
    of a row per lane).  A split's loop requests 2 such passes per batch (kAhead), the first batch ahead of the rotations."""
    return n_splits * 4 * (1024 // d)


def positions(d: int, n_splits: int, max_seq: int = MAX_SEQ):
    """The positions worth mixing in one launch: only the staged row; one cached row; one short of a pass / exactly a pass; the last
    position whose rows all lie in the first batch / the first that sends a workgroup into the second; the last row of a slot."""
    st = stride_of(d, n_splits)
    P = [0, 1, st - 1, st, 2 * st - 1, 2 * st, max_seq - 1]
    assert all(a < b for a, b in zip(P, P[1:])), (d, n_splits, max_seq, P)   # (all of them fit, none coincides)
    return P


def launches(d: int, n_splits: int, max_seq: int = MAX_SEQ):
    """(slot, pos, kind) of the launches of one split count on 5 slots: three sequences on slots that are not the identity with one or
    two slots unused, and single sequences; every position class in some launch, the last row of a slot on the highest slot (what
    lies behind it belongs to nobody)."""
    P = positions(d, n_splits, max_seq)
    return [([3, 0, 4], [P[0], P[5], P[6]], "normal"), ([1, 4, 2], [P[3], P[1], P[4]], "hot"),
            ([2], [P[5]], "hot"), ([4], [P[6]], "normal"), ([3], [P[2]], "normal")]


def make_case(orc, rng, kv_type: int, d: int, g: int, n_slots: int, slot, pos, max_seq: int, kind: str = "normal", n_kv: int = N_KV) -> dict:
    """Inputs of one launch.  kind "hot": scores in the hundreds (the online softmax's rescaling)."""
    slot, pos = [int(x) for x in slot], [int(x) for x in pos]
    n_seq = len(slot)
    assert len(pos) == n_seq and len(set(slot)) == n_seq and all(0 <= s < n_slots for s in slot) and all(0 <= p < max_seq for p in pos)
    assert kind in ("normal", "hot")
    bits, qjl = bits_of(kv_type), is_qjl(kv_type)
    rb, xw = row_bytes(bits, d), d // 32 + 1
    q = rng.standard_normal((n_seq, n_kv * g, d)).astype(np.float32)
    if kind == "hot":
        q *= 30.0
    signs = np.where(rng.random((n_kv, 2, d)) < 0.5, -1.0, 1.0).astype(np.float32)
    S = rng.standard_normal((n_kv, d, d)).astype(np.float32) if qjl else None
    kc = rng.integers(0, 256, (n_slots, n_kv, max_seq, rb)).astype(np.uint8)
    vc = rng.integers(0, 256, (n_slots, n_kv, max_seq, rb)).astype(np.uint8)
    kx = nrm = None
    if qjl:
        kx = rng.integers(0, 2 ** 32, (n_slots, n_kv, max_seq, xw), dtype=np.uint64).astype(np.uint32)
        nrm = (0.3 * np.abs(rng.standard_normal((n_slots, n_kv, max_seq)))).astype(np.float32)
    first_poisoned = [0] * n_slots             # a slot no sequence names: every row
    for s in range(n_seq):
        first_poisoned[slot[s]] = pos[s]
    for sl in range(n_slots):
        vc[sl, :, first_poisoned[sl]:] = 0xFF
        if qjl:
            nrm[sl, :, first_poisoned[sl]:] = np.nan
    if qjl:
        kx[..., xw - 1] = nrm.view(np.uint32)
    # The staged rows are what tells "row pos[s] dropped" or "another sequence's staged rows" from the truth, at a weight of about
    # 1 / (pos + 1).  K rows of about unit length, the range the codebook is made for: the QJL residual norm of the stored row then is of
    # the cached rows' order (0.3), not the ~4 of a saturating N(0, 1) row, which alone puts S (and so the bound) near 100.  V rows
    # N(0, 1) (saturating: every code at an end centroid) with one outlier coordinate per (sequence, kv head), which survives the
    # compression as a coordinate of about 1: a row that differs from the others' mean by more than a bound at weight 1 / 512
    # (tests/test_attention_tq_multi_ref.py measures it).
    k_new = (rng.standard_normal((n_seq, n_kv, d)) / np.sqrt(d)).astype(np.float32)
    v_new = rng.standard_normal((n_seq, n_kv, d)).astype(np.float32)
    for s in range(n_seq):
        for h in range(n_kv):
            v_new[s, h, (7 * s + 3 * h + 1) % d] += 8.0
    return dict(kv_type=kv_type, bits=bits, qjl=qjl, d=d, g=g, n_kv=n_kv, n_slots=n_slots, max_seq=max_seq, slot=slot, pos=pos, q=q, kc=kc, vc=vc,
                kx=kx, signs=signs, S=S, k_new=k_new, v_new=v_new, scale=float(1.0 / np.sqrt(d)))


def before_call(case: dict):
    """The caches as the launch finds them, in after_call's form (row pos[s] still stale: poisoned)."""
    return case["kc"], case["vc"], case["kx"]


def after_call(orc, case: dict, k_new=None, v_new=None):
    """What the caches must hold after the launch: row pos[s] of slot slot[s] as the oracle compresses k_new[s] / v_new[s] with the kv
    head's K / V signs (QJL types: codes, sign words and norm of K), everything else as it was.  -> (kc, vc, kx); kx None without QJL."""
    k_new = case["k_new"] if k_new is None else k_new
    v_new = case["v_new"] if v_new is None else v_new
    bits, qjl, signs = case["bits"], case["qjl"], case["signs"]
    kc, vc = case["kc"].copy(), case["vc"].copy()
    kx = case["kx"].copy() if qjl else None
    for s, (sl, p) in enumerate(zip(case["slot"], case["pos"])):
        for h in range(case["n_kv"]):
            if qjl:
                codes, qb, norm = orc.tq_compress_qjl(k_new[s, h], bits, signs[h, 0], case["S"][h])
                kc[sl, h, p] = codes
                kx[sl, h, p] = np.concatenate([qb.view(np.uint32), np.float32([norm]).view(np.uint32)])
            else:
                kc[sl, h, p] = orc.tq_compress(k_new[s, h], bits, signs[h, 0])
            vc[sl, h, p] = orc.tq_compress(v_new[s, h], bits, signs[h, 1])
    return kc, vc, kx


def sequence_reference(orc, case: dict, after, s: int, slot=None, pos=None, q=None, x_slot=None, signs=None):
    """Sequence s's reference from the caches `after` the call: attention_ref.tq_decode of q[s] over rows 0..pos[s] of slot slot[s].
    -> (out [n_heads, d] float64, S, vmax, n) — the last three are what attention_ref.worst_ratio takes.  The keywords override the
    sequence's own slot, position, query, the slot its QJL rows come from and the signs (for planting a mistake)."""
    sl = case["slot"][s] if slot is None else slot
    n = (case["pos"][s] if pos is None else pos) + 1
    kc, vc, kx = after
    xs = sl if x_slot is None else x_slot
    out, s_mag, vmax = ar.tq_decode(orc, case["q"][s] if q is None else q, kc[sl], vc[sl], case["bits"], case["signs"] if signs is None else signs,
                                    case["scale"], n, kx[xs] if case["qjl"] else None, case["S"])
    return out, s_mag, vmax, n
