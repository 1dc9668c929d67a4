#!/usr/bin/env python3
"""One SHA-256 per attention launch, for comparing two builds bit for bit.

    python tools/attn_bits.py --out profiles/attn_bits_<build>.json           (LGH_LIB_VARIANT picks the library, as everywhere)

Every per-path entry point of the attention kernels is run on seeded inputs: op_attention_decode (split, direct, any),
op_attention_cached, op_attention_decode_multi, op_attention_kv8 / _kv8_multi (cache types 1-3), op_attention_tq (cache types 4-7),
op_attention_prefill, op_attention_prefill_tq (cache types 4, 5) and op_attention_prefill_kv8 (cache types 1-3) — for head_dim
64 / 128 with 1, 2, 4, 8 query heads per kv head, (max_seq, pos) in {(1024, 0), (1024, 65), (1024, 1000), (4096, 4095)} and 1, 7,
32 splits where the path has splits; the multi-sequence forms with 3 sequences in distinct slots at distinct positions.  A case's hash covers the output and, where the entry point returns the cache,
the row the launch wrote.  The prefill op is run once more in a fresh process with LGH_PF_ATTN_VALU=1 (the only route to
attn_partial_kernel<..., PF = true>).

--out gets one SHA-256 per (entry point, head_dim, group size): the digest of that group's case names and case hashes, in order
(1536 cases in 176 groups; small enough to keep beside the code).  --full FILE writes the hash of every case as well, for finding
the case once a group differs.  Two builds compute the same bits exactly when their files are equal.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

SHAPES = [(d, g) for d in (64, 128) for g in (1, 2, 4, 8)]
LENGTHS = [(1024, 0), (1024, 65), (1024, 1000), (4096, 4095)]
SPLITS = (1, 7, 32)
N_KV = 2
PF_TOKENS = 21        # prompt block of the prefill cases: two token tiles, the second partly filled
PF_N_KV = 4           # the prefill ops take n_heads * head_dim in multiples of 256
SLOTS = (2, 0, 3)     # of 4 cache slots


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def multi_positions(pos, max_seq):
    return [pos, min(pos // 2 + 1, max_seq - 1), min(pos // 3 + 2, max_seq - 1)]


def small_fp8(rng, shape):
    """random FP8 bytes of either format with magnitude below 2 (no infinities, no NaN patterns)"""
    b = rng.integers(0, 256, size=shape, dtype=np.uint8)
    return b & np.uint8(0xBF)


def prefill_cases(hb, res, tag, tq):
    for d, g in SHAPES:
        for max_seq, pos in LENGTHS:
            rng = np.random.default_rng([7, d, g, max_seq, pos])
            pos0 = max(pos - PF_TOKENS + 1, 0)
            key = f"d{d}g{g}/s{max_seq}p{pos0}"
            q = rng.standard_normal((PF_TOKENS, PF_N_KV * g, d), dtype=np.float32)
            kc = rng.standard_normal((PF_N_KV, max_seq, d), dtype=np.float32)
            vc = rng.standard_normal((PF_N_KV, max_seq, d), dtype=np.float32)
            res[f"{tag}/{key}"] = sha(hb.op_attention_prefill(q, kc, vc, d ** -0.5, pos0))
            if not tq:
                continue
            signs = rng.choice(np.float32([-1.0, 1.0]), size=(PF_N_KV, 2, d))
            for t in (hb.KV_TQ2, hb.KV_TQ3):
                rb = d // 4 if t == hb.KV_TQ2 else d // 8 * 3
                kcodes = rng.integers(0, 256, (PF_N_KV, max_seq, rb), dtype=np.uint8)
                vcodes = rng.integers(0, 256, (PF_N_KV, max_seq, rb), dtype=np.uint8)
                res[f"prefill_tq_t{t}/{key}"] = sha(hb.op_attention_prefill_tq(t, q, kcodes, vcodes, signs, d ** -0.5, pos0))
            for t in (hb.KV_INT8, hb.KV_FP8_E4M3, hb.KV_FP8_E5M2):
                i8 = t == hb.KV_INT8
                kb = rng.integers(0, 256, (PF_N_KV, max_seq, d), dtype=np.uint8) if i8 else small_fp8(rng, (PF_N_KV, max_seq, d))
                vb = rng.integers(0, 256, (PF_N_KV, max_seq, d), dtype=np.uint8) if i8 else small_fp8(rng, (PF_N_KV, max_seq, d))
                ks = rng.uniform(0.002, 0.03, (PF_N_KV, max_seq)).astype(np.float32) if i8 else None
                vs = rng.uniform(0.002, 0.03, (PF_N_KV, max_seq)).astype(np.float32) if i8 else None
                res[f"prefill_kv8_t{t}/{key}"] = sha(hb.op_attention_prefill_kv8(t, q, kb, vb, ks, vs, d ** -0.5, pos0))


def run(valu_only):
    import __graft_entry__ as graft
    hb = graft.load_package().hip_backend
    res = {}
    if valu_only:
        prefill_cases(hb, res, "prefill_valu", False)
        return res
    prefill_cases(hb, res, "prefill", True)
    for d, g in SHAPES:
        nh, scale = N_KV * g, d ** -0.5
        for max_seq, pos in LENGTHS:
            rng = np.random.default_rng([11, d, g, max_seq, pos])
            key = f"d{d}g{g}/s{max_seq}p{pos}"
            q = rng.standard_normal((nh, d), dtype=np.float32)
            kc = rng.standard_normal((N_KV, max_seq, d), dtype=np.float32)
            vc = rng.standard_normal((N_KV, max_seq, d), dtype=np.float32)
            k_new = rng.standard_normal((N_KV, d), dtype=np.float32)
            v_new = rng.standard_normal((N_KV, d), dtype=np.float32)
            # ---- f32 cache
            res[f"decode_direct/{key}"] = sha(hb.op_attention_decode(hb.ATTN_DIRECT, q, kc, vc, scale, pos))
            res[f"decode_any/{key}"] = sha(hb.op_attention_decode(hb.ATTN_ANY, q, kc, vc, scale, pos))
            for ns in SPLITS:
                res[f"decode_split/{key}/n{ns}"] = sha(hb.op_attention_decode(hb.ATTN_SPLIT, q, kc, vc, scale, pos, ns))
                res[f"cached/{key}/n{ns}"] = sha(hb.op_attention_cached(q, kc, vc, scale, pos + 1, ns))
            # ---- multi-sequence: 3 sequences, distinct slots, distinct positions
            mpos = multi_positions(pos, max_seq)
            qm = rng.standard_normal((3, nh, d), dtype=np.float32)
            kcm = rng.standard_normal((4, N_KV, max_seq, d), dtype=np.float32)
            vcm = rng.standard_normal((4, N_KV, max_seq, d), dtype=np.float32)
            knm = rng.standard_normal((3, N_KV, d), dtype=np.float32)
            vnm = rng.standard_normal((3, N_KV, d), dtype=np.float32)
            for ns in SPLITS:
                res[f"decode_multi/{key}/n{ns}"] = sha(hb.op_attention_decode_multi(qm, kcm, vcm, scale, mpos, SLOTS, ns))
            # ---- byte caches
            for t in (hb.KV_INT8, hb.KV_FP8_E4M3, hb.KV_FP8_E5M2):
                i8 = t == hb.KV_INT8
                kb = rng.integers(0, 256, (N_KV, max_seq, d), dtype=np.uint8) if i8 else small_fp8(rng, (N_KV, max_seq, d))
                vb = rng.integers(0, 256, (N_KV, max_seq, d), dtype=np.uint8) if i8 else small_fp8(rng, (N_KV, max_seq, d))
                ks = rng.uniform(0.002, 0.03, (N_KV, max_seq)).astype(np.float32) if i8 else None
                vs = rng.uniform(0.002, 0.03, (N_KV, max_seq)).astype(np.float32) if i8 else None
                kbm = rng.integers(0, 256, (4, N_KV, max_seq, d), dtype=np.uint8) if i8 else small_fp8(rng, (4, N_KV, max_seq, d))
                vbm = rng.integers(0, 256, (4, N_KV, max_seq, d), dtype=np.uint8) if i8 else small_fp8(rng, (4, N_KV, max_seq, d))
                ksm = rng.uniform(0.002, 0.03, (4, N_KV, max_seq)).astype(np.float32) if i8 else None
                vsm = rng.uniform(0.002, 0.03, (4, N_KV, max_seq)).astype(np.float32) if i8 else None
                for ns in SPLITS:
                    out, k2, v2, ks2, vs2 = hb.op_attention_kv8(t, q, kb, vb, ks, vs, k_new, v_new, scale, pos, ns)
                    res[f"kv8_t{t}/{key}/n{ns}"] = sha(out, k2[:, pos], v2[:, pos], ks2[:, pos] if i8 else None, vs2[:, pos] if i8 else None)
                    out, k2, v2, ks2, vs2 = hb.op_attention_kv8_multi(t, qm, kbm, vbm, ksm, vsm, knm, vnm, scale, mpos, SLOTS, ns)
                    rows = [a[s, :, p] for a in (k2, v2) + ((ks2, vs2) if i8 else ()) for s, p in zip(SLOTS, mpos)]
                    res[f"kv8_multi_t{t}/{key}/n{ns}"] = sha(out, *rows)
            # ---- TurboQuant caches
            signs = rng.choice(np.float32([-1.0, 1.0]), size=(N_KV, 2, d))
            for t in (hb.KV_TQ2, hb.KV_TQ3, hb.KV_TQ2_QJL, hb.KV_TQ3_QJL):
                bits = 2 if t in (hb.KV_TQ2, hb.KV_TQ2_QJL) else 3
                qjl = t in (hb.KV_TQ2_QJL, hb.KV_TQ3_QJL)
                rb = d // 4 if bits == 2 else d // 8 * 3
                kcodes = rng.integers(0, 256, (N_KV, max_seq, rb), dtype=np.uint8)
                vcodes = rng.integers(0, 256, (N_KV, max_seq, rb), dtype=np.uint8)
                kx = S = None
                if qjl:
                    kx = rng.integers(0, 1 << 32, (N_KV, max_seq, d // 32 + 1), dtype=np.uint32)
                    kx[:, :, d // 32] = rng.uniform(0.0, 0.5, (N_KV, max_seq)).astype(np.float32).view(np.uint32)   # the residual norms
                    S = rng.standard_normal((N_KV, d, d), dtype=np.float32)
                for ns in SPLITS:
                    out, k2, v2, x2 = hb.op_attention_tq(t, q, kcodes, vcodes, kx, k_new, v_new, signs, S, scale, pos, ns)
                    res[f"tq_t{t}/{key}/n{ns}"] = sha(out, k2[:, pos], v2[:, pos], x2[:, pos] if qjl else None)
        print(f"head_dim {d}, {g} per kv head: {len(res)} cases so far", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True, help="JSON file: {entry point/shape: sha256 over its cases}")
    ap.add_argument("--full", help="JSON file: {case: sha256}")
    ap.add_argument("--valu-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.valu_child:
        json.dump(run(True), open(args.out, "w"))
        return
    # the VALU prompt kernel is chosen once per process, by the environment: a fresh child, before this process opens the GPU
    tmp = args.out + ".valu.tmp"
    subprocess.run([sys.executable, os.path.abspath(__file__), "--valu-child", "--out", tmp], check=True, env=dict(os.environ, LGH_PF_ATTN_VALU="1"))
    res = json.load(open(tmp))
    os.remove(tmp)
    res.update(run(False))
    if args.full:
        json.dump(res, open(args.full, "w"), indent=0, sort_keys=True)
    groups = {}
    for case in sorted(res):   # "<entry point>/d<head_dim>g<group size>/..."
        groups.setdefault("/".join(case.split("/")[:2]), hashlib.sha256()).update(f"{case} {res[case]}\n".encode())
    out = {"cases": len(res), "groups": {k: h.hexdigest() for k, h in groups.items()}}
    json.dump(out, open(args.out, "w"), indent=0, sort_keys=True)
    print(f"{len(res)} cases in {len(groups)} groups -> {args.out}; digest of all: {hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest()}")


if __name__ == "__main__":
    main()
