#!/usr/bin/env python3
"""Decode attention of a group size without split kernels (lgh_model_desc.attn_policy: ATTN_GROUP_MATRIX = 1) against the default,
attn_decode_any_kernel: `python tools/attn_group_bench.py [--model llama-3.2-3b --mix Q4_K_M --rows 272,4000 --steps 32 --reps 3]`, one
JSON line per measurement (profiles/attn_group.md).

One engine per policy word over the same synthetic weights, measured alternately; repetition 0 warms every path up and is dropped:
  decode   tokens/s of lgh_decode_greedy over --steps steps ending at each of --rows cached rows (graph replays, one synchronise)
  prompt   ms of lgh_prefill_batch over 128 tokens: the batched pass with the bit, token by token without it
`--kernels POS --max-seq M`: no engine; the two attention launches through lgh_op_attention_decode at position POS of an M-row cache, the
model's head shape and the engine's split count, alternately, for a `rocprofv3 --kernel-trace --stats` run of its own.
`--kv f32,int8,fp8_e4m3[,fp8_e5m2]`: the cache types instead of the policy words, every engine WITH the bit (profiles/attn_group_kv8.md):
decode as above (a byte cache's prompt goes token by token, so no prompt figure), every line with the engine's lgh_stats.kv_bytes; with
`--kernels`, attn_group_kernel and attn_group_kv8_kernel (lgh_op_attention_kv8) alternately."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def timed(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3.2-3b")
    ap.add_argument("--mix", default="Q4_K_M")
    ap.add_argument("--rows", default="272,4000")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=-1)
    ap.add_argument("--max-seq", type=int, default=4096)
    ap.add_argument("--kv", default="")
    a = ap.parse_args()
    pkg = graft.load_package()
    hb = pkg.hip_backend
    kv_types = {"f32": hb.KV_F32, "int8": hb.KV_INT8, "fp8_e4m3": hb.KV_FP8_E4M3, "fp8_e5m2": hb.KV_FP8_E5M2}
    kvs = [kv_types[k] for k in a.kv.split(",")] if a.kv else []
    if a.kernels >= 0:
        cfg = pkg.make_config(a.model)
        rng = np.random.default_rng(1)
        q = rng.standard_normal((cfg.num_heads, cfg.head_dim)).astype(np.float32)
        k, v = (rng.standard_normal((cfg.num_kv_heads, a.max_seq, cfg.head_dim)).astype(np.float32) for _ in range(2))
        scale, splits = cfg.head_dim ** -0.5, min(32, 256 // cfg.num_kv_heads)
        kb, vb = (rng.integers(1, 0x40, k.shape).astype(np.uint8) for _ in range(2))   # finite in every byte format
        ks, vs = (rng.uniform(0.005, 0.03, k.shape[:2]).astype(np.float32) for _ in range(2))
        for _ in range(a.reps + 1):
            for path in (hb.ATTN_GROUP, hb.ATTN_ANY) if not kvs else ():
                hb.op_attention_decode(path, q, k, v, scale, a.kernels, splits)
            for kv in kvs:
                if kv == hb.KV_F32:
                    hb.op_attention_decode(hb.ATTN_GROUP, q, k, v, scale, a.kernels, splits)
                else:
                    hb.op_attention_kv8(kv, q, kb, vb, ks, vs, k[:, 0], v[:, 0], scale, a.kernels, splits)
        return
    rows = [int(r) for r in a.rows.split(",")]
    cfg = pkg.make_config(a.model, max_seq_len=max(rows) + 16)
    model = pkg.SynthModel(cfg, mix=a.mix)
    keys = [(hb.ATTN_GROUP_MATRIX, kv) for kv in kvs] if kvs else [(hb.ATTN_GROUP_MATRIX, hb.KV_F32), (0, hb.KV_F32)]   # (policy word, cache type)
    engines = {k: pkg.HipGpuInference.from_model(model, cfg.max_seq_len, attn_policy=k[0], kv_cache_type=k[1]) for k in keys}
    toks = [(7 * i + 3) % cfg.vocab_size for i in range(max(rows))]
    res = {}
    for rep in range(a.reps + 1):
        for k, eng in engines.items():
            eng.reset()
            if not kvs:
                res.setdefault((k, "prompt128_ms"), []).append(1e3 * timed(eng, lambda: eng.forward_batch(toks[:128])))
            for r in rows:
                eng.reset()
                eng.forward_batch(toks[:r - a.steps])
                res.setdefault((k, f"decode_tok_s_rows{r}"), []).append(a.steps / timed(eng, lambda: eng.decode_greedy(toks[-1], a.steps)))
    for (k, what), x in sorted(res.items()):
        x = sorted(x[1:])
        print(json.dumps({"model": a.model, "mix": a.mix, "attn_policy": k[0], "kv_cache_type": k[1], "what": what, "min": round(x[0], 3),
                          "median": round(x[len(x) // 2], 3), "max": round(x[-1], 3), "reps": len(x),
                          "batched_prompt": engines[k].prefill_is_batched(), "kv_bytes": engines[k].stats()["kv_bytes"]}), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
