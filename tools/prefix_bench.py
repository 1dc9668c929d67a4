#!/usr/bin/env python3
"""Times the device prompt cache against recomputing the prompt (profiles/prefix_cache.md).

  --mode copy        lgh_prefix_save / lgh_prefix_restore of a prefix of N rows, own sequence and a slot: best (median .. max) of
                     --reps calls, each between two stream synchronisations, after --warm untimed calls.  The rows are zeros put
                     there by an import (a copy's time does not depend on the bytes), so no prompt is computed in this mode.
                     Traffic = 2 x the prefix's bytes (read + written), next to the 6.29 TB/s float4-copy rate of the MI355X.
  --mode recompute   the same prompts computed: forward_batch on the own sequence (the batched pass for f32 / tq2 / tq3, token by
                     token otherwise) and batch_prefill on a slot.  Uses entry points older than the prompt cache only, so
                     --root can point it at a checkout of the parent commit (built there) to time that library.
                     --policy 1 (PREFILL_BATCH_BYTE_KV, lgh_set_prefill_policy) sends int8 / FP8 prompts, slots included, through
                     the batched pass; 0, the default, calls nothing a parent checkout lacks.

`python tools/prefix_bench.py --mode copy|recompute [--root DIR] [--kv f32,int8,tq3,tq3-qjl] [--lengths 128,512,2048]`;
prints one JSON line per (format, length, target) and a markdown table."""
import argparse
import json
import os
import struct
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KV = {"f32": 0, "int8": 1, "fp8-e4m3": 2, "fp8-e5m2": 3, "tq2": 4, "tq3": 5, "tq2-qjl": 6, "tq3-qjl": 7}
COPY_RATE = 6.29e12   # bytes/s, float4 copy, read + write


def timed(eng, fn, reps, warm, before=None):
    out = []
    for i in range(warm + reps):
        if before:
            before()
        eng.synchronize()
        t0 = time.perf_counter()
        r = fn()
        eng.synchronize()
        dt = time.perf_counter() - t0
        if i >= warm:
            out.append(dt)
        if hasattr(r, "free"):
            r.free()
    out.sort()
    return out


def stat(ts):
    return {"best_us": 1e6 * ts[0], "median_us": 1e6 * ts[len(ts) // 2], "max_us": 1e6 * ts[-1], "reps": len(ts)}


def zero_blob(cfg, hb, kv, n, max_seq):
    lay = hb.kv_cache_layout(kv, cfg.num_kv_heads, max_seq, cfg.head_dim)
    payload = cfg.num_layers * cfg.num_kv_heads * n * (2 * (lay.row_bytes + lay.scale_bytes) + lay.qjl_bytes)
    head = struct.pack("<8IQ", 0x5850474C, 1, kv, cfg.num_kv_heads, cfg.head_dim, 0, cfg.num_layers, n, payload)
    return head + bytes(payload)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["copy", "recompute"])
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are timed")
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--mix", default="Q4_K_M")
    ap.add_argument("--kv", default="f32,int8,tq3,tq3-qjl")
    ap.add_argument("--lengths", default="128,512,2048")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--policy", type=int, default=0, help="lgh_set_prefill_policy word, set on every engine when not 0")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import __graft_entry__ as graft
    pkg = graft.load_package()
    hb = pkg.hip_backend
    lengths = [int(x) for x in a.lengths.split(",")]
    max_seq = max(lengths) + 64
    cfg = pkg.make_config(a.model, max_seq_len=max_seq)
    model = pkg.SynthModel(cfg, mix=a.mix)
    rows = []
    for name in a.kv.split(","):
        kv = KV[name]
        eng = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=kv)
        if a.policy:
            eng.set_prefill_policy(a.policy)
        eng.batch_create(1)
        for n in lengths:
            prompt = [(7 * i + 3) % cfg.vocab_size for i in range(n)]
            for target, slot in (("own", -1), ("slot", 0)):
                rec = {"mode": a.mode, "model": a.model, "mix": a.mix, "kv": name, "policy": a.policy, "n": n, "target": target}
                if a.mode == "copy":
                    src = eng.prefix_from_bytes(zero_blob(cfg, hb, kv, n, max_seq))
                    eng.prefix_restore(src, slot)
                    rec["bytes"] = src.nbytes
                    rec["save"] = stat(timed(eng, lambda: eng.prefix_save(n, slot), a.reps, a.warm))   # (allocation included)
                    rec["restore"] = stat(timed(eng, lambda: eng.prefix_restore(src, slot), a.reps, a.warm))
                    for k in ("save", "restore"):
                        rec[k]["traffic_TBps"] = 2 * src.nbytes / (rec[k]["best_us"] * 1e-6) / 1e12
                    src.free()
                else:
                    batched = eng.prefill_is_batched() if slot < 0 else name == "f32" or (eng.prefill_is_batched() and KV[name] in (1, 2, 3))
                    reps, warm = (a.reps, a.warm) if batched else (3, 1)
                    if slot < 0:
                        ts = timed(eng, lambda: eng.forward_batch(prompt), reps, warm, before=eng.reset)
                    else:
                        ts = timed(eng, lambda: eng.batch_prefill(0, prompt), reps, warm, before=lambda: eng.batch_reset(0))
                    rec["recompute"] = stat(ts)
                    rec["us_per_token"] = rec["recompute"]["best_us"] / n
                rows.append(rec)
                print(json.dumps(rec), flush=True)
        eng.close()

    def cell(s):
        return f"{s['best_us']:.0f} ({s['median_us']:.0f} .. {s['max_us']:.0f})"
    if a.mode == "copy":
        print("\n| cache | rows | target | MB | save us | restore us | save TB/s | restore TB/s | restore / 6.29 TB/s |\n|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['kv']} | {r['n']} | {r['target']} | {r['bytes'] / 1e6:.1f} | {cell(r['save'])} | {cell(r['restore'])} | "
                  f"{r['save']['traffic_TBps']:.2f} | {r['restore']['traffic_TBps']:.2f} | {r['restore']['traffic_TBps'] * 1e12 / COPY_RATE:.0%} |")
    else:
        print("\n| cache | tokens | target | recompute us | us per token |\n|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['kv']} | {r['n']} | {r['target']} | {cell(r['recompute'])} | {r['us_per_token']:.1f} |")


if __name__ == "__main__":
    main()
