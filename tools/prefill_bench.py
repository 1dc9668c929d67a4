#!/usr/bin/env python3
"""Times lgh_prefill_batch alone (the batched f16-GEMM prompt path): `python tools/prefill_bench.py [--model M --mix X
--prompt N --iters I --kv f32|tq2|tq3|... --policy P]`; run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
--kv selects the KV cache type (f32 and the TurboQuantMSE types tq2 / tq3 have the batched path; int8 / fp8-* have it with
--policy 1 = PREFILL_BATCH_BYTE_KV (lgh_set_prefill_policy); the others run token by token)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--mix", default="Q4_K_M")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--kv", default="f32", choices=["f32", "int8", "fp8-e4m3", "fp8-e5m2", "tq2", "tq3", "tq2-qjl", "tq3-qjl"])
    ap.add_argument("--policy", type=int, default=0, help="lgh_set_prefill_policy word (1: int8 / FP8 caches take the batched pass)")
    a = ap.parse_args()
    pkg = graft.load_package()
    hb = pkg.hip_backend
    kv = {"f32": hb.KV_F32, "int8": hb.KV_INT8, "fp8-e4m3": hb.KV_FP8_E4M3, "fp8-e5m2": hb.KV_FP8_E5M2, "tq2": hb.KV_TQ2, "tq3": hb.KV_TQ3,
          "tq2-qjl": hb.KV_TQ2_QJL, "tq3-qjl": hb.KV_TQ3_QJL}[a.kv]
    cfg = pkg.make_config(a.model, max_seq_len=max(512, a.prompt + 16))
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix=a.mix), cfg.max_seq_len, kv_cache_type=kv, prefill_policy=a.policy)
    prompt = [i % 32000 % cfg.vocab_size for i in range(a.prompt)]
    eng.forward_batch(prompt)
    times = []
    for _ in range(a.iters):
        eng.reset()
        eng.synchronize()
        t0 = time.perf_counter()
        eng.forward_batch(prompt)
        eng.synchronize()
        times.append(time.perf_counter() - t0)
    times.sort()
    best = times[0]
    print(f"{a.model} {a.mix} kv={a.kv} policy={a.policy}: {a.prompt} prompt tokens, batched={eng.prefill_is_batched()}, best {1e3 * best:.3f} ms "
          f"= {a.prompt / best:.0f} tokens/s (median {1e3 * times[len(times) // 2]:.3f}, max {1e3 * times[-1]:.3f} ms over {a.iters})")
    eng.close()


if __name__ == "__main__":
    main()
