#!/usr/bin/env python3
"""F16 / BF16 weights kept 16-bit in HBM (lgh_set_weight_policy: WEIGHTS_HALF_TILES) against the same build's f32 expansion:
`python tools/half_bench.py [--model M --mix F16 --policy 4 --steps N --prompt P --reps R]`, one JSON line per measurement.

ONE engine per process — an F16 Llama-3-8B is 16 GB with the policy and 32 GB without — so alternate fresh processes with --policy 4 and
--policy 0 and compare; the spread between processes of one policy is part of the result (profiles/half_weights.md).  A quantized mix
(--mix Q8_0 --policy 0) gives the yardstick "a tile format at its byte count" from the same session.
  decode   ms per token of lgh_decode_greedy over N steps (captured graph replays, one device synchronise at the end) after a warm-up
           run, and the bytes of the matrices a step streams (resident weights minus the embedding table) per second
  prompt   ms of lgh_prefill_batch over P tokens: the batched pass with the policy (and for a tile format), token by token through the
           f32 mat-vec without it"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def timed(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--mix", default="F16")
    ap.add_argument("--policy", type=int, default=4)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pkg = graft.load_package()
    cfg = pkg.make_config(a.model, max_seq_len=max(512, a.prompt + a.steps + 16))
    model = pkg.SynthModel(cfg, mix=a.mix)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len, weight_policy=a.policy)
    embd = next(s.nbytes for s in model.specs() if s.name == "token_embd.weight")
    streamed = eng.stats()["weight_bytes"] - embd
    prompt = [(7 * i + 3) % cfg.vocab_size for i in range(a.prompt)]
    res = {"decode": [], "prompt": []}
    for rep in range(a.reps + 1):                      # repetition 0 warms every path up and is dropped
        eng.reset()
        res["prompt"].append(timed(eng, lambda: eng.forward_batch(prompt)))
        res["decode"].append(timed(eng, lambda: eng.decode_greedy(prompt[-1], a.steps)) / a.steps)
    for what, ms in sorted(res.items()):
        ms = sorted(ms[1:])
        row = {"model": a.model, "mix": a.mix, "weight_policy": a.policy, "what": what, "best_ms": round(ms[0], 4),
               "median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4), "reps": len(ms),
               "steps": a.steps if what == "decode" else a.prompt, "batched_prompt": eng.prefill_is_batched(),
               "weight_bytes": eng.stats()["weight_bytes"]}
        if what == "decode":
            row["streamed_gb_per_s"] = round(streamed / ms[len(ms) // 2] / 1e6, 1)
        print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
