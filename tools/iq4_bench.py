#!/usr/bin/env python3
"""IQ4_NL / IQ4_XS weights in their tile layouts (lgh_set_weight_policy: WEIGHTS_IQ4_TILES = 16) against the f32-expanded path:
`python tools/iq4_bench.py [--model M --mix IQ4_NL --policies 16,0 --steps N --prompt P --reps R]`, one JSON line per measurement.

One engine per policy word over the same synthetic weights, measured alternately, R repetitions each, best and median reported:
  decode   ms per token of lgh_decode_greedy over N steps (captured graph replays, one device synchronise at the end) after a warm-up run
  prompt   ms of lgh_prefill_batch over P tokens — the batched pass with the policy, token by token without it (no tile layout, no
           batched path) — and of P lgh_prefill_token calls on the policy engine
`--policies 0` measures the expanded path alone: that form also runs on a checkout that does not know the bit, which is how the parent
commit's expanded path is put beside this one's (profiles/iq4_weights.md)."""
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
    ap.add_argument("--mix", default="IQ4_NL")
    ap.add_argument("--policies", default="16,0")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    pkg = graft.load_package()
    cfg = pkg.make_config(a.model, max_seq_len=max(512, a.prompt + a.steps + 16))
    model = pkg.SynthModel(cfg, mix=a.mix)
    engines = {p: pkg.HipGpuInference.from_model(model, cfg.max_seq_len, weight_policy=p) for p in (int(w) for w in a.policies.split(","))}
    prompt = [(7 * i + 3) % cfg.vocab_size for i in range(a.prompt)]
    res = {(p, what): [] for p in engines for what in ("decode", "prompt", "prompt_tokenwise")}
    for rep in range(a.reps + 1):                      # repetition 0 warms every path up and is dropped
        for p, eng in engines.items():
            eng.reset()
            res[p, "prompt"].append(timed(eng, lambda: eng.forward_batch(prompt)))
            res[p, "decode"].append(timed(eng, lambda: eng.decode_greedy(prompt[-1], a.steps)) / a.steps)
            if p:
                eng.reset()
                res[p, "prompt_tokenwise"].append(timed(eng, lambda: [eng.prefill_token(t) for t in prompt]))
    for (p, what), ms in sorted(res.items()):
        ms = sorted(ms[1:])
        if ms:
            eng = engines[p]
            print(json.dumps({"tag": a.tag, "model": a.model, "mix": a.mix, "weight_policy": p, "what": what, "best_ms": round(ms[0], 4),
                              "median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4), "reps": len(ms),
                              "steps": a.steps if what == "decode" else a.prompt, "batched_prompt": eng.prefill_is_batched(),
                              "weight_bytes": eng.stats()["weight_bytes"]}), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
