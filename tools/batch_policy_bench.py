#!/usr/bin/env python3
"""Multi-sequence decode, the default path against lgh_set_batch_policy(LGH_BATCH_F32_MATRIX), by `bench.py --batch`'s protocol:
Llama-3-8B Q4_K_M, 128-token prompts (sequence s: the bench prompt shifted by 977 s), the greedy loop on the device.

    python tools/batch_policy_bench.py [--seqs 2,4,5,6,8,12,16 --steps 64 --warmup 4 --reps 5 --root TREE]

One context with 16 slots serves every sequence count.  Every repetition starts from the same cache state: the slots are reset and
take their prompts again, then `warmup` untimed steps, then `steps` timed ones.  Per count the two paths alternate repetition by
repetition.  One JSON line per (count, path): best and median ms per step, aggregate tokens/s of the best.
--root TREE measures another checkout of the project (the parent commit, built there); a tree without the policy gives the default
path only.  A driver that compares commits runs this once per tree, alternately, each run under its own `timeout`, chained with &&."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--mix", default="Q4_K_M")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--seqs", default="2,4,5,6,8,12,16")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seq", type=int, default=2, help="the policy's minimum sequence count (bits 8..15 of the word)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    max_seq = max(512, a.prompt + a.warmup + a.steps + 16)
    cfg = pkg.make_config(a.model, max_seq_len=max_seq)
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix=a.mix), max_seq)
    eng.batch_create(16)
    has_policy = hasattr(eng, "set_batch_policy")
    prompts = [[(i % 32000 % cfg.vocab_size + 977 * s) % cfg.vocab_size for i in range(a.prompt)] for s in range(16)]
    paths = [("default", 0)] + ([("f32_matrix", 1 | a.min_seq << 8)] if has_policy else [])

    def rep(B, word):
        slots = list(range(B))
        for s in slots:
            eng.batch_reset(s)
            eng.batch_prefill(s, prompts[s][:-1])
        if has_policy:
            eng.set_batch_policy(word)
        warm = eng.decode_greedy_multi(slots, [p[-1] for p in prompts[:B]], 1 + a.warmup)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.decode_greedy_multi(slots, [int(t) for t in warm[-1]], a.steps)
        eng.synchronize()
        return (time.perf_counter() - t0) / a.steps

    for B in [int(v) for v in a.seqs.split(",")]:
        times = {name: [] for name, _ in paths}
        for _ in range(a.reps):
            for name, word in paths:
                times[name].append(rep(B, word))
        for name, _ in paths:
            best, med = min(times[name]), statistics.median(times[name])
            print(json.dumps({"tree": a.label, "path": name, "seqs": B, "ms_per_step_best": round(1e3 * best, 4),
                              "ms_per_step_median": round(1e3 * med, 4), "tokens_per_s_best": round(B / best, 1), "reps": a.reps,
                              "steps": a.steps}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
