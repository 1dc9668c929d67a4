#!/usr/bin/env python3
"""What sampling on the device costs per token (csrc/sample.hip): `python tools/sample_bench.py [--model M --mix X --prompt N
--steps K --reps R --batches 8,16]`.  One JSON line per row, then a summary line; every row is the mean (and min) over R
timed repetitions of a K-step decode after an N-token prompt.

  decode_greedy                  lgh_decode_greedy (the arg-max graph; bench.py's headline path)
  decode_sample engine_default   lgh_decode_sample with EngineConfig::default's settings (T 0.7, top-k 40, top-p 0.95, rp 1.1)
  decode_sample creative         ... with SamplerConfig::creative (T 1.0, top-k 0, top-p 0.9, rp 1.2) without its min_p
  decode_sample creative_ref     ... with SamplerConfig::creative as the reference has it (min_p 0.05)
  decode_sample mirostat_v2      ... with SamplerConfig::mirostat_v2(5.0, 0.1)
  forward + host sampler         lgh_forward (full logits to the host) + the numpy restatement of Sampler::sample
                                 (tests/sampler_ref.py) on the host: the path a host with a sampling config has without this
  multi B greedy / sample        lgh_decode_greedy_multi / lgh_decode_sample_multi with B sequences (aggregate tokens/s)
  op_sample peaked <config>      lgh_op_sample on confident logits (top probability > 0.9, vocabulary of the model): ms per call,
                                 median of 10 calls.  Each call also sets up and tears down its buffers, so the difference between
                                 rows, not the value, is the sampling kernels' cost; engine_default is the fast-path reference."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
from sampler_ref import Sampler  # noqa: E402
from sampler_ref_ex import PRESETS_EX as PRESETS  # noqa: E402


def timed(reps, prepare, run):
    ts = []
    for _ in range(reps):
        prepare()
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    return float(np.mean(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--mix", default="Q4_K_M")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="8,16")
    a = ap.parse_args()
    pkg = graft.load_package()
    batches = [int(b) for b in a.batches.split(",") if b]
    cfg = pkg.make_config(a.model, max_seq_len=a.prompt + a.steps + 16)
    model = pkg.SynthModel(cfg, mix=a.mix)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    prompt = [(i * 7919) % cfg.vocab_size for i in range(a.prompt)]
    K = a.steps
    rng = np.random.default_rng(0)
    unis = rng.random(K, dtype=np.float32)
    rows = []

    def emit(name, mean, best, per, extra=None):
        row = dict(row=name, ms_per_token=1e3 * mean / per, min_ms_per_token=1e3 * best / per, steps=K, reps=a.reps)
        row.update(extra or {})
        rows.append(row)
        print(json.dumps(row), flush=True)

    def fresh(sampler=None):
        def f():
            eng.reset()
            eng.forward_batch(prompt[:-1])
            if sampler:
                eng.set_sampler(**PRESETS[sampler])
            eng.synchronize()
        return f

    fresh()()
    eng.decode_greedy(prompt[-1], 8)   # graphs captured outside the timed regions
    decode_presets = ("engine_default", "creative", "creative_ref", "mirostat_v2")
    for preset in decode_presets:
        fresh(preset)()
        eng.decode_sample(prompt[-1], prompt[:-1], 8, unis)
    m, b = timed(a.reps, fresh(), lambda: eng.decode_greedy(prompt[-1], K))
    emit("decode_greedy", m, b, K)
    greedy_ms = 1e3 * m / K
    for preset in decode_presets:
        m, b = timed(a.reps, fresh(preset), lambda: eng.decode_sample(prompt[-1], prompt[:-1], K, unis))
        emit(f"decode_sample {preset}", m, b, K, dict(extra_us_per_token=1e3 * (1e3 * m / K - greedy_ms)))

    def host_path():
        s = Sampler(cfg.vocab_size, **PRESETS["engine_default"])
        ctx, tok = list(prompt), prompt[-1]
        for i in range(K):
            tok = s.sample(eng.forward(tok), ctx, float(unis[i]))
            ctx.append(tok)
    m, b = timed(a.reps, fresh(), host_path)
    emit("forward + host sampler engine_default", m, b, K)

    if batches:
        eng.batch_create(max(batches))
        for B in batches:
            slots = list(range(B))

            def prep(sample):
                def f():
                    for s in slots:
                        eng.batch_reset(s)
                        eng.batch_prefill(s, prompt[:-1])
                        if sample:
                            eng.batch_set_sampler(s, **PRESETS["engine_default"])
                    eng.synchronize()
                return f
            ub = rng.random((K, B), dtype=np.float32)
            hist = [prompt[:-1]] * B
            prep(False)()
            eng.decode_greedy_multi(slots, [prompt[-1]] * B, 4)
            prep(True)()
            eng.decode_sample_multi(slots, [prompt[-1]] * B, hist, 4, ub)
            mg, bg = timed(a.reps, prep(False), lambda: eng.decode_greedy_multi(slots, [prompt[-1]] * B, K))
            emit(f"multi B={B} decode_greedy_multi", mg, bg, K, dict(aggregate_tok_s=B * K / mg))
            ms, bs = timed(a.reps, prep(True), lambda: eng.decode_sample_multi(slots, [prompt[-1]] * B, hist, K, ub))
            emit(f"multi B={B} decode_sample_multi", ms, bs, K, dict(aggregate_tok_s=B * K / ms, vs_greedy=mg / ms))
    # confident steps: one token far above a broad body (p0 > 0.9 at T 1), as a real model's logits mostly are
    peaked = []
    for _ in range(10):
        x = rng.normal(0.0, 1.0, cfg.vocab_size).astype(np.float32)
        x[rng.integers(0, cfg.vocab_size)] += 18.0
        peaked.append(x)
    p0 = min(float(Sampler(cfg.vocab_size, **PRESETS["creative"]).probs(x, []).max()) for x in peaked)
    hb = pkg.hip_backend
    for name, conf in (("engine_default", PRESETS["engine_default"]), ("creative", PRESETS["creative"]),
                       ("creative_ref", PRESETS["creative_ref"]), ("mirostat_v2", PRESETS["mirostat_v2"]),
                       ("mirostat_v1", dict(PRESETS["mirostat_v2"], mirostat=1)),
                       ("top_k 0 top_p 1", dict(temperature=1.0, top_k=0, top_p=1.0, repeat_penalty=1.0, repeat_window=0))):
        hb.op_sample(peaked[0], uniform=0.5, **conf)
        ts = []
        for i, x in enumerate(peaked):
            t0 = time.perf_counter()
            hb.op_sample(x, uniform=float(unis[i]), **conf)
            ts.append(time.perf_counter() - t0)
        row = dict(row=f"op_sample peaked {name}", ms_per_call=1e3 * float(np.median(ts)), min_ms_per_call=1e3 * min(ts),
                   calls=len(ts), min_top_probability=p0)
        rows.append(dict(row, ms_per_token=row["ms_per_call"]))
        print(json.dumps(row), flush=True)
    print(json.dumps(dict(summary=True, model=a.model, mix=a.mix, prompt=a.prompt, steps=K, reps=a.reps,
                          rows={r["row"]: round(r["ms_per_token"], 4) for r in rows})))
    eng.close()


if __name__ == "__main__":
    main()
