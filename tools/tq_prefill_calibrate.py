#!/usr/bin/env python3
"""Calibrates the model-level tolerance factor K of the batched prompt pass over a TurboQuant KV cache
(tests/test_gpu_tq_prefill.py::test_model_parity; profiles/README.md "TurboQuant prompt pass: the tolerance factor K").

TurboQuant codes are discontinuous: an f16-level change of a K / V row can move a coordinate into the neighbouring Lloyd-Max cell,
so the f16 GEMM path's error shows larger in the logits over a TurboQuant cache than over the f32 cache.  How much larger is measured:

  (a)  GPU:  python tools/tq_prefill_calibrate.py --measure-a
       the f32 batched path's max|dlogit| / tol against the oracle, per model (tol = 1e-2 max|logit| + 1e-2)
  (b)  CPU:  python tools/tq_prefill_calibrate.py --a test-dense=A1,test-dense-d128=A2,test-moe=A3
       the oracle alone: attn_norm / ffn_norm weights times (1 + eps u), u uniform in [-1, 1]; eps scaled until the f32-cache oracle's
       perturbed-versus-unperturbed ratio reproduces (a) (the response is linear); at that eps the TurboQuant oracle's ratio, bits 2
       and 3, 5 perturbation seeds
  (c)  K = 2 x the largest ratio of (b)

Prompts of 70 and 300 tokens, then 4 tokens, as the test runs them."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import tq_prefill_ref as tr      # noqa: E402

MODELS = [("test-dense", "Q4_K_M"), ("test-dense-d128", "Q4_K_M"), ("test-moe", "Q5_K_M")]
PROMPTS = (70, 300)
EPS0 = 2.0 ** -11


def worst(steps):
    return max(err / tol for err, tol, _, _ in steps)


def measure_a(pkg, orc):
    for name, mix in MODELS:
        ratios = []
        for n in PROMPTS:
            cfg = pkg.make_config(name, max_seq_len=n + 8)
            model = pkg.SynthModel(cfg, mix=mix)
            ref = tr.oracle_model(orc, cfg, model)
            eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
            assert eng.prefill_is_batched()
            prompt = tr.prompt_tokens(cfg, n)
            eng.forward_batch(prompt)
            ratios.append(worst(tr.follow(orc, eng.forward, ref, prompt)))
            eng.close()
            ref.close()
        print(f"(a) {name}/{mix}: f32 batched path max|dlogit| / tol = {max(ratios):.4f}  (prompts {PROMPTS}: {['%.4f' % r for r in ratios]})", flush=True)


def perturbed(eps, seed):
    def f(name, data):
        if not (name.endswith("attn_norm.weight") or name.endswith("ffn_norm.weight")):
            return data
        w = np.ascontiguousarray(data).view(np.float32)
        rng = np.random.default_rng([seed, len(name), int(name.split(".")[1])])
        return (w * (1.0 + eps * rng.uniform(-1.0, 1.0, w.shape))).astype(np.float32).view(np.asarray(data).dtype)
    return f


def oracle_ratio(pkg, orc, name, mix, n, eps, seed, bits):
    """max|dlogit| / tol of the oracle with perturbed norm weights against the unperturbed oracle; bits 0: the f32 cache."""
    cfg = pkg.make_config(name, max_seq_len=n + 8)
    model = pkg.SynthModel(cfg, mix=mix)
    ref, per = tr.oracle_model(orc, cfg, model), tr.oracle_model(orc, cfg, model, perturbed(eps, seed))
    if bits:
        signs = tr.model_signs(cfg, 7 + bits)
        ref.set_kv_turboquant(bits, signs)
        per.set_kv_turboquant(bits, signs)
    prompt = tr.prompt_tokens(cfg, n)
    per.forward(prompt)
    r = worst(tr.follow(orc, lambda tok: per.forward([tok]), ref, prompt))
    ref.close()
    per.close()
    return r


def calibrate(pkg, orc, a):
    biggest = 0.0
    for name, mix in MODELS:
        base = max(oracle_ratio(pkg, orc, name, mix, n, EPS0, 0, 0) for n in PROMPTS)
        eps = EPS0 * a[name] / base
        check = max(oracle_ratio(pkg, orc, name, mix, n, eps, 0, 0) for n in PROMPTS)
        print(f"(b) {name}/{mix}: f32-cache oracle moves {base:.4f} tol at eps 2^-11; (a) = {a[name]:.4f} -> eps = {eps:.3e} = 2^{np.log2(eps):.2f} "
              f"(f32-cache oracle at that eps: {check:.4f})", flush=True)
        for bits in (2, 3):
            rs = [max(oracle_ratio(pkg, orc, name, mix, n, eps, seed, bits) for n in PROMPTS) for seed in range(5)]
            biggest = max(biggest, max(rs))
            print(f"(b) {name}/{mix} tq{bits}: perturbed / unperturbed over 5 seeds = {['%.3f' % r for r in rs]}", flush=True)
    print(f"(c) largest ratio {biggest:.3f} -> K = {2 * biggest:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure-a", action="store_true")
    ap.add_argument("--a", default="")
    args = ap.parse_args()
    pkg, orc = graft.load_package(), graft.load_oracle()
    orc.set_threads(min(16, os.cpu_count() or 1))
    if args.measure_a:
        measure_a(pkg, orc)
    if args.a:
        calibrate(pkg, orc, {k: float(v) for k, v in (kv.split("=") for kv in args.a.split(","))})


if __name__ == "__main__":
    main()
