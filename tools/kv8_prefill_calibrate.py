#!/usr/bin/env python3
"""Calibrates the model-level tolerance factor K of the batched prompt pass over the byte KV caches (int8, FP8 E4M3, FP8 E5M2;
tests/test_gpu_kv8_prefill.py::test_model_parity; profiles/README.md "Byte-cache prompt pass: the tolerance factor K").

The byte formats are discontinuous as the TurboQuant codes are: an f16-level change of a K / V row can move an element across a
rounding (int8) or truncation (FP8) boundary, and an int8 row's scale moves with its largest element.  The method is
tools/tq_prefill_calibrate.py's, with the oracle's byte caches in place of its TurboQuant cache:

  (a)  GPU:  python tools/tq_prefill_calibrate.py --measure-a        (the f32 batched path against the oracle; shared with TurboQuant)
  (b)  CPU:  python tools/kv8_prefill_calibrate.py --a test-dense=A1,test-dense-d128=A2,test-moe=A3
       the oracle alone, norm weights perturbed until its f32-cache logits move by (a); at that eps the int8 / E4M3 / E5M2 oracle's
       perturbed-versus-unperturbed ratio, 5 perturbation seeds
  (c)  K = 2 x the largest ratio of (b)

Nothing here runs the code under test."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as graft          # noqa: E402
import kv8_prefill_ref as kr             # noqa: E402
import tq_prefill_calibrate as tc        # noqa: E402
import tq_prefill_ref as tr              # noqa: E402


def oracle_ratio(pkg, orc, name, mix, n, eps, seed, kv_type):
    """max|dlogit| / tol of the oracle with perturbed norm weights against the unperturbed oracle, both with a kv_type cache."""
    cfg = pkg.make_config(name, max_seq_len=n + 8)
    model = pkg.SynthModel(cfg, mix=mix)
    ref, per = tr.oracle_model(orc, cfg, model), tr.oracle_model(orc, cfg, model, tc.perturbed(eps, seed))
    kr.set_oracle_format(orc, ref, kv_type)
    kr.set_oracle_format(orc, per, kv_type)
    prompt = tr.prompt_tokens(cfg, n)
    per.forward(prompt)
    r = tc.worst(tr.follow(orc, lambda tok: per.forward([tok]), ref, prompt))
    ref.close()
    per.close()
    return r


def calibrate(pkg, orc, a):
    biggest = 0.0
    for name, mix in tc.MODELS:
        base = max(tc.oracle_ratio(pkg, orc, name, mix, n, tc.EPS0, 0, 0) for n in tc.PROMPTS)
        eps = tc.EPS0 * a[name] / base
        print(f"(b) {name}/{mix}: f32-cache oracle moves {base:.4f} tol at eps 2^-11; (a) = {a[name]:.4f} -> eps = {eps:.3e} = 2^{np.log2(eps):.2f}",
              flush=True)
        for kv_type in kr.FORMATS:
            rs = [max(oracle_ratio(pkg, orc, name, mix, n, eps, seed, kv_type) for n in tc.PROMPTS) for seed in range(5)]
            biggest = max(biggest, max(rs))
            print(f"(b) {name}/{mix} {kr.NAMES[kv_type]}: perturbed / unperturbed over 5 seeds = {['%.3f' % r for r in rs]}", flush=True)
    print(f"(c) largest ratio {biggest:.3f} -> K = {2 * biggest:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True, help="test-dense=A1,test-dense-d128=A2,test-moe=A3: step (a)'s ratios")
    args = ap.parse_args()
    pkg, orc = graft.load_package(), graft.load_oracle()
    orc.set_threads(min(16, os.cpu_count() or 1))
    calibrate(pkg, orc, {k: float(v) for k, v in (kv.split("=") for kv in args.a.split(","))})


if __name__ == "__main__":
    main()
