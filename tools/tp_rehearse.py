#!/usr/bin/env python3
"""Tensor-parallel rehearsal on ONE GPU: every rank of lgh_tp_* on device 0, so every rank's bytes go through the same HBM and the
token's graph grows with the rank count.  It shows that the structure runs a full-size model and what it costs there; it says
nothing about N real GPUs, and it is expected to be SLOWER than the single context.

Llama-3-8B Q4_K_M synthetic weights, 128-token prompt, 128 greedy steps, 3 repetitions; for N = 1, 2, 4, 8 and the single context of
the same session: tokens/s (best repetition), graph nodes per token, and max|dlogit| against the single context on the same
history, in units of the decode tolerance 2e-3 * max|logit| + 2e-3.  Prints a markdown table (profiles/tp_rehearsal.md).
    tp_rehearse.py [--config llama-3-8b] [--mix Q4_K_M] [--prompt 128] [--steps 128] [--reps 3] [--ranks 1,2,4,8] [--out FILE]

--batched-prompt adds a second table: the same prompt through forward_batch (lgh_tp_prefill_batch, blocks of 128 tokens over the ranks)
and token by token on the same handle, ms per prompt pass (best, median and max of --reps passes), next to the single context's
lgh_prefill_batch.  The ranks run one after another on the one device, so the table shows the pass's overhead, not its scaling."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def rate(eng, prompt, steps, reps):
    """Best of `reps`: prompt token by token, then `steps` greedy tokens fed back on the device (one synchronisation at the end)."""
    best, toks = 0.0, None
    for _ in range(reps):
        eng.reset()
        for t in prompt[:-2]:
            eng.prefill_token(t)
        eng.forward(prompt[-2])            # synchronises: the prompt is done before the clock starts
        t0 = time.perf_counter()
        toks = eng.decode_greedy(prompt[-1], steps)
        best = max(best, steps / (time.perf_counter() - t0))
    return best, toks.tolist()


def prompt_ms(eng, prompt, reps, batched):
    """(best, median, max) ms of one prompt pass from position 0: forward_batch, or prefill_token one by one.  Both end synchronised
    (forward_batch of a single token is one prefill_token and a synchronisation)."""
    times = []
    for _ in range(reps + 1):               # the first pass allocates the scratch and is dropped
        eng.reset()
        eng.forward_batch(prompt[:1])
        eng.reset()
        t0 = time.perf_counter()
        if batched:
            eng.forward_batch(prompt)
        else:
            for t in prompt[:-1]:
                eng.prefill_token(t)
            eng.forward_batch(prompt[-1:])
        times.append(1e3 * (time.perf_counter() - t0))
    times = sorted(times[1:])
    return times[0], times[len(times) // 2], times[-1]


def history_logits(eng, prompt, fed):
    """Logits after the prompt and after each token of `fed` (the single context's greedy tokens: the same history for everyone)."""
    eng.reset()
    for t in prompt[:-1]:
        eng.prefill_token(t)
    out = [eng.forward(prompt[-1])]
    for t in fed:
        out.append(eng.forward(int(t)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="llama-3-8b")
    ap.add_argument("--mix", default="Q4_K_M")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ranks", default="1,2,4,8")
    ap.add_argument("--layers", type=int, default=0, help="cut the model to this many layers (a quick look)")
    ap.add_argument("--out", default="")
    ap.add_argument("--batched-prompt", action="store_true", help="also time the prompt through forward_batch against token by token")
    a = ap.parse_args()
    pkg = graft.load_package()
    max_seq = a.prompt + a.steps + 16
    over = {"num_layers": a.layers} if a.layers else {}
    cfg = pkg.make_config(a.config, max_seq_len=max_seq, **over)
    model = pkg.SynthModel(cfg, mix=a.mix, threads=16)
    for _ in model.tensors(keep=True):     # generate once, upload five times
        pass
    prompt = [(31 * i + 7) % cfg.vocab_size for i in range(a.prompt)]
    n_cmp = 8

    one = pkg.HipGpuInference.from_model(model, max_seq)
    tps1, toks1 = rate(one, prompt, a.steps, a.reps)
    ref = history_logits(one, prompt, toks1[:n_cmp])
    nodes1 = int(one.stats()["graph_nodes"])
    pf_rows = [("single context", one.prefill_is_batched(), prompt_ms(one, prompt, a.reps, True), None)] if a.batched_prompt else []
    one.close()
    rows = [("single context", tps1, nodes1, None, None)]
    print("single context: %.1f tokens/s" % tps1, file=sys.stderr, flush=True)
    for n in [int(v) for v in a.ranks.split(",")]:
        tp = pkg.HipTensorParallel.from_model(model, max_seq, n)
        tps, toks = rate(tp, prompt, a.steps, a.reps)
        got = history_logits(tp, prompt, toks1[:n_cmp])
        worst = max(float(np.abs(g - w).max()) / (2e-3 * float(np.abs(w).max()) + 2e-3) for g, w in zip(got, ref))
        same = sum(1 for x, y in zip(toks, toks1) if x == y)
        rows.append(("N = %d, all on device 0" % n, tps, tp.graph_nodes(), worst, same))
        if a.batched_prompt:
            pf_rows.append(("N = %d, all on device 0" % n, tp.prefill_is_batched(), prompt_ms(tp, prompt, a.reps, True),
                            prompt_ms(tp, prompt, min(a.reps, 2), False)))
        tp.close()
        print("N = %d: %.1f tokens/s" % (n, tps), file=sys.stderr, flush=True)
    lines = ["# Tensor-parallel rehearsal on one MI355X (tools/tp_rehearse.py)", "",
             "%s %s synthetic weights, %d-token prompt (token by token), %d greedy steps, best of %d repetitions, every rank on" %
             (a.config + (" cut to %d layers" % a.layers if a.layers else ""), a.mix, a.prompt, a.steps, a.reps),
             "device 0.  All ranks share one HBM and one stream, and the token's graph grows with N: this run shows that the structure",
             "works on a full-size model and what it costs on ONE device.  It is NOT a measurement of N GPUs and no speed claim.", "",
             "| run | tokens/s | graph nodes per token | max\\|dlogit\\| vs single context / decode tolerance | greedy tokens equal to the single context's |",
             "|---|---|---|---|---|"]
    for name, tps, nodes, worst, same in rows:
        lines.append("| %s | %.1f | %d | %s | %s |" % (name, tps, nodes, "-" if worst is None else "%.4f" % worst,
                                                     "-" if same is None else "%d / %d" % (same, a.steps)))
    if a.batched_prompt:
        lines += ["", "Prompt pass of %d tokens, ms: best (median ... max) of %d passes through forward_batch, best of %d token by token on the same" %
                  (a.prompt, a.reps, min(a.reps, 2)), "handle.  Ranks on one device run one after another: overhead, not scaling.", "",
                  "| run | batched path | forward_batch ms | token by token ms | token by token / forward_batch | forward_batch / single context |",
                  "|---|---|---|---|---|---|"]
        base = pf_rows[0][2][0]
        for name, is_b, (b, med, mx), tok in pf_rows:
            lines.append("| %s | %s | %.3f (%.3f ... %.3f) | %s | %s | %.3f |" % (
                name, "yes" if is_b else "no", b, med, mx, "-" if tok is None else "%.1f" % tok[0], "-" if tok is None else "%.1f" % (tok[0] / b), b / base))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
