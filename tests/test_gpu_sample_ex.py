"""min-p and Mirostat v1 / v2 on the device (csrc/sample.hip; lgh_op_sample_ex, lgh_set_sampler_ex, lgh_batch_set_sampler_ex,
lgh_get_sampler_mu) against the numpy restatement (tests/sampler_ref_ex.py).

As in test_gpu_sample.py, a decision within 1e-5 of a boundary may legitimately go either way (outside Mirostat the device sums
the softmax as a tree; under Mirostat it sums in the reference's order, but its expf / log2f may still differ from the host's by
an ulp): such a case is left out.  At most 10 % of the random cases of a
parametrization may be, and none of the crafted ones; that the restatement alone stays within this on the chosen seeds is
checked without the device's answers.  mu is compared with the float64 recurrence over the restatement's f32 selected
probabilities: the device's value and the f32 restatement's must both lie within sampler_ref_ex.mu_bound of it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sampler_ref_ex import PRESETS_EX, SamplerEx, draw_unambiguous_ex, mu_bound

pytestmark = pytest.mark.gpu

TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT = dict(temperature=1.0, top_k=0, top_p=1.0, repeat_penalty=1.0, repeat_window=0)
V1 = dict(FLAT, mirostat=1, tau=3.0, eta=0.2)
V2 = dict(PRESETS_EX["mirostat_v2"])
VOCABS = (7, 64, 65, 1000, 5000, 32000)   # 65: one past the candidates; 5000: two bands of the walk


def _llm_like(rng, vocab, scale=1.0, spikes=24):
    x = rng.normal(0.0, scale, vocab).astype(np.float32)
    k = min(spikes, vocab)
    x[rng.choice(vocab, size=k, replace=False)] += rng.uniform(6.0, 15.0, k).astype(np.float32)
    return x


# ---- the inputs (also what tests/test_sampler_ref_ex.py plants its mutants on)
def random_cases(vocab):
    """[(logits, cfg, recent, counts, r, mu_in)]: spiked and flat logits under creative_ref, min_p 0.01 / 0.5 / 1.0 with and
    without top_k 40, Mirostat v2 from mu 0 / 3 / 10 / 20 and v1, each bare and with a window, counts and penalties."""
    rng = np.random.default_rng(1000 + vocab)
    configs = [(dict(PRESETS_EX["creative_ref"]), None)]
    for mp in (0.01, 0.5, 1.0):
        for tk in (0, 40):
            configs.append((dict(FLAT, min_p=mp, top_k=tk, top_p=0.95 if tk else 1.0), None))
    configs += [(dict(V2), mu) for mu in (0.0, 3.0, 10.0, 20.0)] + [(dict(V1), 6.0)]
    cases = []
    for cfg, mu in configs:
        for kind in ("spiked", "flat"):
            for pen in (False, True):
                for _ in range(2):
                    x = _llm_like(rng, vocab, spikes=min(24, max(1, vocab // 4))) if kind == "spiked" else \
                        rng.normal(0.0, 0.5, vocab).astype(np.float32)
                    c, recent, counts = dict(cfg), (), None
                    if pen:
                        c.update(repeat_penalty=1.3, repeat_window=32, frequency_penalty=0.4, presence_penalty=0.2)
                        recent = tuple(int(t) for t in np.concatenate([rng.integers(0, vocab, 40), np.argsort(-x)[:3]]))
                        counts = (rng.integers(1, 4, vocab) * (rng.random(vocab) < 0.05)).astype(np.int64)
                        counts[np.argmax(x)] = 2
                    cases.append((x, c, recent, counts, float(rng.random(dtype=np.float32)), mu))
    return cases


def _confident():
    """p = 0.9026, 0.0497, 0.0472 and a body of 997 x 2.8e-7: the top token alone is above top_p 0.9, and min_p 0.05 keeps three."""
    x = np.full(1000, -3.0, np.float32)
    x[[5, 600, 77]] = (12.0, 9.1, 9.05)
    return x


def crafted_cases():
    cases = []
    for n_high in (63, 64, 65):                      # a min-p cut exactly at / next to the last candidate
        x = np.zeros(200, np.float32)
        x[20:20 + n_high] = 5.0 - 0.001 * np.arange(n_high, dtype=np.float32)
        for r in (0.02, 0.5, 0.97, 0.9999):
            cases.append((x, dict(FLAT, min_p=0.5), (), None, r, None))
        cases.append((x, dict(FLAT, min_p=0.5, top_k=70, top_p=0.9), (), None, 0.93, None))
    tie = np.full(400, -2.0, np.float32)             # a tie group of 100 right at the threshold: kept whole or dropped whole
    tie[7] = 3.0
    tie[50:150] = 2.0                                # p / p0 = exp(-1) = 0.3679
    for mp in (0.36, 0.37):
        for r in (0.1, 0.45, 0.9, 0.999):
            cases.append((tie, dict(FLAT, min_p=mp), (), None, r, None))
        cases.append((tie, dict(FLAT, min_p=mp, top_k=30), (), None, 0.8, None))
    conf = _confident()                              # top-p cutoff 0 keeps the min-p set (3 tokens), not the vocabulary
    for r in (0.5, 0.93, 0.99, 0.9999):
        cases.append((conf, dict(FLAT, min_p=0.05, top_p=0.9), (), None, r, None))
    cases.append((conf, dict(FLAT, min_p=0.05, top_k=2), (), None, 0.999, None))   # top-k against the min-p length: 2 < 3
    cases.append((conf, dict(FLAT, min_p=0.05, top_k=5), (), None, 0.9999, None))  # ... and 5 > 3: the min-p set
    cases.append((conf, dict(FLAT, min_p=0.05, temperature=0.0), (), None, 0.7, None))   # greedy ignores min_p
    two = np.log(np.array([0.6, 0.3, 0.06, 0.04], np.float32)).astype(np.float32)   # surprises 0.74, 1.74, 4.06, 4.64
    for mu in (0.5, 1.0, 2.0, 4.5):                  # v2: rank 0 exceeds (max(rank, 1)), rank 1, rank 2, none
        for r in (0.3, 0.65, 0.95):
            cases.append((two, dict(V2), (), None, r, mu))
    far = np.full(1000, -5.0, np.float32)            # v2 truncation beyond the candidates: 100 tokens around 2^-7, the rest 2^-21
    far[300:400] = 5.0 - 0.01 * np.arange(100, dtype=np.float32)
    for r in (0.1, 0.5, 0.95):
        cases.append((far, dict(V2), (), None, r, 10.0))
        cases.append((far, dict(V1), (), None, r, 6.0))
    for x in (two, far, conf):                       # a draw that no cumulative sum exceeds: the TOP token, not the last
        cases.append((x, dict(V2), (), None, 1.001, 10.0))
        cases.append((x, dict(V1), (), None, 1.001, 6.0))
    cases.append((conf, dict(V2, temperature=0.0, top_k=1, top_p=0.5, min_p=0.9), (), None, 0.9999, 20.0))   # all ignored
    cases.append((two, dict(V2, repeat_penalty=2.0, frequency_penalty=0.5), (0, 0), np.array([1, 0, 2, 0]), 0.4, 3.0))
    return cases


def reference(case, mutant=None):
    """(token, margin, mu after in f32, mu after in f64, surprise) of the restatement."""
    x, cfg, recent, counts, r, mu = case
    s = SamplerEx(len(x), mutant=mutant, **cfg)
    if counts is not None:
        s.counts[:] = counts
    if mu is not None:
        s.mu, s.mu64 = np.float32(mu), float(mu)
    tok, margin, counted = s.decide(x, list(recent), r)
    s.commit(tok, counted)
    return tok, margin, float(s.mu), s.mu64, s.s_max


def _device(hb, case):
    x, cfg, recent, counts, r, mu = case
    got = hb.op_sample(x, recent=recent, counts=counts, uniform=r, mu=mu, **cfg)
    return got if isinstance(got, tuple) else (got, None)


_RESULTS = {}


def _results(hb, key, cases):
    """[(reference(case), device token, device mu)] of the cases that are compared; how many were left out.  Computed once."""
    if key not in _RESULTS:
        rows, left_out = [], 0
        for i, case in enumerate(cases):
            ref = reference(case)
            if ref[1] <= TOL:
                left_out += 1
                continue
            rows.append((i, case, ref) + _device(hb, case))
        _RESULTS[key] = rows, left_out
    return _RESULTS[key]


def _tokens_match(hb, key, cases, allowed):
    rows, left_out = _results(hb, key, cases)
    for i, case, (want, margin, *_), tok, mu in rows:
        assert tok == want, (i, case[1], case[4], case[5], tok, want, margin)
        assert (mu is not None) == bool(case[1].get("mirostat"))
    assert left_out <= allowed, (left_out, len(cases))


def _mu_within_bound(hb, key, cases):
    rows, _ = _results(hb, key, cases)
    worst = (0.0, None)
    for i, case, (_, _, mu32, mu64, s), tok, mu in rows:
        if case[1].get("mirostat"):
            bound = mu_bound(1, case[1]["eta"], s)
            worst = max(worst, (max(abs(mu - mu64), abs(mu32 - mu64)) / bound, (i, mu, mu32, mu64, bound)), key=lambda w: w[0])
    print(f"mu {key}: worst |mu - mu64| / bound = {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize("vocab", VOCABS)
def test_op_sample_ex_random_vectors(gpu, vocab):
    cases = random_cases(vocab)
    assert sum(reference(c)[1] <= TOL for c in cases) <= len(cases) // 10   # the restatement alone, whatever the device says
    _tokens_match(gpu, vocab, cases, len(cases) // 10)


@pytest.mark.parametrize("vocab", VOCABS)
def test_op_sample_ex_random_vectors_mu(gpu, vocab):
    """mu after one step, device and f32 restatement, within |eta| * 4 * ulp32(s) + ulp32(20) of the float64 recurrence.

    The bound allows for log2f and one rounding of mu only, so it also pins the softmax denominator: the reference sums
    exp(x - max) sequentially in f32, which on spiked logits is 2.2e-5 (vocabulary 5000) to 1.5e-4 (32000) relative away from
    the exact sum, 3 to 21 times this bound in mu.  Under Mirostat the device therefore sums in the reference's order (sample.hip,
    samp_merge); an accurate tree sum there fails this test at 5000 and 32000."""
    _mu_within_bound(gpu, vocab, random_cases(vocab))


def test_op_sample_ex_crafted_vectors(gpu):
    _tokens_match(gpu, "crafted", crafted_cases(), 0)


def test_op_sample_ex_crafted_vectors_mu(gpu):
    """As test_op_sample_ex_random_vectors_mu; the v1 draw over `far` (100 tokens of weight ~1, 900 of weight 4.5e-5) is the
    case here whose sequential f32 softmax sum is furthest (4.6e-5) from the exact one."""
    _mu_within_bound(gpu, "crafted", crafted_cases())


def test_creative_ref_is_not_creative(gpu):
    """On a confident step min-p keeps a handful of tokens where the min-p-less `creative` keeps the vocabulary (top-p's cutoff-0
    quirk): a draw deep in the tail tells them apart, through the old entry point too (which must refuse nothing and drop
    nothing: the keyword routes to the _ex one)."""
    x = _confident()
    with_min_p = gpu.op_sample(x, uniform=0.99999, **gpu.SAMPLER_PRESETS["creative_ref"])
    without = gpu.op_sample(x, uniform=0.99999, **gpu.SAMPLER_PRESETS["creative"])
    assert with_min_p == 77 and without > 77
    assert gpu.SAMPLER_PRESETS["creative_ref"] == PRESETS_EX["creative_ref"] and gpu.SAMPLER_PRESETS["mirostat_v2"] == PRESETS_EX["mirostat_v2"]


def trajectory(cfg, draws=None, mutant=None):
    """24 steps of one sampler over fresh logits (every third flat): yields (logits, recent, counts before, r, token, sampler
    after the step).  draws: the uniforms to use (default: chosen away from the boundaries, and every step must be settled)."""
    rng, rng_draws = np.random.default_rng(31), np.random.default_rng(32)
    s = SamplerEx(1000, mutant=mutant, **cfg)
    recent = []
    for step in range(24):
        x = _llm_like(rng, 1000, scale=1.5, spikes=6) if step % 3 else rng.normal(0, 0.5, 1000).astype(np.float32)
        counts, before = s.counts.copy(), list(recent)
        if draws is None:
            r, tok, settled = draw_unambiguous_ex(s, x, recent, rng_draws, tol=TOL)
            assert settled, step
        else:
            r, tok = draws[step], s.sample(x, recent, draws[step])
        recent.append(tok)
        yield x, before, counts, r, tok, s


TRAJECTORIES = [V2, V1, dict(V2, tau=6.0, repeat_penalty=1.2, repeat_window=8, frequency_penalty=0.3)]


@pytest.mark.parametrize("cfg", TRAJECTORIES, ids=["v2", "v1", "v2-tau6"])
def test_op_sample_ex_mu_trajectory(gpu, cfg):
    """24 steps, the device carrying its own mu from call to call: tokens as the restatement's, and both f32 values of mu within
    steps * (|eta| * 4 * ulp32(s_max) + ulp32(20)) of the float64 recurrence."""
    mu, worst = None, (0.0, None)   # (the first call starts from 2 * tau, as Sampler::new does)
    for step, (x, recent, counts, r, want, s) in enumerate(trajectory(cfg)):
        tok, mu = gpu.op_sample(x, recent=recent, counts=counts, uniform=r, mu=mu, **cfg)
        assert tok == want, (step, tok, want)
        worst = max(worst, (max(abs(mu - s.mu64), abs(float(s.mu) - s.mu64)) / s.bound(), (step, mu, float(s.mu), s.mu64, s.bound())),
                    key=lambda w: w[0])
    print(f"mu trajectory: worst |mu - mu64| / bound = {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst
    assert s.mu_steps == 24 and s.counts.sum() == 24   # Mirostat always counts


def test_bad_ex_configs_are_invalid_arguments(pkg, gpu):
    x = np.zeros(16, np.float32)
    nan, inf = float("nan"), float("inf")
    bad = (dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=nan), dict(min_p=inf), dict(mirostat=3), dict(mirostat=2, tau=-1.0),
           dict(mirostat=2, tau=nan), dict(mirostat=1, eta=inf), dict(mirostat=0, tau=inf), dict(min_p=0.1, top_p=0.0))
    for cfg in bad:
        with pytest.raises(gpu.BackendError) as ei:
            gpu.op_sample(x, **cfg)
        assert ei.value.status == 6, cfg
    with pytest.raises(gpu.BackendError) as ei:
        gpu.op_sample(x, mu=21.0, **V2)
    assert ei.value.status == 6
    conf, model = _model(pkg, "test-dense")
    eng = pkg.HipGpuInference.from_model(model, conf.max_seq_len)
    eng.batch_create(2)
    for cfg in bad:
        with pytest.raises(pkg.BackendError) as ei:
            eng.set_sampler(**cfg)
        assert ei.value.status == 6, cfg
        with pytest.raises(pkg.BackendError) as ei:
            eng.batch_set_sampler(1, **cfg)
        assert ei.value.status == 6, cfg
    wrong = gpu.sampler_config_ex(**V2)
    wrong.struct_size -= 4
    lib = gpu.load_library()
    import ctypes as C
    assert lib.lgh_set_sampler_ex(eng._h, C.byref(wrong)) == 6
    assert lib.lgh_batch_set_sampler_ex(eng._h, 0, C.byref(wrong)) == 6
    with pytest.raises(pkg.BackendError):
        eng.sampler_mu()          # no sampler yet
    with pytest.raises(pkg.BackendError):
        eng.sampler_mu(1)


# ---- decode: the sampler inside the per-token graph
def _model(pkg, name, mix="Q4_K_M", max_seq=96, **kw):
    cfg = pkg.make_config(name, max_seq_len=max_seq, **kw)
    return cfg, pkg.SynthModel(cfg, mix=mix)


DECODE_CONFIGS = {
    "creative_ref": dict(PRESETS_EX["creative_ref"]),
    "v2": dict(V2),
    "v2-tau8": dict(V2, tau=8.0, repeat_penalty=1.2, repeat_window=8, frequency_penalty=0.3, presence_penalty=0.1),
    "v1": dict(V1, repeat_penalty=1.1, repeat_window=16, frequency_penalty=0.2),
}


def _teacher_forced(ref_engine, cfg_s, prompt, n_steps, rng):
    """test_gpu_sample._teacher_forced with a SamplerEx: (tokens, draws, settled leading steps, the sampler after the steps).
    After the step that samples cfg_s["eos_token"] neither the counts nor mu move.  The sampler's `settled_mu` is (f32 mu, f64
    mu, bound) as they stood after the settled leading steps."""
    s = SamplerEx(ref_engine.vocab_size, **cfg_s)
    s.settled_mu = (float(s.mu), s.mu64, 0.0)
    ref_engine.reset()
    ref_engine.forward_batch(prompt[:-1])
    ctx = list(prompt)
    tok, toks, unis, n_settled, eos_seen = prompt[-1], [], [], None, False
    for i in range(n_steps):
        logits = ref_engine.forward(tok)
        r, tok, settled = draw_unambiguous_ex(s, logits, ctx, rng, tol=TOL, frozen=eos_seen)
        eos_seen = eos_seen or tok == cfg_s.get("eos_token", -1)
        if not settled and n_settled is None:
            n_settled = i
        if n_settled is None:
            s.settled_mu = (float(s.mu), s.mu64, s.bound())
        unis.append(r)
        toks.append(tok)
        ctx.append(tok)
    return np.array(toks, np.uint32), np.array(unis, np.float32), n_steps if n_settled is None else n_settled, s


def _mu_ok(eng, s, slot=-1):
    """The device's mu against the restatement's after its settled leading steps (all of them, where every step settled)."""
    mu = eng.sampler_mu(slot)
    mu32, mu64, bound = s.settled_mu
    assert abs(mu - mu64) <= bound and abs(mu32 - mu64) <= bound, (mu, mu32, mu64, bound)


@pytest.mark.parametrize("name", ["test-dense", "test-moe"])
def test_decode_sample_ex_matches_the_restatement_teacher_forced(pkg, gpu, name):
    cfg, model = _model(pkg, name)
    ref = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    rng = np.random.default_rng(17)
    prompt = [int(t) for t in rng.integers(0, cfg.vocab_size, size=6)]
    mu_checked = 0
    for key, conf in DECODE_CONFIGS.items():
        want, unis, n, s = _teacher_forced(ref, conf, prompt, 24, rng)
        assert n >= 12, (key, n)
        eng.reset()
        eng.forward_batch(prompt[:-1])
        eng.set_sampler(**conf)
        if conf.get("mirostat"):
            assert eng.sampler_mu() == np.float32(2.0) * np.float32(conf["tau"])   # Sampler::new
        one = eng.decode_sample(prompt[-1], prompt[:-1], 24, unis)
        assert one[:n].tolist() == want[:n].tolist(), (name, key, n)
        mu_one = eng.sampler_mu()
        if conf.get("mirostat"):   # mu after the call, or, where a later step is unsettled, after a call of the n settled ones
            if n < 24:
                eng.reset()
                eng.forward_batch(prompt[:-1])
                eng.set_sampler(**conf)
                assert eng.decode_sample(prompt[-1], prompt[:-1], n, unis[:n]).tolist() == want[:n].tolist()
            _mu_ok(eng, s)
            mu_checked += 1
        # the same steps as three calls of 8: mu and the counts persist; set_sampler restarts both
        eng.reset()
        eng.forward_batch(prompt[:-1])
        eng.set_sampler(**conf)
        ctx, tok, three = list(prompt[:-1]), prompt[-1], []
        for c in range(3):
            got = eng.decode_sample(tok, ctx, 8, unis[8 * c:8 * c + 8])
            ctx.append(tok)
            ctx += got[:-1].tolist()
            tok = int(got[-1])
            three += got.tolist()
        assert three == one.tolist(), (name, key)
        assert eng.sampler_mu() == mu_one
        eng.set_sampler(**conf)
        assert eng.sampler_mu() == (np.float32(2.0) * np.float32(conf["tau"]) if conf.get("mirostat") else 10.0)
    assert mu_checked == 3, mu_checked   # v2, v2-tau8 and v1


def test_eos_mid_call_freezes_the_counts_and_mu(pkg, gpu):
    cfg, model = _model(pkg, "test-dense")
    ref = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    prompt = [int(t) for t in np.random.default_rng(9).integers(0, cfg.vocab_size, size=6)]
    conf = dict(DECODE_CONFIGS["v2-tau8"])
    base, _, _, s_free = _teacher_forced(ref, conf, prompt, 16, np.random.default_rng(21))
    conf["eos_token"] = int(base[3])                      # sampled at step 3 (or earlier) with the same draws
    want, unis, n, s = _teacher_forced(ref, conf, prompt, 16, np.random.default_rng(21))
    assert n == 16 and conf["eos_token"] in want[:4].tolist()
    eos_at = want.tolist().index(conf["eos_token"])
    assert s.mu_steps == eos_at + 1 and s.counts.sum() == eos_at + 1
    eng.forward_batch(prompt[:-1])
    eng.set_sampler(**conf)
    got = eng.decode_sample(prompt[-1], prompt[:-1], 16, unis)
    assert got.tolist() == want.tolist()                  # (frozen counts: the later steps' penalties say so)
    _mu_ok(eng, s)                                        # mu as after the eos step, 12 steps earlier
    assert abs(s_free.mu64 - s.mu64) > s_free.bound()     # (which the unfrozen recurrence leaves)


def test_set_sampler_equals_set_sampler_ex_with_nothing_added_and_runs_repeat(pkg, gpu):
    cfg, model = _model(pkg, "test-dense")
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    prompt = [5, 99, 310, 7]
    unis = np.random.default_rng(1).random(24, dtype=np.float32)
    runs = {}
    for key, conf in (("old", dict(PRESETS_EX["server"])), ("ex", dict(PRESETS_EX["server"], min_p=0.0, mirostat=0)),
                      ("v2", dict(V2)), ("v2 again", dict(V2)), ("creative_ref", dict(PRESETS_EX["creative_ref"])),
                      ("creative_ref again", dict(PRESETS_EX["creative_ref"]))):
        eng.reset()
        eng.forward_batch(prompt[:-1])
        eng.set_sampler(**conf)
        runs[key] = (eng.decode_sample(prompt[-1], prompt[:-1], 24, unis).tolist(), eng.sampler_mu())
    assert runs["old"] == runs["ex"]
    assert runs["v2"] == runs["v2 again"] and runs["creative_ref"] == runs["creative_ref again"]
    assert runs["old"][1] == 10.0 and runs["v2"][1] != 10.0


# ---- multi-sequence: slots mix ordinary and Mirostat samplers
def _slot_cfg(s):
    return [dict(PRESETS_EX["engine_default"]), dict(PRESETS_EX["creative_ref"]), dict(PRESETS_EX["mirostat_v2"])][s % 3]


def _multi_case(pkg, name, B, n_steps=12, seed=0):
    """(tokens [n_steps, B] and mu per slot of lgh_decode_sample_multi, the same one by one through lgh_decode_sample)."""
    cfg, model = _model(pkg, name, max_seq=64)
    multi = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    single = pkg.HipGpuInference.from_model(model, cfg.max_seq_len, attn_direct=255)
    multi.batch_create(B)
    rng = np.random.default_rng(300 + B + seed)
    hists, firsts = [], []
    for s in range(B):
        h = [int(t) for t in rng.integers(0, cfg.vocab_size, size=3 + (7 * s) % 13)]
        multi.batch_reset(s)
        multi.batch_prefill(s, h[:-1])
        multi.batch_set_sampler(s, **_slot_cfg(s))
        hists.append(h[:-1])
        firsts.append(h[-1])
    unis = rng.random((n_steps, B), dtype=np.float32)
    got = multi.decode_sample_multi(list(range(B)), firsts, hists, n_steps, unis)
    got_mu = [multi.sampler_mu(s) for s in range(B)]
    want, want_mu = np.zeros_like(got), []
    for s in range(B):
        single.reset()
        single.forward_batch(hists[s])
        single.set_sampler(**_slot_cfg(s))
        want[:, s] = single.decode_sample(firsts[s], hists[s], n_steps, unis[:, s])
        want_mu.append(single.sampler_mu())
    return got, got_mu, want, want_mu


@pytest.mark.parametrize("name,B", [("test-dense", 3), ("test-dense", 8), ("test-moe", 3)])
def test_decode_sample_multi_ex_equals_single_sequence(pkg, gpu, name, B):
    got, got_mu, want, want_mu = _multi_case(pkg, name, B)
    assert got.tolist() == want.tolist()
    assert got_mu == want_mu
    assert got_mu[0] == 10.0 and got_mu[1] == 10.0 and got_mu[2] != 10.0


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as graft
from test_gpu_sample_ex import _single_case
print(json.dumps(_single_case(graft.load_package())))
"""


def _single_case(pkg):
    cfg, model = _model(pkg, "test-dense", max_seq=48)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    prompt = [11, 500, 999, 64, 8]
    eng.forward_batch(prompt[:-1])
    eng.set_sampler(**V2)
    toks = eng.decode_sample(prompt[-1], prompt[:-1], 16, np.random.default_rng(4).random(16, dtype=np.float32))
    return [toks.tolist(), eng.sampler_mu()]


def test_fresh_process_first_gpu_work_is_a_mirostat_decode(pkg, gpu):
    """A kernel first launched inside a capture is not replayed (engine.hip warm_kernels): a child whose FIRST GPU work is a
    Mirostat decode must get the parent's tokens and mu."""
    want = _single_case(pkg)
    res = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads(res.stdout.strip().splitlines()[-1]) == want
