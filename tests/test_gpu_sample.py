"""Sampling on the device (csrc/sample.hip; lgh_op_sample, lgh_decode_sample, lgh_decode_sample_multi) against the numpy
restatement of the reference's Sampler::sample (tests/sampler_ref.py).

The device sums the softmax as a tree where the reference sums sequentially, and its expf may differ from the host's by an
ulp, so a decision that lies within 1e-5 (relative) of a boundary — the draw against a cumulative sum, the top-p cut, a
probability tie at the top-k edge — may legitimately go either way.  Such steps are skipped (at most 1 %); every other step
must match exactly.  Where the draws are chosen by the test (teacher-forced decode) they are chosen away from the
boundaries, and the token sequences must be identical."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sampler_ref import PRESETS, Sampler, draw_unambiguous

pytestmark = pytest.mark.gpu

TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _llm_like(rng, vocab, scale=1.0, spikes=24):
    """Logits shaped like a language model's: a broad body and a few tokens far above it that carry most of the mass."""
    x = rng.normal(0.0, scale, vocab).astype(np.float32)
    k = min(spikes, vocab)
    x[rng.choice(vocab, size=k, replace=False)] += rng.uniform(6.0, 15.0, k).astype(np.float32)
    return x


def _check(hb, logits, cfg, recent=(), counts=None, r=0.5):
    s = Sampler(len(logits), **cfg)
    if counts is not None:
        s.counts[:] = counts
    want, margin, _ = s.decide(logits, list(recent), r)
    got = hb.op_sample(logits, recent=recent, counts=counts, uniform=r, **cfg)
    return want, got, margin


FLAT = dict(temperature=1.0, top_k=0, top_p=1.0, repeat_penalty=1.0, repeat_window=0)


def _crafted():
    rng = np.random.default_rng(11)
    cases = []
    ties = np.zeros(100, np.float32)
    ties[:4] = 1.0
    for r in (0.1, 0.4, 0.7, 0.95):
        cases.append((ties, dict(FLAT, top_k=3), (), None, r))               # exact ties: kept 0, 1, 2 in index order
    wide = np.zeros(300, np.float32)
    wide[10:210] = 2.0
    for r in (0.05, 0.5, 0.99):
        cases.append((wide, dict(FLAT, top_k=40), (), None, r))              # a 200-way tie across the top-k edge
    neg = rng.normal(0, 1, 500).astype(np.float32)
    neg[[0, 7, 100, 499]] = -np.inf
    for r in (0.2, 0.8):
        cases.append((neg, dict(FLAT, top_k=50, top_p=0.9), (), None, r))     # -inf entries
    top_ninf = neg.copy()
    top_ninf[:300] = -np.inf
    cases.append((top_ninf, dict(FLAT, temperature=0.7), (), None, 0.3))
    gmax = rng.normal(0, 1, 1000).astype(np.float32)
    gmax[rng.choice(1000, 100, replace=False)] = 5.0
    cases.append((gmax, dict(PRESETS["greedy"]), (), None, 0.0))              # greedy: the last of 100 maxima
    cases.append((np.array([0, 2, 2, 1], np.float32), dict(PRESETS["greedy"]), (), None, 0.0))
    p0 = np.array([10.0] + [0.0] * 9, np.float32)
    cases.append((p0, dict(FLAT, top_p=0.5), (), None, 0.99993))             # top-p cutoff at 0 keeps everything
    cases.append((np.zeros(4, np.float32), dict(FLAT, top_k=3), (), None, 1.0))   # fallback: the last kept index
    pen = np.array([2.0, -1.0, 0.0, 1.0, 1.5, -0.5, 0.7], np.float32)
    cases.append((pen, dict(temperature=0.0, top_k=1, top_p=1.0, repeat_penalty=2.0, repeat_window=0), (0, 0, 1, 2), None, 0.0))
    cases.append((pen, dict(temperature=0.9, top_k=5, top_p=0.97, repeat_penalty=1.3, repeat_window=3), (4, 0, 0, 4, 6), None, 0.6))
    cases.append((pen, dict(FLAT, frequency_penalty=0.5, presence_penalty=0.3), (), np.array([0, 3, 1, 0, 2, 0, 0]), 0.45))
    for vocab in (7, 64, 65, 1000):
        x = rng.normal(0, 1, vocab).astype(np.float32)
        cases.append((x, dict(FLAT, top_k=vocab + 5), (), None, 0.37))        # top_k >= vocab
        cases.append((x, dict(FLAT, top_k=vocab), (), None, 0.81))
    for vocab in (1000, 5000, 20000):
        x = rng.normal(0, 0.5, vocab).astype(np.float32)
        for r in (0.13, 0.5, 0.9):
            cases.append((x, dict(FLAT), (), None, r))                       # a draw over the whole vocabulary (band walk)
        cases.append((x, dict(FLAT, top_k=300, top_p=0.7), (), None, 0.77))   # top_k > 64
    for vocab in (32000, 128256):                                            # confident steps: p0 > top_p keeps everything
        x = rng.normal(0, 1, vocab).astype(np.float32)
        x[123] += 18.0
        for r in (0.3, 0.99, 0.9995):
            cases.append((x, dict(PRESETS["creative"]), (), None, r))
            cases.append((x, dict(FLAT), (), None, r))
            cases.append((x, dict(FLAT, temperature=0.05, top_p=0.9), (), None, r))   # the tail vanishes below half an ulp
    eq = np.zeros(10000, np.float32)                                         # one tie group larger than a band
    for r in (0.0, 0.5, 0.99995):
        cases.append((eq, dict(FLAT), (), None, r))
        cases.append((eq, dict(FLAT, top_p=0.5), (), None, r))
    return cases


def test_op_sample_crafted_vectors(gpu):
    checked = 0
    for i, (logits, cfg, recent, counts, r) in enumerate(_crafted()):
        want, got, margin = _check(gpu, logits, cfg, recent, counts, r)
        if margin <= TOL and want != got:
            continue
        assert got == want, (i, cfg, r, got, want, margin)
        checked += 1
    assert checked >= len(_crafted()) - 2


@pytest.mark.parametrize("vocab", [7, 1000, 32000, 128256, 151936])
def test_op_sample_random_vectors(gpu, vocab):
    rng = np.random.default_rng(vocab)
    configs = [PRESETS["engine_default"], PRESETS["server"], PRESETS["creative"], PRESETS["greedy"]]
    n, skipped = 0, 0
    for cfg in configs:
        for trial in range(25 if vocab < 100000 else 13):
            logits = _llm_like(rng, vocab, spikes=min(24, max(1, vocab // 4)))
            recent = rng.integers(0, vocab, size=int(rng.integers(0, 100))).tolist()
            counts = rng.integers(0, 3, size=vocab) * (rng.random(vocab) < 0.01) if cfg is PRESETS["server"] else None
            r = float(rng.random(dtype=np.float32))
            want, got, margin = _check(gpu, logits, cfg, recent, counts, r)
            n += 1
            if margin <= TOL:
                skipped += 1
                continue
            assert got == want, (cfg, trial, r, got, want, margin)
    assert skipped <= max(1, n // 100), (skipped, n)


def test_bad_configs_are_invalid_arguments(gpu):
    x = np.zeros(16, np.float32)
    for bad in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_p=0.0),
                dict(top_p=1.5), dict(repeat_penalty=0.0), dict(repeat_penalty=-1.0)):
        with pytest.raises(gpu.BackendError) as ei:
            gpu.op_sample(x, **bad)
        assert ei.value.status == 6


# ---- decode: the sampler inside the per-token graph
def _model(pkg, name, mix="Q4_K_M", max_seq=96, **kw):
    cfg = pkg.make_config(name, max_seq_len=max_seq, **kw)
    return cfg, pkg.SynthModel(cfg, mix=mix)


def _teacher_forced(ref_engine, cfg_s, prompt, n_steps, rng):
    """Tokens and the draws that give them: ref_engine's lgh_forward logits, the restatement's decisions with every draw away
    from the boundaries; and how many leading steps are settled (a step whose top-p cut, top-k edge or greedy choice lies
    within TOL of a boundary may go either way whatever the draw: the comparison ends before it).  After the step that samples
    cfg_s["eos_token"] the counts stay as they are (the library's contract for the steps the reference never takes)."""
    s = Sampler(ref_engine.vocab_size, **cfg_s)
    ref_engine.reset()
    ref_engine.forward_batch(prompt[:-1])
    ctx = list(prompt)
    tok, toks, unis, n_settled, eos_seen = prompt[-1], [], [], None, False
    for i in range(n_steps):
        logits = ref_engine.forward(tok)
        frozen = s.counts.copy()
        r, tok, settled = draw_unambiguous(s, logits, ctx, rng, tol=TOL)
        if eos_seen:
            s.counts[:] = frozen
        eos_seen = eos_seen or tok == cfg_s.get("eos_token", -1)
        if not settled and n_settled is None:
            n_settled = i
        unis.append(r)
        toks.append(tok)
        ctx.append(tok)
    return np.array(toks, np.uint32), np.array(unis, np.float32), n_steps if n_settled is None else n_settled


@pytest.mark.parametrize("name", ["test-dense", "test-dense-d128", "test-moe"])
def test_decode_sample_matches_the_restatement_teacher_forced(pkg, gpu, name):
    cfg, model = _model(pkg, name)
    ref = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    rng = np.random.default_rng(7)
    prompt = [int(t) for t in rng.integers(0, cfg.vocab_size, size=6)]
    compared = 0
    for preset in ("engine_default", "server", "creative", "greedy"):
        want, unis, n = _teacher_forced(ref, PRESETS[preset], prompt, 20, rng)
        eng.reset()
        eng.forward_batch(prompt[:-1])
        eng.set_sampler(**PRESETS[preset])
        got = eng.decode_sample(prompt[-1], prompt[:-1], 20, unis)
        assert got[:n].tolist() == want[:n].tolist(), (name, preset, n)
        compared += n
    assert compared >= 60, compared


def test_window_and_eos_follow_the_restatement(pkg, gpu):
    """A repetition window of 4 (tokens leave it from the history and then from the call's own tokens) and an EOS token the
    restatement samples early (the counts freeze after it), each against the restatement."""
    cfg, model = _model(pkg, "test-dense")
    ref = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    prompt = [int(t) for t in np.random.default_rng(9).integers(0, cfg.vocab_size, size=6)] + [77, 77]
    windowed = dict(PRESETS["server"], repeat_penalty=1.8, repeat_window=4)
    base = _teacher_forced(ref, windowed, prompt, 24, np.random.default_rng(21))[0]
    eos = int(base[2])                                    # sampled at step 2 (or earlier) with the same draws
    for conf in (windowed, dict(windowed, eos_token=eos)):
        want, unis, n = _teacher_forced(ref, conf, prompt, 24, np.random.default_rng(21))
        eng.reset()
        eng.forward_batch(prompt[:-1])
        eng.set_sampler(**conf)
        got = eng.decode_sample(prompt[-1], prompt[:-1], 24, unis)
        assert n >= 12, n
        assert got[:n].tolist() == want[:n].tolist(), (conf, n)
    assert eos in want[:3].tolist()


def test_decode_sample_full_llama3_vocabulary(pkg, gpu):
    """The full 128 256-token vocabulary.  (`creative` is covered on the small models: the synthetic model's logits are so flat
    that over this vocabulary its top-p cut lies within TOL of a boundary at every step.)"""
    cfg, model = _model(pkg, "llama-3-8b", max_seq=40, num_layers=2)
    ref = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    rng = np.random.default_rng(8)
    prompt = [int(t) for t in rng.integers(0, cfg.vocab_size, size=5)]
    for preset in ("engine_default", "server", "greedy"):
        want, unis, n = _teacher_forced(ref, PRESETS[preset], prompt, 8, rng)
        eng.reset()
        eng.forward_batch(prompt[:-1])
        eng.set_sampler(**PRESETS[preset])
        assert eng.decode_sample(prompt[-1], prompt[:-1], 8, unis)[:n].tolist() == want[:n].tolist(), (preset, n)
        assert n >= 4, n


def test_greedy_config_equals_decode_greedy_and_runs_are_bitwise_repeatable(pkg, gpu):
    cfg, model = _model(pkg, "test-dense")
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    prompt = [5, 99, 310, 7]
    eng.forward_batch(prompt[:-1])
    greedy = eng.decode_greedy(prompt[-1], 24)
    eng.reset()
    eng.forward_batch(prompt[:-1])
    eng.set_sampler(temperature=0.0, top_k=40, top_p=0.95, repeat_penalty=1.0)
    assert eng.decode_sample(prompt[-1], prompt[:-1], 24, None).tolist() == greedy.tolist()
    runs = []
    unis = np.random.default_rng(1).random(24, dtype=np.float32)
    for _ in range(2):
        eng.reset()
        eng.forward_batch(prompt[:-1])
        eng.set_sampler(**PRESETS["server"])
        runs.append(eng.decode_sample(prompt[-1], prompt[:-1], 24, unis))
    assert runs[0].tolist() == runs[1].tolist()


def test_one_call_equals_three_calls_with_counts_persisting(pkg, gpu):
    cfg, model = _model(pkg, "test-dense")
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    prompt = [17, 3, 900, 41, 41]
    unis = np.random.default_rng(2).random(24, dtype=np.float32)
    conf = dict(PRESETS["server"], repeat_window=6)   # a window short enough that tokens leave it inside and across calls
    eng.forward_batch(prompt[:-1])
    eng.set_sampler(**conf)
    one = eng.decode_sample(prompt[-1], prompt[:-1], 24, unis)
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
    assert three == one.tolist()


def test_sampling_without_set_sampler_is_an_invalid_argument(pkg, gpu):
    cfg, model = _model(pkg, "test-dense")
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    with pytest.raises(pkg.BackendError) as ei:
        eng.decode_sample(1, [], 4, np.zeros(4, np.float32))
    assert ei.value.status == 6
    with pytest.raises(pkg.BackendError):
        eng.set_sampler(top_p=0.0)


# ---- multi-sequence
def _slot_cfg(s):
    return [dict(PRESETS["engine_default"]), dict(PRESETS["server"]), dict(PRESETS["creative"]),
            dict(PRESETS["greedy"]), dict(PRESETS["engine_default"], repeat_window=5, eos_token=3)][s % 5]


def _multi_case(pkg, name, B, n_steps=12, seed=0):
    """(tokens of lgh_decode_sample_multi [n_steps, B], the same sequences one by one through lgh_decode_sample)."""
    cfg, model = _model(pkg, name, max_seq=64)
    multi = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    single = pkg.HipGpuInference.from_model(model, cfg.max_seq_len, attn_direct=255)
    multi.batch_create(B)
    rng = np.random.default_rng(100 + B + seed)
    hists, firsts = [], []
    for s in range(B):
        # ragged positions; prompts of >= 2 tokens, so that both engines take the batched prompt path
        h = [int(t) for t in rng.integers(0, cfg.vocab_size, size=3 + (7 * s) % 13)]
        multi.batch_reset(s)
        multi.batch_prefill(s, h[:-1])
        multi.batch_set_sampler(s, **_slot_cfg(s))
        hists.append(h[:-1])
        firsts.append(h[-1])
    unis = rng.random((n_steps, B), dtype=np.float32)
    got = multi.decode_sample_multi(list(range(B)), firsts, hists, n_steps, unis)
    want = np.zeros_like(got)
    for s in range(B):
        single.reset()
        single.forward_batch(hists[s])
        single.set_sampler(**_slot_cfg(s))
        want[:, s] = single.decode_sample(firsts[s], hists[s], n_steps, unis[:, s])
    return got, want


@pytest.mark.parametrize("name,B", [("test-dense", 1), ("test-dense", 3), ("test-dense", 5), ("test-dense", 8), ("test-dense", 16),
                                    ("test-moe", 3), ("test-moe", 8), ("test-moe", 16)])
def test_decode_sample_multi_equals_single_sequence(pkg, gpu, name, B):
    got, want = _multi_case(pkg, name, B)
    assert got.tolist() == want.tolist()


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as graft
from test_gpu_sample import _multi_case
pkg = graft.load_package()
out = {}
for name, B in (("test-dense", 16), ("test-moe", 3)):
    got, _ = _multi_case(pkg, name, B, seed=1)
    out[name] = got.tolist()
from test_gpu_sample import _single_case
out["single"] = _single_case(pkg).tolist()
print(json.dumps(out))
"""


def _single_case(pkg):
    cfg, model = _model(pkg, "test-dense-d128", max_seq=48)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    prompt = [11, 500, 1999, 64, 8]
    eng.forward_batch(prompt[:-1])
    eng.set_sampler(**PRESETS["engine_default"])
    return eng.decode_sample(prompt[-1], prompt[:-1], 16, np.random.default_rng(4).random(16, dtype=np.float32))


def test_fresh_process_first_gpu_work_is_sampling(pkg, gpu):
    """A kernel first launched inside a capture is not replayed (engine.hip warm_kernels): a child whose FIRST GPU work is a
    multi-sequence and a single-sequence sampled decode must get the parent's tokens."""
    want = {}
    for name, B in (("test-dense", 16), ("test-moe", 3)):
        want[name] = _multi_case(pkg, name, B, seed=1)[0].tolist()
    want["single"] = _single_case(pkg).tolist()
    res = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got == want
