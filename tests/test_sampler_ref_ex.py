"""The restatement of min-p and Mirostat (tests/sampler_ref_ex.py) — the arbiter of the device sampler's _ex tests — against
sampler_ref on the paths they share, hand-worked cases of each quirk, and planted mistakes on the GPU test's own inputs.

The reference has no unit test of min-p or Mirostat (src/sampling/mod.rs:423-465 tests the default and greedy configs, greedy
sampling and reset, which tests/test_sampler_ref.py restates); what it fixes about them is the presets' fields, restated below."""
import numpy as np
import pytest

from sampler_ref import PRESETS, Sampler
from sampler_ref_ex import F, MUTANTS, PRESETS_EX, SamplerEx, mu_bound, ulp32
import test_gpu_sample_ex as G


def _flat(**kw):
    base = dict(temperature=1.0, top_k=0, top_p=1.0, repeat_penalty=1.0, repeat_window=0)
    base.update(kw)
    return base


def _logits(probs):
    return np.log(np.array(probs, np.float64)).astype(np.float32)


# ---- the reference's presets (sampling/mod.rs:26-34, 100-135)
def test_reference_presets(pkg):
    c, m = PRESETS_EX["creative_ref"], PRESETS_EX["mirostat_v2"]
    assert (c["temperature"], c["top_k"], c["top_p"], c["min_p"], c["repeat_penalty"], c["repeat_window"]) == (1.0, 0, 0.9, 0.05, 1.2, 64)
    assert (m["temperature"], m["top_k"], m["top_p"], m["repeat_penalty"], m["repeat_window"]) == (1.0, 0, 1.0, 1.0, 0)
    assert (m["mirostat"], m["tau"], m["eta"]) == (2, 5.0, 0.1)   # MirostatConfig::default
    hb = pkg.hip_backend
    assert hb.SAMPLER_PRESETS["creative_ref"] == c and hb.SAMPLER_PRESETS["mirostat_v2"] == m
    assert hb.SAMPLER_PRESETS["creative"] == PRESETS["creative"]   # the min-p-less entry stays
    ex = hb.sampler_config_ex(**m)
    assert (ex.struct_size, ex.mirostat, ex.mirostat_tau, ex.base.top_p, ex.min_p) == (52, 2, 5.0, 1.0, 0.0)
    for sym in ("lgh_set_sampler_ex", "lgh_batch_set_sampler_ex", "lgh_get_sampler_mu", "lgh_op_sample_ex"):
        assert sym in hb.ABI_SYMBOLS and getattr(hb.load_library(), sym) is not None


# ---- the shared paths
def test_without_min_p_and_mirostat_it_is_sampler_ref():
    rng = np.random.default_rng(12)
    configs = [PRESETS["engine_default"], PRESETS["server"], PRESETS["creative"], PRESETS["greedy"], _flat(top_k=5, top_p=0.5)]
    for i in range(200):
        vocab = int(rng.choice([5, 64, 300, 2000]))
        cfg = configs[i % len(configs)]
        x = G._llm_like(rng, vocab, spikes=3) if i % 2 else rng.normal(0, 1, vocab).astype(np.float32)
        recent = rng.integers(0, vocab, size=int(rng.integers(0, 80))).tolist()
        a, b = Sampler(vocab, **cfg), SamplerEx(vocab, min_p=0.0, mirostat=0, **cfg)
        a.counts[:] = b.counts[:] = rng.integers(0, 3, vocab) * (rng.random(vocab) < 0.1)
        r = float(rng.random(dtype=np.float32))
        assert a.decide(x, recent, r) == b.decide(x, recent, r), (i, cfg)
        assert a.fixed_margin == b.fixed_margin
        assert a.sample(x, recent, r) == b.sample(x, recent, r) and np.array_equal(a.counts, b.counts)
        assert b.mu == F(10) and b.mu_steps == 0   # Sampler::new without Mirostat (mod.rs:161); never touched


# ---- the quirks, worked by hand
def test_min_p_cuts_before_top_k_and_never_to_nothing():
    x = _logits([0.5, 0.3, 0.1, 0.06, 0.04])
    s = SamplerEx(5, **_flat(min_p=0.5))               # threshold 0.25: keeps 0.5, 0.3 -> cumulative 0.625, 1.0
    assert [s.decide(x, [], r)[0] for r in (0.6, 0.63, 0.99)] == [0, 1, 1]
    s = SamplerEx(5, **_flat(min_p=0.15, top_k=4))     # threshold 0.075 keeps three; top_k 4 is not below that length
    assert s.decide(x, [], 0.999)[0] == 2
    s = SamplerEx(5, **_flat(min_p=0.15, top_k=2))     # ... and top_k 2 is
    assert s.decide(x, [], 0.999)[0] == 1
    s = SamplerEx(5, **_flat(min_p=1.0))               # threshold = the top probability itself: the top token stays
    assert s.decide(x, [], 0.999)[0] == 0 and s.fixed_margin > 0.1   # (not "ambiguous": it sits ON its threshold in any arithmetic)
    tie = SamplerEx(4, **_flat(min_p=1.0))             # ... with everything that ties it, in index order
    assert [tie.decide([1.0, 0.0, 1.0, 1.0], [], r)[0] for r in (0.2, 0.5, 0.9)] == [0, 2, 3]
    assert SamplerEx(5, **_flat(min_p=0.5, temperature=0.0)).decide([0.0, 2.0, 2.0, 1.0, 0.0], [], 0.3)[::2] == (2, False)   # greedy first


def test_top_p_cutoff_zero_keeps_the_min_p_set():
    x = _logits([0.95, 0.03, 0.015, 0.005])
    s = SamplerEx(4, **_flat(min_p=0.02, top_p=0.9))   # 0.95 > top_p at position 0: nothing more is cut; min-p kept 0.95, 0.03
    assert s.decide(x, [], 0.9999)[0] == 1             # (renormalized cumulative 0.969, 1.0; without min-p: token 3)
    assert SamplerEx(4, **_flat(top_p=0.9)).decide(x, [], 0.9999)[0] == 3


def test_mirostat_v2_truncates_at_max_rank_1():
    x = _logits([0.6, 0.3, 0.06, 0.04])                # surprises 0.737, 1.737, 4.06, 4.64
    for mu, kept in ((0.5, 1), (1.0, 1), (2.0, 2), (4.5, 3), (5.0, 4)):
        s = SamplerEx(4, **PRESETS_EX["mirostat_v2"])
        s.mu = F(mu)
        cs = np.cumsum(np.array([0.6, 0.3, 0.06, 0.04], np.float32)[:kept], dtype=np.float32)
        want = int(np.nonzero(cs > F(F(0.97) * cs[-1]))[0][0])
        assert s.decide(x, [], 0.97)[0] == want == kept - 1, (mu, kept)


def test_mirostat_fallback_is_the_top_token_and_the_sum_is_not_renormalized():
    x = _logits([0.1, 0.6, 0.3])
    for version in (1, 2):
        s = SamplerEx(3, **_flat(mirostat=version, tau=5.0))
        assert s.decide(x, [], 1.0)[0] == 1            # r * fsum is not below the last cumulative sum: token 1, not token 0 (the last)
        assert s.decide(x, [], 0.65)[0] == 2 and s.decide(x, [], 0.95)[0] == 0
    s = SamplerEx(3, **PRESETS_EX["mirostat_v2"])
    s.mu = F(1.0)                                      # keeps 0.6 only... (rank 1 exceeds): r * 0.6 against 0.6
    assert s.decide(x, [], 0.999)[0] == 1


def test_no_legal_draw_reaches_the_mirostat_fallback():
    """Why the fallback cases draw 1.001: rng.gen::<f32>() is at most 1 - 2^-24, and fl(r * fsum) is then below fsum for every
    f32 fsum (fsum * 2^-24 is at least half an ulp of fsum, and exactly half only at a power of two, whose lower neighbour is
    half an ulp away).  The last cumulative sum IS fsum, so `cumsum > r * fsum` holds there at the latest: the largest legal
    draw selects the last candidate, and the fallback branch (mod.rs:338, 366) is dead code under a legal draw."""
    r = float(np.nextafter(F(1), F(0)))
    rng = np.random.default_rng(5)
    fs = np.concatenate([rng.random(20000, dtype=np.float32) + F(1e-3), F(2.0) ** np.arange(-20, 2, dtype=np.float32)]).astype(F)
    assert np.all((F(r) * fs).astype(F) < fs)
    for case in G.crafted_cases():
        x, cfg, recent, counts, r_case, mu = case
        if cfg.get("mirostat") and r_case > 1.0 and not recent:
            s = SamplerEx(len(x), **cfg)
            s.mu = F(mu)
            p = s.probs(x, [])
            order = np.argsort(-p, kind="stable")
            tok = s.sample(x, [], r)
            assert tok != order[0] and tok == G.reference((x, cfg, (), None, r, mu), mutant="last_fallback")[0]


def test_mirostat_ignores_temperature_and_top_k_1_and_always_counts():
    x = _logits([0.1, 0.6, 0.3])
    s = SamplerEx(3, temperature=0.0, top_k=1, top_p=0.1, min_p=0.9, repeat_penalty=1.0, mirostat=2, tau=5.0, eta=0.1)
    assert not s.greedy
    assert s.sample(x, [], 0.95) == 0 and s.counts.tolist() == [1, 0, 0]
    hot = SamplerEx(3, temperature=5.0, top_k=0, top_p=1.0, repeat_penalty=1.0, mirostat=1)
    assert np.array_equal(hot.probs(x, []), SamplerEx(3, **_flat()).probs(x, []))
    pen = SamplerEx(3, **_flat(mirostat=2, repeat_penalty=2.0, frequency_penalty=0.5))   # the penalties still come first
    pen.counts[:] = [0, 2, 0]
    assert pen.penalized([2.0, 4.0, -1.0], [0, 2]).tolist() == [1.0, 3.0, -2.0]


def test_mu_starts_at_two_tau_clamps_and_freezes_after_eos():
    s = SamplerEx(3, **_flat(mirostat=2, tau=3.5, eta=0.1))
    assert s.mu == F(7.0) and s.mu64 == 7.0
    x = _logits([0.5, 0.25, 0.25])
    s.sample(x, [], 0.1)                               # token 0, surprise 1: mu = 7 - 0.1 * (1 - 3.5)
    assert s.mu == F(F(7.0) - F(F(0.1) * F(F(1.0) - F(3.5)))) and abs(s.mu64 - 7.25) < 1e-7
    up = SamplerEx(3, **_flat(mirostat=2, tau=10.0, eta=1.0))   # mu 20: 20 + 9 clamps to 20
    up.sample(x, [], 0.1)
    assert up.mu == F(20) and up.mu64 == 20.0
    down = SamplerEx(3, **_flat(mirostat=1, tau=0.0, eta=5.0))  # mu 0: 0 - 5 clamps to 0
    down.sample(x, [], 0.1)
    assert down.mu == F(0) and down.mu64 == 0.0
    before = (float(s.mu), s.mu64, s.counts.copy())
    tok, _, counted = s.decide(x, [], 0.9)
    s.commit(tok, counted, frozen=True)                # a step after eos
    assert (float(s.mu), s.mu64) == before[:2] and np.array_equal(s.counts, before[2])


def test_mu_bound():
    assert ulp32(20.0) == 2.0 ** -19 and ulp32(5.0) == 2.0 ** -21
    assert mu_bound(24, 0.1, 5.0) == 24 * (0.1 * 4 * 2.0 ** -21 + 2.0 ** -19)


# ---- the GPU test's inputs: quiet enough, and sharp enough
@pytest.mark.parametrize("vocab", G.VOCABS)
def test_the_random_inputs_leave_out_at_most_a_tenth(vocab):
    cases = G.random_cases(vocab)
    margins = [G.reference(c)[1] for c in cases]
    assert sum(m <= G.TOL for m in margins) <= len(cases) // 10
    for case in cases:                                  # and the f32 mu stays within the bound of the float64 recurrence
        if case[1].get("mirostat"):
            _, _, mu32, mu64, s = G.reference(case)
            assert abs(mu32 - mu64) <= mu_bound(1, case[1]["eta"], s)


def test_no_crafted_input_is_left_out():
    for i, case in enumerate(G.crafted_cases()):
        assert G.reference(case)[1] > G.TOL, (i, case[1], case[4])


def _observations(mutant):
    """What the GPU tests compare, computed by a sampler with `mutant` planted: [(token, mu or None, bound on mu, checked)]."""
    out = []
    for cases in [G.random_cases(v) for v in (7, 65, 1000)] + [G.crafted_cases()]:
        for case in cases:
            _, margin, _, mu64, s = G.reference(case)
            tok, _, mu32, _, _ = G.reference(case, mutant)
            miro = bool(case[1].get("mirostat"))
            out.append((tok, mu32 if miro else None, (mu64, mu_bound(1, case[1].get("eta", 0.0), s)), margin > G.TOL))
    for cfg in G.TRAJECTORIES:
        real = list(G.trajectory(cfg))
        draws = [step[3] for step in real]
        state = [(float(s.mu), s.mu64, s.bound()) for *_, s in _freeze(G.trajectory(cfg))]
        planted = [(tok, float(s.mu)) for *_, tok, s in _freeze(G.trajectory(cfg, draws, mutant))]
        for (tok, mu), (_, mu64, bound) in zip(planted, state):
            out.append((tok, mu, (mu64, bound), True))
    return out


def _freeze(gen):
    """The trajectory's sampler is one live object: copy what a later step would change."""
    import copy
    for *head, s in gen:
        yield (*head, copy.copy(s))


@pytest.mark.parametrize("mutant", [m for m in MUTANTS if m != "min_p_after_top_k"])
def test_planted_mistakes_are_told_apart(mutant):
    """Each mistake changes a token the GPU test compares, or pushes mu outside the bound it asserts."""
    real, planted = _observations(None), _observations(mutant)
    caught = 0
    for (tok, mu, (mu64, bound), checked), (tok_m, mu_m, _, _) in zip(real, planted):
        assert mu is None or abs(mu - mu64) <= bound
        if checked and (tok_m != tok or (mu is not None and abs(mu_m - mu64) > bound)):
            caught += 1
    assert caught > 0, mutant


def test_min_p_after_top_k_is_no_mistake():
    """min-p and top-k both cut the same sorted order to a prefix, and min-p's threshold reads only the first entry: whichever
    runs first, min(top_k, min-p length) entries remain.  No input can tell the two orders apart (so this one cannot be a
    mutant that a test catches); shown on every min-p input of the GPU test."""
    n = 0
    for cases in [G.random_cases(v) for v in (7, 65, 1000)] + [G.crafted_cases()]:
        for case in cases:
            if case[1].get("min_p") and not case[1].get("mirostat"):
                assert G.reference(case)[0] == G.reference(case, "min_p_after_top_k")[0]
                n += 1
    assert n > 100
