"""The numpy restatement of Sampler::sample (tests/sampler_ref.py) completed with the two paths it left out: min-p
(src/sampling/mod.rs:248-258) and Mirostat v1 / v2 (mod.rs:210-213, 304-387).  The arbiter of the device sampler's _ex tests.

Everything is f32 and every sum sequential (np.cumsum(dtype=f32)), as in sampler_ref.  `decide` keeps reporting a margin; it
now also covers
  * min-p: the relative distance to the threshold p[order[0]] * min_p of the probabilities at ranks cutoff-1 and cutoff.  A rank
    whose penalized logit EQUALS the top one's is left out of this: its probability is the same number as p[order[0]] in any
    implementation, and fl(p0 * min_p) <= p0, so `p < threshold` is false for it whatever the rounding of exp and of the sum
    (without this, min_p = 1.0 would make every case "ambiguous": the top token sits exactly on its own threshold);
  * Mirostat v2: |surprise - mu| (absolute, as both are O(1..20)) at the rank that first exceeded mu and at the one before it,
    or at the last rank when none exceeded it;
  * the Mirostat draw: cumsum against r * fsum.
Next to the f32 mu the class evaluates the mu recurrence in float64 from the f32 selected probabilities (`mu64`): the
yardstick of the mu tests, with `mu_bound` the distance either f32 evaluation may keep from it.

`mutant` plants one mistake (tests/test_sampler_ref_ex.py shows that the GPU test's inputs tell each from the real thing)."""
from __future__ import annotations

import math

import numpy as np

from sampler_ref import F, PRESETS, Sampler, _rel

PRESETS_EX = dict(PRESETS)
# SamplerConfig::creative with its min_p (sampling/mod.rs:100-114)
PRESETS_EX["creative_ref"] = dict(PRESETS["creative"], min_p=0.05)
# SamplerConfig::mirostat_v2(5.0, 0.1) (sampling/mod.rs:116-135)
PRESETS_EX["mirostat_v2"] = dict(temperature=1.0, top_k=0, top_p=1.0, repeat_penalty=1.0, repeat_window=0, mirostat=2, tau=5.0, eta=0.1)

MUTANTS = ("eta_1.01", "mu_init_tau", "natural_log", "renormalize", "last_fallback", "min_p_after_top_k")


def ulp32(x) -> float:
    return float(np.spacing(F(abs(x))))


def mu_bound(steps: int, eta: float, s_max: float) -> float:
    """steps * (|eta| * 4 * ulp32(s_max) + ulp32(20)): each log2f is good to a few ulp of the surprise, then mu is rounded once."""
    return steps * (abs(float(eta)) * 4.0 * ulp32(s_max) + ulp32(20.0))


class SamplerEx(Sampler):
    """Sampler::new(config, vocab_size) with min_p and MirostatConfig: the config, zeroed counts and mirostat_mu = 2 * tau."""

    def __init__(self, vocab: int, min_p=0.0, mirostat=0, tau=5.0, eta=0.1, mutant=None, **cfg):
        super().__init__(vocab, **cfg)
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant
        self.min_p, self.mirostat, self.tau, self.eta = F(min_p), int(mirostat), F(tau), F(eta)
        if mutant == "eta_1.01":
            self.eta = F(self.eta * F(1.01))
        self.mu = (self.tau if mutant == "mu_init_tau" else F(self.tau * F(2))) if self.mirostat else F(10)
        self.mu64 = float(self.mu)      # the float64 recurrence
        self.s_max = 0.0                # the largest surprise on the trajectory
        self.mu_steps = 0
        self._psel = None

    @property
    def greedy(self) -> bool:
        return not self.mirostat and super().greedy

    def penalized(self, logits, recent) -> np.ndarray:
        if not self.mirostat:
            return super().penalized(logits, recent)
        keep, self.temperature = self.temperature, F(1)   # sample_mirostat returns before the temperature (mod.rs:210-221)
        try:
            return super().penalized(logits, recent)
        finally:
            self.temperature = keep

    def _log2(self, p):
        with np.errstate(divide="ignore"):
            return np.log(p).astype(F) if self.mutant == "natural_log" else np.log2(p).astype(F)

    # ---- the decision
    def _decide(self, logits, recent, r: float):
        self._psel = None
        if self.mirostat:
            return self._decide_mirostat(logits, recent, r)
        if self.greedy:
            return super()._decide(logits, recent, r)
        x = self.penalized(logits, recent)
        p = self.probs(logits, recent)
        n = len(p)
        order = np.argsort(-p, kind="stable")
        margin = np.inf

        def min_p(order, margin):
            if not self.min_p > F(0):
                return order, margin
            thr = F(p[order[0]] * self.min_p)
            below = np.nonzero(p[order] < thr)[0]
            cutoff = int(below[0]) if below.size else len(order)
            if cutoff > 0 and x[order[cutoff - 1]] != x[order[0]]:
                margin = min(margin, _rel(p[order[cutoff - 1]], thr))
            if below.size:
                margin = min(margin, _rel(p[order[cutoff]], thr))
            return (order[:cutoff] if cutoff > 0 else order), margin

        def top_k(order, margin):
            if 0 < self.top_k < len(order):
                if p[order[self.top_k - 1]] != p[order[self.top_k]]:
                    margin = min(margin, _rel(p[order[self.top_k - 1]], p[order[self.top_k]]))
                order = order[:self.top_k]
            return order, margin

        for step in ((top_k, min_p) if self.mutant == "min_p_after_top_k" else (min_p, top_k)):
            order, margin = step(order, margin)
        if self.top_p < F(1):
            cs = np.cumsum(p[order], dtype=F)
            over = np.nonzero(cs > self.top_p)[0]
            cutoff = int(over[0]) if over.size else len(order)
            if over.size:
                margin = min(margin, _rel(cs[cutoff], self.top_p))
                if cutoff > 0:
                    margin = min(margin, _rel(cs[cutoff - 1], self.top_p))
            else:
                margin = min(margin, _rel(cs[-1], self.top_p))
            if cutoff > 0:   # (a cutoff at 0 truncates nothing, so it keeps the min-p set)
                order = order[:cutoff + 1]
        fixed = margin
        kept = p[order]
        fsum = np.cumsum(kept, dtype=F)[-1]
        cum = np.cumsum((kept / fsum).astype(F), dtype=F)
        r = F(r)
        hit = np.nonzero(r < cum)[0]
        if hit.size:
            k = int(hit[0])
            margin = min(margin, _rel(r, cum[k]))
            if k > 0:
                margin = min(margin, _rel(r, cum[k - 1]))
            tok = int(order[k])
        else:   # fallback: the last kept token
            margin = min(margin, _rel(r, cum[-1]))
            tok = int(order[-1])
        return tok, margin, True, fixed

    def _decide_mirostat(self, logits, recent, r: float):
        p = self.probs(logits, recent)
        n = len(p)
        order = np.argsort(-p, kind="stable")
        margin = np.inf
        if self.mirostat == 2:   # the first rank whose surprise exceeds mu, at least 1 (mod.rs:348-359)
            s = -self._log2(p[order])
            over = np.nonzero(s > self.mu)[0]
            if over.size:
                rank = int(over[0])
                trunc = max(rank, 1)
                margin = min(margin, abs(float(s[rank]) - float(self.mu)))
                if rank > 0:
                    margin = min(margin, abs(float(s[rank - 1]) - float(self.mu)))
            else:
                trunc = n
                margin = min(margin, abs(float(s[-1]) - float(self.mu)))
        else:
            # v1 (mod.rs:325-330): n = clamp((2^mu * vocab) as usize, 1, vocab).  tau >= 0 is required, so mu starts at
            # 2 * tau >= 0 and is clamped to [0, 20] after every update: 2^mu >= 1 and n == vocab, no truncation.
            assert F(0) <= self.mu <= F(20)
            trunc = min(max(int(F(F(2) ** self.mu) * F(n)), 1), n)
            assert trunc == n
        fixed = margin
        cand = order[:trunc]
        kept = p[cand]
        if self.mutant == "renormalize":
            kept = (kept / np.cumsum(kept, dtype=F)[-1]).astype(F)
        cs = np.cumsum(kept, dtype=F)
        rr = F(F(r) * cs[-1])
        hit = np.nonzero(cs > rr)[0]
        if hit.size:
            k = int(hit[0])
            margin = min(margin, _rel(rr, cs[k]))
            if k > 0:
                margin = min(margin, _rel(rr, cs[k - 1]))
        else:   # nobody above r: the TOP token (mod.rs:338, 366), not the last kept one
            margin = min(margin, _rel(rr, cs[-1]))
            k = len(cand) - 1 if self.mutant == "last_fallback" else 0
        tok = int(cand[k])
        # (the update reads the unnormalized probability, mod.rs:378; a sampler that renormalized in place would read the other)
        self._psel = F(kept[k]) if self.mutant == "renormalize" else F(p[tok])
        return tok, margin, True, fixed

    # ---- the state
    def commit(self, tok: int, counted: bool = True, frozen: bool = False) -> None:
        """What sample() does after the decision: count the token and, under Mirostat, update mu (mod.rs:377-385).  `frozen`:
        a step after the one that sampled eos_token, which updates neither (the library's contract for those steps)."""
        if frozen:
            return
        if counted:
            self.counts[tok] += 1
        if self.mirostat:
            ps = self._psel
            s = F(-self._log2(np.array([ps], dtype=F))[0])
            self.mu = F(min(max(F(self.mu - F(self.eta * F(s - self.tau))), F(0)), F(20)))
            s64 = -math.log2(float(ps)) if ps > 0 else math.inf
            self.mu64 = min(max(self.mu64 - float(self.eta) * (s64 - float(self.tau)), 0.0), 20.0)
            if math.isfinite(s64):
                self.s_max = max(self.s_max, s64)
            self.mu_steps += 1

    def sample(self, logits, recent, r: float) -> int:
        tok, _, counted = self.decide(logits, recent, r)
        self.commit(tok, counted)
        return tok

    def bound(self) -> float:
        return mu_bound(self.mu_steps, self.eta, self.s_max)


def draw_unambiguous_ex(sampler: SamplerEx, logits, recent, rng, tol=1e-5, tries=64, frozen=False):
    """sampler_ref.draw_unambiguous for a SamplerEx: (r, token, settled), the token committed (counts and mu)."""
    for _ in range(tries):
        r = F(rng.random(dtype=np.float32))
        tok, margin, counted = sampler.decide(logits, recent, r)
        if margin > tol or sampler.fixed_margin <= tol:
            sampler.commit(tok, counted, frozen)
            return float(r), tok, sampler.fixed_margin > tol
    raise AssertionError("no unambiguous draw found")
