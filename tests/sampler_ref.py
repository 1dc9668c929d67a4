"""A numpy restatement of the reference's Sampler::sample (src/sampling/mod.rs:188-304, non-mirostat path; penalties 390-424).

It is the arbiter of the device sampler's tests.  Every step is f32 as in the reference; every sum is SEQUENTIAL f32
(np.cumsum accumulates left to right, np.sum would sum pairwise).  `decide` also reports how close the decision came to a
boundary — the draw against the cumulative sums, the top-p cut against top_p, a probability tie at the top-k edge —
as a relative distance, so that a test can tell a real mismatch from a step that f32 rounding may legitimately flip."""
from __future__ import annotations

import numpy as np

F = np.float32

PRESETS = {
    # EngineConfig::default's sampling settings (src/engine.rs:117-130)
    "engine_default": dict(temperature=0.7, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_window=64),
    # what the OpenAI-style server adds (src/server/handlers.rs:292-298)
    "server": dict(temperature=1.0, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_window=64, frequency_penalty=0.5,
                   presence_penalty=0.3),
    # SamplerConfig::creative (sampling/mod.rs:96-110) without min_p, which no reference caller sets
    "creative": dict(temperature=1.0, top_k=0, top_p=0.9, repeat_penalty=1.2, repeat_window=64),
    # SamplerConfig::greedy (sampling/mod.rs:82-94)
    "greedy": dict(temperature=0.0, top_k=1, top_p=1.0, repeat_penalty=1.0, repeat_window=0),
}


def _rel(a, b) -> float:
    a, b = float(a), float(b)
    d = max(abs(a), abs(b))
    return abs(a - b) / d if d > 0 else 0.0


class Sampler:
    """Sampler::new(config, vocab_size): the config and zeroed token counts."""

    def __init__(self, vocab: int, temperature=0.8, top_k=40, top_p=0.95, repeat_penalty=1.1, repeat_window=64,
                 frequency_penalty=0.0, presence_penalty=0.0, eos_token=-1):
        self.vocab = vocab
        self.temperature, self.top_p = F(temperature), F(top_p)
        self.repeat_penalty, self.frequency_penalty, self.presence_penalty = F(repeat_penalty), F(frequency_penalty), F(presence_penalty)
        self.top_k, self.repeat_window, self.eos_token = int(top_k), int(repeat_window), int(eos_token)
        self.counts = np.zeros(vocab, dtype=np.int64)

    @property
    def greedy(self) -> bool:
        return self.temperature == F(0) or self.top_k == 1

    def penalized(self, logits, recent) -> np.ndarray:
        x = np.array(logits, dtype=F, copy=True)
        if self.repeat_penalty != F(1):   # apply_repetition_penalty: once per occurrence, in window order
            recent = list(recent)
            w = min(len(recent), self.repeat_window) if self.repeat_window > 0 else len(recent)
            for t in recent[len(recent) - w:]:
                if t < len(x):
                    x[t] = x[t] / self.repeat_penalty if x[t] > F(0) else x[t] * self.repeat_penalty
        if self.frequency_penalty != F(0) or self.presence_penalty != F(0):   # apply_frequency_presence_penalty
            m = self.counts > 0
            x[m] = x[m] - self.frequency_penalty * self.counts[m].astype(F)
            x[m] = x[m] - self.presence_penalty
        if self.temperature > F(0) and self.temperature != F(1):
            x = x * (F(1) / self.temperature)
        return x

    def probs(self, logits, recent) -> np.ndarray:
        x = self.penalized(logits, recent)
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.exp(x - x.max()).astype(F)
            s = np.cumsum(e, dtype=F)[-1]
            return (e / s).astype(F)

    def decide(self, logits, recent, r: float):
        """(token, margin, counted): what sample() would return, the relative distance of the decision to its nearest
        boundary (inf when there is none), and whether the token is counted.  `self.fixed_margin` keeps the part of the
        margin that no draw can change (greedy near-ties, the top-k edge, the top-p cut)."""
        tok, margin, counted, self.fixed_margin = self._decide(logits, recent, r)
        return tok, margin, counted

    def _decide(self, logits, recent, r: float):
        p = self.probs(logits, recent)
        n = len(p)
        if self.greedy:   # max_by: the LAST maximal probability
            tok = n - 1 - int(np.argmax(p[::-1]))
            others = p[p != p[tok]]
            margin = _rel(p[tok], others.max()) if others.size else np.inf
            return tok, margin, False, margin
        order = np.argsort(-p, kind="stable")   # stable: equal probabilities keep ascending index order
        margin = np.inf
        if 0 < self.top_k < n:
            if p[order[self.top_k - 1]] != p[order[self.top_k]]:
                margin = min(margin, _rel(p[order[self.top_k - 1]], p[order[self.top_k]]))
            order = order[:self.top_k]
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
            if cutoff > 0:   # (a cutoff at 0 truncates nothing: reference quirk)
                order = order[:cutoff + 1]
        fixed = margin
        kept = p[order]
        fsum = np.cumsum(kept, dtype=F)[-1]
        q = (kept / fsum).astype(F)
        cum = np.cumsum(q, dtype=F)
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

    def sample(self, logits, recent, r: float) -> int:
        tok, _, counted = self.decide(logits, recent, r)
        if counted:
            self.counts[tok] += 1
        return tok


def draw_unambiguous(sampler: Sampler, logits, recent, rng, tol=1e-5, tries=64):
    """(r, token, settled): a uniform whose draw stays more than `tol` (relative) from the cumulative sums, the token it gives
    (counted), and whether the rest of the decision (greedy near-ties, the top-k edge, the top-p cut) is settled too — no
    draw can change that part."""
    for _ in range(tries):
        r = F(rng.random(dtype=np.float32))
        tok, margin, counted = sampler.decide(logits, recent, r)
        if margin > tol or sampler.fixed_margin <= tol:
            if counted:
                sampler.counts[tok] += 1
            return float(r), tok, sampler.fixed_margin > tol
    raise AssertionError("no unambiguous draw found")
