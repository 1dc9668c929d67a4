"""The numpy restatement of Sampler::sample (tests/sampler_ref.py) — the arbiter of the device sampler — against the
reference's own sampler tests (src/sampling/mod.rs:442-464) and hand-worked cases of each quirk it has; and the build
properties of the sampling kernels (csrc/sample.hip)."""
import os
import re
import subprocess

import numpy as np

import __graft_entry__ as graft
from sampler_ref import F, PRESETS, Sampler, draw_unambiguous


# ---- the reference's tests (sampling/mod.rs:442-464)
def test_reference_default_config():
    s = Sampler(10)   # SamplerConfig::default
    assert s.temperature == F(0.8) and s.top_k == 40 and abs(float(s.top_p) - 0.95) < 0.001


def test_reference_greedy_config():
    s = Sampler(10, **PRESETS["greedy"])
    assert s.temperature == F(0) and s.top_k == 1


def test_reference_greedy_sampling():
    s = Sampler(10, **PRESETS["greedy"])
    logits = [0.0, 0.1, 0.2, 0.3, 0.4, 1.0, 0.2, 0.1, 0.0, -0.1]
    assert s.sample(logits, [], 0.5) == 5


def test_reference_sampler_reset():
    s = Sampler(10)
    s.counts[5] = 10
    s = Sampler(10)   # Sampler::reset zeroes the counts, as a new sampler has them
    assert s.counts[5] == 0


# ---- the quirks, worked by hand
def _flat(**kw):
    base = dict(temperature=1.0, top_k=0, top_p=1.0, repeat_penalty=1.0, repeat_window=0)
    base.update(kw)
    return base


def test_ties_keep_index_order():
    s = Sampler(4, **_flat(top_k=2))
    logits = [1.0, 1.0, 1.0, 0.0]   # three equal probabilities; the stable sort keeps 0, 1, 2 in that order
    assert s.decide(logits, [], 0.4)[0] == 0
    assert s.decide(logits, [], 0.6)[0] == 1   # the kept pair is (0, 1), never 2


def test_greedy_picks_the_last_maximum():
    s = Sampler(4, **PRESETS["greedy"])
    assert s.decide([0.0, 2.0, 2.0, 1.0], [], 0.0)[0] == 2


def test_top_p_cutoff_zero_keeps_everything():
    s = Sampler(4, **_flat(top_p=0.5))
    logits = [10.0, 0.0, 0.0, 0.0]   # p0 = 0.99986 > top_p at position 0: nothing is truncated
    p = s.probs(logits, [])
    cum = np.cumsum(p / np.cumsum(p, dtype=F)[-1], dtype=F)
    r = float((cum[1] + cum[2]) / 2)
    assert s.decide(logits, [], r)[0] == 2


def test_top_p_cut_keeps_the_crossing_token():
    s = Sampler(4, **_flat(top_p=0.6))
    logits = np.log([0.4, 0.3, 0.2, 0.1]).astype(np.float32)   # cumsum 0.4, 0.7 > 0.6 at position 1: keep 2
    assert s.decide(logits, [], 0.99)[0] == 1


def test_repetition_penalty_compounds_and_multiplies_non_positive():
    s = Sampler(4, temperature=0.0, top_k=1, top_p=1.0, repeat_penalty=2.0, repeat_window=0)
    x = s.penalized([2.0, -1.0, 0.0, 1.0], [0, 0, 1, 2])
    assert x.tolist() == [0.5, -2.0, 0.0, 1.0]   # 2 / 2 / 2; -1 * 2; 0 * 2 (x > 0 is false)
    assert s.decide([2.0, -1.0, 0.0, 1.0], [0, 0, 1, 2], 0.0)[0] == 3


def test_repetition_window_is_the_end_of_recent():
    s = Sampler(4, temperature=0.0, top_k=1, top_p=1.0, repeat_penalty=2.0, repeat_window=2)
    assert s.penalized([2.0, 2.0, 2.0, 2.0], [0, 1, 2, 2]).tolist() == [2.0, 2.0, 0.5, 2.0]


def test_frequency_then_presence_penalty():
    s = Sampler(3, **_flat(frequency_penalty=0.5, presence_penalty=0.25))
    s.counts[:] = [0, 1, 3]
    x = s.penalized([1.0, 1.0, 1.0], [])
    assert x.tolist() == [1.0, F(F(1.0) - F(0.5)) - F(0.25), F(F(1.0) - F(1.5)) - F(0.25)]


def test_temperature_multiplies_by_the_f32_reciprocal():
    s = Sampler(2, **_flat(temperature=0.7))
    x = s.penalized([3.0, 1.0], [])
    assert x[0] == F(3.0) * (F(1) / F(0.7))


def test_fallback_returns_the_last_kept_index():
    s = Sampler(4, **_flat(top_k=3))
    logits = [0.0, 0.0, 0.0, 0.0]   # kept 0, 1, 2 with cumsum 1/3, 2/3, 1.0; r = 1.0 is below none of them
    assert s.decide(logits, [], 1.0)[0] == 2


def test_greedy_does_not_count_and_sampling_does():
    g = Sampler(4, **PRESETS["greedy"])
    g.sample([0.0, 1.0, 0.0, 0.0], [], 0.3)
    assert g.counts.sum() == 0
    s = Sampler(4, **_flat())
    t = s.sample([0.0, 1.0, 0.0, 0.0], [], 0.3)
    assert s.counts.sum() == 1 and s.counts[t] == 1


def test_sums_are_sequential_f32():
    rng = np.random.default_rng(3)
    logits = rng.normal(0, 3, 5000).astype(np.float32)
    s = Sampler(5000, **_flat())
    e = np.exp(logits - logits.max()).astype(F)
    acc = F(0)
    for v in e:
        acc = F(acc + v)
    assert np.array_equal(s.probs(logits, []), (e / acc).astype(F))


def test_unambiguous_draws_stay_off_the_boundaries():
    rng = np.random.default_rng(5)
    s = Sampler(1000, **PRESETS["engine_default"])
    for _ in range(20):
        logits = rng.normal(0, 2, 1000).astype(np.float32)
        before = s.counts.copy()
        r, tok, settled = draw_unambiguous(s, logits, [], rng)
        s.counts[:] = before
        t2, margin, _ = s.decide(logits, [], r)
        assert t2 == tok and (margin > 1e-5 or not settled)


# ---- build properties of the sampling kernels
def test_sampling_kernels_use_no_scratch_and_do_not_spill():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mllvm", "-amdgpu-kernarg-preload-count=8",
             "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c"]
    out = subprocess.run([hipcc, *flags, os.path.join(graft.PKG_DIR, "csrc", "sample.hip"), "-o", os.devnull],
                         capture_output=True, text=True, check=True).stderr
    usage, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    kernels = {fn for fn in usage if "samp_partial" in fn or "samp_merge" in fn}
    assert len(kernels) == 2, sorted(usage)
    for fn, u in usage.items():
        assert u.get("ScratchSize", 0) == 0, f"{fn} uses {u['ScratchSize']} B/lane of scratch"
        assert u.get("VGPRs Spill", 0) == 0, f"{fn} spills {u['VGPRs Spill']} VGPRs"
