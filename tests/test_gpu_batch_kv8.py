"""Multi-sequence decode over int8 / FP8 KV cache slots (kv_cache_type LGH_KV_INT8 / FP8_E4M3 / FP8_E5M2) against the
single-sequence engine with the same cache type, and against the CPU oracle.

The byte caches have one attention structure (splits + merge, four waves per workgroup whatever max_seq is), and the multi-sequence
step runs that very kernel with the sequence as the grid's second dimension, each sequence's staged K / V rows quantized into its own
slot.  So the bar is the one tests/test_gpu_batch.py sets for f32 slots: every sequence's logits are BIT-IDENTICAL to the
single-sequence engine's on the same token history — and here the single engine needs no attention override.  The single-sequence
byte-cache engine is pinned to the oracle by tests/test_gpu_model.py::test_quantized_kv_cache_follows_the_reference_formats; one test
here repeats that on a multi-sequence step directly.  Slots take their prompts token by token (no batched prompt pass over a byte cache)."""
import numpy as np
import pytest

from sampler_ref import PRESETS

pytestmark = pytest.mark.gpu

KV_NAMES = {1: "int8", 2: "fp8_e4m3", 3: "fp8_e5m2"}


def _config(pkg, name, max_seq, **kw):
    if name == "test-moe-e1024-k4":   # four of eight experts of width 1024 per token: the expert-grouped step (tests/test_gpu_batch.py)
        name, kw = "test-moe", dict(kw, expert_intermediate_size=1024, num_experts=8, num_experts_per_token=4)
    return pkg.make_config(name, max_seq_len=max_seq, **kw)


def _engines(pkg, name, mix, kv, max_seq=64):
    cfg = _config(pkg, name, max_seq)
    model = pkg.SynthModel(cfg, mix=mix)
    multi = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=kv)
    single = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=kv)
    return cfg, model, multi, single


def _history(cfg, seq, n):
    rng = np.random.default_rng(2000 + seq)
    return [int(t) for t in rng.integers(0, cfg.vocab_size, size=n)]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("name,mix,B,kv", [("test-dense", "Q4_K_M", 5, 1), ("test-dense-d128", "Q4_K_M", 16, 1), ("test-dense-d128", "Q6_K", 4, 2),
                                           ("test-dense", "Q8_0", 3, 3), ("test-moe", "Q5_K_M", 4, 1), ("test-moe-e1024-k4", "Q4_K_M", 5, 2)])
def test_every_sequence_gets_the_single_sequence_logits_bitwise(pkg, name, mix, B, kv):
    """B sequences with different histories and RAGGED lengths, token by token through lgh_forward_multi over byte-cache slots; each
    sequence's logits at every step equal, bit for bit, those of a single-sequence engine with the same cache type fed the same history."""
    cfg, model, multi, single = _engines(pkg, name, mix, kv)
    try:
        multi.batch_create(B)
        lens = [3 + (5 * s) % 11 for s in range(B)]                   # sequence s joins the batch `lens[s]` steps before the end
        T = max(lens)
        hist = [_history(cfg, s, lens[s]) for s in range(B)]
        got = [[] for _ in range(B)]
        for step in range(T):
            active = [s for s in range(B) if step >= T - lens[s]]      # ragged: sequences join at different steps
            toks = [hist[s][step - (T - lens[s])] for s in active]
            logits, nxt = multi.forward_multi(active, toks, want_logits=True, greedy=True)
            for i, s in enumerate(active):
                got[s].append(logits[i].copy())
                assert int(nxt[i]) == int(np.flatnonzero(logits[i] == logits[i].max())[-1])
        for s in range(B):
            assert multi.batch_position(s) == lens[s]
            single.reset()
            for t, tok in enumerate(hist[s]):
                want = single.forward(tok)
                assert _bits_equal(got[s][t], want), (KV_NAMES[kv], s, t, float(np.abs(got[s][t] - want).max()))
    finally:
        multi.close()
        single.close()


def test_long_and_short_slots_in_one_step_stay_bitwise(pkg):
    """int8, max_seq 384: one slot with a prompt of 300 rows and one with 5 (both token by token through lgh_batch_prefill), then 4 steps
    of both: the long sequence's workgroups run several batches of cache rows while the short one's mostly see the staged row only."""
    cfg, model, multi, single = _engines(pkg, "test-dense-d128", "Q4_K_M", 1, max_seq=384)
    try:
        multi.batch_create(3)
        slots = [2, 0]
        prompts = [_history(cfg, 310, 301), _history(cfg, 311, 6)]
        for sl, p in zip(slots, prompts):
            multi.batch_prefill(sl, p[:-1])
            assert multi.batch_position(sl) == len(p) - 1
        toks = [p[-1] for p in prompts]
        got = []
        for step in range(4):
            logits, nxt = multi.forward_multi(slots, toks, want_logits=True, greedy=True)
            got.append(logits.copy())
            toks = [int(t) for t in nxt]
        for s in range(2):
            single.reset()
            for t in prompts[s][:-1]:
                single.prefill_token(t)
            tok = prompts[s][-1]
            for step in range(4):
                want = single.forward(tok)
                assert _bits_equal(got[step][s], want), (s, step, float(np.abs(got[step][s] - want).max()))
                tok = int(np.flatnonzero(want == want.max())[-1])
            assert multi.batch_position(slots[s]) == len(prompts[s]) - 1 + 4
    finally:
        multi.close()
        single.close()


@pytest.mark.parametrize("kv", [1, 2], ids=["int8", "fp8_e4m3"])
def test_batched_step_matches_the_cpu_oracle(pkg, orc, kv):
    """The multi-sequence step over byte-cache slots against the CPU oracle with the same format switched on: 4 slots, 6 steps.
    Tolerance: the decode path's (2e-3 max|logit| + 2e-3) for int8 and 4x that for FP8, as
    tests/test_gpu_model.py::test_quantized_kv_cache_follows_the_reference_formats sets and explains them."""
    ktol = 1.0 if kv == 1 else 4.0
    cfg = pkg.make_config("test-dense-d128", max_seq_len=64)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    eng = pkg.HipGpuInference.from_model(model, 64, kv_cache_type=kv)
    try:
        eng.batch_create(4)
        refs = []
        for s in range(4):
            ref = orc.Model(cfg.as_dict())
            for nm, t, ne, data in model.tensors(keep=True):
                ref.add_tensor(nm, t, ne, data)
            ref.finalize()
            if kv == 1:
                ref.set_kv_int8(True)
            else:
                ref.set_kv_fp8(kv - 1)
            refs.append(ref)
        hist = [_history(cfg, 40 + s, 6) for s in range(4)]
        worst = 0.0
        for t in range(6):
            logits, _ = eng.forward_multi([0, 1, 2, 3], [hist[s][t] for s in range(4)])
            for s in range(4):
                want = refs[s].forward([hist[s][t]])
                err = float(np.abs(logits[s] - want).max())
                tol = ktol * (2e-3 * float(np.abs(want).max()) + 2e-3)
                worst = max(worst, err / tol)
                assert err <= tol, (s, t, err, tol)
        print(f"multi-sequence step over {KV_NAMES[kv]} slots vs oracle: worst err / tolerance = {worst:.3f}")
    finally:
        eng.close()


@pytest.mark.parametrize("kv", [1, 3], ids=["int8", "fp8_e5m2"])
def test_device_fed_greedy_loop_reset_and_own_sequence(pkg, kv):
    """lgh_decode_greedy_multi (tokens fed back on the device) equals a host loop over lgh_forward_multi and the single-sequence greedy
    decode; a reset slot starts over while the others keep going; the context's own single sequence (its byte cache and position) is
    untouched by all the slot work."""
    cfg, model, multi, single = _engines(pkg, "test-dense-d128", "Q4_K_M", kv, max_seq=96)
    other = pkg.HipGpuInference.from_model(model, 96, kv_cache_type=kv)
    try:
        B = 3
        multi.batch_create(4)
        own = _history(cfg, 600, 5)
        for tok in own[:4]:                                              # the context's own sequence, before any slot work
            multi.forward(tok)
            other.forward(tok)
        prompts = [_history(cfg, 70 + s, 9 + 7 * s) for s in range(B)]
        slots = [3, 0, 2]                                                # not the identity, one slot left unused
        for s in range(B):
            multi.batch_prefill(slots[s], prompts[s][:-1])
            assert multi.batch_position(slots[s]) == len(prompts[s]) - 1
        dev = multi.decode_greedy_multi(slots, [p[-1] for p in prompts], 12)          # [12, B]
        want = []
        for s in range(B):
            single.reset()
            for t in prompts[s][:-1]:
                single.prefill_token(t)
            want.append(single.decode_greedy(prompts[s][-1], 12))
        for s in range(B):
            assert np.array_equal(dev[:, s], want[s]), (s, dev[:, s], want[s])
            assert multi.batch_position(slots[s]) == len(prompts[s]) - 1 + 12
        # host loop on fresh slots == device loop
        for s in range(B):
            multi.batch_reset(slots[s])
            multi.batch_prefill(slots[s], prompts[s][:-1])
        toks = [p[-1] for p in prompts]
        for step in range(12):
            _, nxt = multi.forward_multi(slots, toks, want_logits=False, greedy=True)
            assert np.array_equal(nxt, dev[step])
            toks = [int(t) for t in nxt]
        # one slot starts over with another prompt while the others continue
        multi.batch_reset(slots[1])
        assert multi.batch_position(slots[1]) == 0
        p2 = _history(cfg, 99, 9)
        multi.batch_prefill(slots[1], p2[:-1])
        l_multi, _ = multi.forward_multi([slots[1], slots[0]], [p2[-1], toks[0]])
        single.reset()
        for t in p2[:-1]:
            single.prefill_token(t)
        assert _bits_equal(l_multi[0], single.forward(p2[-1]))
        # the own sequence: position kept, next logits those of an engine that never had slots
        assert multi.position() == 4
        got, ref = multi.forward(own[4]), other.forward(own[4])
        assert _bits_equal(got, ref), float(np.abs(got - ref).max())
    finally:
        multi.close()
        single.close()
        other.close()


def test_decode_sample_multi_equals_single_sequence(pkg):
    """Each int8 slot sampled by its own sampler inside the device-fed loop: the tokens of the single engine's lgh_decode_sample with the
    same config and draws."""
    cfg, model, multi, single = _engines(pkg, "test-dense", "Q4_K_M", 1)
    cfgs = [dict(PRESETS["engine_default"]), dict(PRESETS["server"]), dict(PRESETS["creative"]), dict(PRESETS["greedy"])]
    try:
        B, n_steps = 4, 12
        multi.batch_create(B)
        rng = np.random.default_rng(104)
        hists, firsts = [], []
        for s in range(B):
            h = [int(t) for t in rng.integers(0, cfg.vocab_size, size=3 + (7 * s) % 13)]
            multi.batch_prefill(s, h[:-1])
            multi.batch_set_sampler(s, **cfgs[s])
            hists.append(h[:-1])
            firsts.append(h[-1])
        unis = rng.random((n_steps, B), dtype=np.float32)
        got = multi.decode_sample_multi(list(range(B)), firsts, hists, n_steps, unis)
        want = np.zeros_like(got)
        for s in range(B):
            single.reset()
            for t in hists[s]:
                single.prefill_token(t)
            single.set_sampler(**cfgs[s])
            want[:, s] = single.decode_sample(firsts[s], hists[s], n_steps, unis[:, s])
        assert got.tolist() == want.tolist()
    finally:
        multi.close()
        single.close()


@pytest.mark.parametrize("kv", [1, 2, 3], ids=["int8", "fp8_e4m3", "fp8_e5m2"])
def test_slot_memory_and_context_state(pkg, kv):
    """The slots' caches are the byte ones (under a third of the f32 context's kv_bytes; no f32 slot caches), and the context still
    answers that its prompt pass is not batched."""
    cfg = pkg.make_config("test-dense-d128", max_seq_len=64)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    eng = pkg.HipGpuInference.from_model(model, 64, kv_cache_type=kv)
    f32 = pkg.HipGpuInference.from_model(model, 64)
    try:
        own, own32 = eng.stats()["kv_bytes"], f32.stats()["kv_bytes"]
        eng.batch_create(8)
        f32.batch_create(8)
        assert eng.stats()["kv_bytes"] * 3 < f32.stats()["kv_bytes"]
        # exactly: per slot, layer and kv head max_seq rows of head_dim bytes for K and for V, + a 4-byte scale each for int8
        rows = 8 * cfg.num_layers * cfg.num_kv_heads * 64
        assert eng.stats()["kv_bytes"] - own == 2 * rows * (cfg.head_dim + (4 if kv == 1 else 0))
        assert f32.stats()["kv_bytes"] - own32 == 2 * rows * cfg.head_dim * 4
        assert eng.prefill_is_batched() is False
        assert f32.prefill_is_batched() is True
    finally:
        eng.close()
        f32.close()


def test_errors_leave_the_slots_unchanged(pkg):
    cfg, model, multi, single = _engines(pkg, "test-dense", "Q4_K_M", 1, max_seq=8)
    try:
        with pytest.raises(pkg.BackendError) as ei:
            multi.forward_multi([0], [1])                                 # before lgh_batch_create
        assert ei.value.variant == "InvalidArgument"
        multi.batch_create(2)
        for bad_slots, toks in (([0, 0], [1, 2]), ([2], [1]), ([0, 1, 1], [1, 2, 3])):
            with pytest.raises(pkg.BackendError) as ei:
                multi.forward_multi(bad_slots, toks)
            assert ei.value.variant == "InvalidArgument"
        with pytest.raises(pkg.BackendError):
            multi.forward_multi([0], [cfg.vocab_size])
        got = []
        for t in range(8):
            got.append(multi.forward_multi([0], [t])[0][0].copy())
        with pytest.raises(pkg.BackendError) as ei:                       # the slot is full: nothing moves, the other slot is untouched
            multi.forward_multi([1, 0], [3, 4])
        assert ei.value.variant == "InvalidArgument"
        assert multi.batch_position(0) == 8 and multi.batch_position(1) == 0
        with pytest.raises(pkg.BackendError):
            multi.batch_prefill(1, list(range(9)))                        # a prompt longer than the slot
        assert multi.batch_position(1) == 0
        with pytest.raises(pkg.BackendError):
            multi.batch_create(3)                                         # already created with another size
        # the refused calls wrote nothing: slot 1 starts clean and slot 0's rows were what the single engine computes
        for t in range(8):
            assert _bits_equal(got[t], single.forward(t))
        single.reset()
        assert _bits_equal(multi.forward_multi([1], [5])[0][0], single.forward(5))
    finally:
        multi.close()
        single.close()
