"""The device prompt cache on the GPU (csrc/kv_prefix.hip; include/llama_gguf_hip.h lgh_prefix_*): a sequence's KV rows saved into
one packed device buffer and restored by copying — PrefixSharing::save_prefix / try_restore (src/model/cache.rs:269-326) on the device.

  kernel     kv_prefix_copy_kernel through lgh_op_kv_prefix_copy against the numpy pack / unpack (tests/kv_prefix_ref.py), byte for byte
  engine     a restore is `reset` + the prompt: the next step's logits are BIT-IDENTICAL to the same step on the cache the prefix was
             saved from, for the own sequence of every cache format and between slots and the own sequence
Everything compared is a copy of bytes or the same kernels over the same bytes, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import kv_prefix_ref as ref

pytestmark = pytest.mark.gpu

KV_NAMES = {0: "f32", 1: "int8", 2: "fp8_e4m3", 3: "fp8_e5m2", 4: "tq2", 5: "tq3", 6: "tq2-qjl", 7: "tq3-qjl"}
PROMPT = 40


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _tokens(cfg, seed, n):
    return [int(t) for t in np.random.default_rng(7000 + seed).integers(0, cfg.vocab_size, size=n)]


def _argmax_last(logits):
    return int(np.flatnonzero(logits == logits.max())[-1])


def _same_caches(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for la, lb in zip(a, b) for x, y in zip(la, lb))


# ---- 1. the kernel ----
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("kv", range(8), ids=[KV_NAMES[k] for k in range(8)])
def test_copy_kernel_packs_and_unpacks_byte_for_byte(pkg, kv, d):
    """3 layers x 3 slots x 2 kv heads, max_seq 37 (odd: 12-, 20- and 24-byte positions leave segments that are only 4-byte aligned),
    random bytes everywhere, one launch per call.  Save: slot 1's rows [0, n) equal the numpy pack.  Restore: other random rows into
    slot 2 of a canary-filled cache; rows [0, n_rows) of slot 2 match and every other byte of every slot and layer keeps its canary
    (the whole cache is compared with the numpy unpack).  Two runs give the same bytes."""
    hb = pkg.hip_backend
    n_layers, n_slots, n_kv, max_seq = 3, 3, 2, 37
    lay = hb.kv_cache_layout(kv, n_kv, max_seq, d)
    rng = np.random.default_rng(100 * kv + d)
    src = ref.random_caches(rng, lay, n_layers, n_slots, n_kv, max_seq)
    canary = ref.random_caches(rng, lay, n_layers, n_slots, n_kv, max_seq, fill=0xA5)
    for n in (1, 5, 36, 37):
        want = ref.pack(src, 1, n)
        assert want.size == ref.packed_size(lay, n_layers, n_kv, n)
        got = hb.op_kv_prefix_copy(kv, src, 1, n, d)
        assert np.array_equal(got, want), (KV_NAMES[kv], d, n, int((got != want).sum()))
        assert np.array_equal(hb.op_kv_prefix_copy(kv, src, 1, n, d), got)
        for n_rows in (n, n - 3):
            if n_rows < 1:
                continue
            packed = rng.integers(0, 256, size=ref.packed_size(lay, n_layers, n_kv, n_rows), dtype=np.uint8)
            want_c = ref.unpack(canary, 2, n_rows, packed)
            got_c = hb.op_kv_prefix_copy(kv, canary, 2, n_rows, d, packed=packed)
            assert _same_caches(got_c, want_c), (KV_NAMES[kv], d, n_rows)
            for layer in got_c:                 # (what the comparison above implies, said directly)
                for t in layer:
                    if t is not None:
                        assert (t[:2] == 0xA5).all() and (t[2, :, n_rows:] == 0xA5).all()
            assert _same_caches(hb.op_kv_prefix_copy(kv, canary, 2, n_rows, d, packed=packed), got_c)


def test_copy_entry_point_refuses_bad_arguments(pkg):
    hb = pkg.hip_backend
    lay = hb.kv_cache_layout(hb.KV_INT8, 2, 8, 64)
    caches = ref.random_caches(np.random.default_rng(0), lay, 1, 2, 2, 8)
    for slot, n in ((2, 4), (0, 0), (0, 9)):
        with pytest.raises(pkg.BackendError) as ei:
            hb.op_kv_prefix_copy(hb.KV_INT8, caches, slot, n, 64, packed=np.zeros(ref.packed_size(lay, 1, 2, n), np.uint8))
        assert ei.value.variant == "InvalidArgument"


# ---- 2. the own sequence, every cache format ----
def _feed_prompt(eng, prompt):
    if eng.prefill_is_batched():
        eng.forward_batch(prompt)
    else:
        for t in prompt:
            eng.prefill_token(t)


OWN_CASES = [("test-dense", kv) for kv in range(8)] + [("test-dense-d128", 5), ("test-dense-d128", 7), ("test-dense-d128", 1), ("test-moe", 0)]


@pytest.mark.parametrize("name,kv", OWN_CASES, ids=[f"{n}-{KV_NAMES[k]}" for n, k in OWN_CASES])
def test_restore_is_reset_plus_the_prompt_on_the_own_sequence(pkg, name, kv):
    cfg = pkg.make_config(name, max_seq_len=64)
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q4_K_M"), 64, kv_cache_type=kv)
    try:
        prompt, t = _tokens(cfg, kv, PROMPT), 11
        _feed_prompt(eng, prompt)
        assert eng.position() == PROMPT
        p = eng.prefix_save()
        assert p.n_rows == PROMPT and eng.position() == PROMPT          # a save does not move the source
        want = eng.forward(t)
        eng.kv_truncate(PROMPT)
        host_tokens, tok = [], t                                           # the host loop from the same point
        for _ in range(4):
            tok = _argmax_last(eng.forward(tok))
            host_tokens.append(tok)
        eng.kv_truncate(25)
        want25 = eng.forward(t)                                            # rows [0, 25) of the original cache, then the same step

        eng.reset()
        eng.prefix_restore(p)
        assert eng.position() == PROMPT
        got = eng.forward(t)
        assert _bits_equal(got, want), float(np.abs(got - want).max())
        assert eng.position() == PROMPT + 1
        # the device's own position word: the graph-fed greedy loop reads it, not the host's
        eng.prefix_restore(p)
        assert eng.decode_greedy(t, 4).tolist() == host_tokens
        assert eng.position() == PROMPT + 4

        # fewer rows: a prefix saved with 25, and 25 rows out of the prefix of 40
        eng.prefix_restore(p)
        p25 = eng.prefix_save(25)
        assert p25.n_rows == 25 and p25.nbytes * PROMPT == p.nbytes * 25
        for prefix, n in ((p25, None), (p, 25)):
            eng.reset()
            eng.prefix_restore(prefix, n=n)
            assert eng.position() == 25
            got25 = eng.forward(t)
            assert _bits_equal(got25, want25), (n, float(np.abs(got25 - want25).max()))
        p.free()
        p25.free()
        assert eng.prefix_total_bytes() == 0
    finally:
        eng.close()


def test_a_stage_context_saves_and_restores_its_own_layers(pkg):
    """The first stage of a 3-layer model owning layers [0, 2): its prefix holds two layers, and a restore puts the stage where it was."""
    hb = pkg.hip_backend
    cfg = pkg.make_config("test-dense-d128", max_seq_len=32)
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q4_K_M"), 32, layer_range=(0, 2), kv_cache_type=hb.KV_INT8)
    try:
        for tok in _tokens(cfg, 50, 6):
            eng.stage_forward(tok)
        p = eng.prefix_save()
        info = p.info()
        lay = hb.kv_cache_layout(hb.KV_INT8, cfg.num_kv_heads, 32, cfg.head_dim)
        assert (info.layer_begin, info.layer_end, info.n_rows, info.kv_cache_type) == (0, 2, 6, hb.KV_INT8)
        assert info.bytes == 2 * cfg.num_kv_heads * 6 * (2 * (lay.row_bytes + lay.scale_bytes) + lay.qjl_bytes)
        eng.stage_forward(9)
        want = eng.read_hidden()
        eng.reset()
        for tok in _tokens(cfg, 51, 3):           # other rows in the way
            eng.stage_forward(tok)
        eng.prefix_restore(p)
        assert eng.position() == 6
        eng.stage_forward(9)
        assert _bits_equal(eng.read_hidden(), want)
    finally:
        eng.close()


# ---- 3. slots ----
@pytest.mark.parametrize("kv", [0, 1, 5, 7], ids=[KV_NAMES[k] for k in (0, 1, 5, 7)])
def test_prefixes_move_between_slots_and_the_own_sequence(pkg, kv):
    """Every restore here goes into a target that already holds other rows and a non-zero position.  attn_direct=255 as in
    tests/test_gpu_batch.py: the f32 single-sequence step then runs the attention structure the multi-sequence step always runs."""
    cfg = pkg.make_config("test-dense", max_seq_len=64)
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q4_K_M"), 64, kv_cache_type=kv, attn_direct=255)
    try:
        eng.batch_create(8)
        a, b, t = _tokens(cfg, 1, 20), _tokens(cfg, 2, 7), 5
        # slot to slot
        eng.batch_prefill(4, a)
        eng.batch_prefill(1, b)
        p = eng.prefix_save(slot=4)
        assert p.n_rows == 20 and eng.batch_position(4) == 20
        eng.prefix_restore(p, slot=1)
        assert eng.batch_position(1) == 20
        logits, _ = eng.forward_multi([4, 1], [t, t])
        assert _bits_equal(logits[0], logits[1]), float(np.abs(logits[0] - logits[1]).max())
        p.free()
        # own sequence to slot
        _feed_prompt(eng, a)
        eng.batch_prefill(2, b)
        p = eng.prefix_save()
        eng.prefix_restore(p, slot=2)
        assert eng.batch_position(2) == 20 and eng.position() == 20
        want = eng.forward(t)
        got, _ = eng.forward_multi([2], [t])
        assert _bits_equal(got[0], want), float(np.abs(got[0] - want).max())
        p.free()
        # slot to own sequence (the own sequence is at 21, slot 5 gets another prompt)
        c = _tokens(cfg, 3, 13)
        eng.batch_prefill(5, c)
        p = eng.prefix_save(slot=5)
        eng.prefix_restore(p)
        assert eng.position() == 13 and eng.batch_position(5) == 13
        want = eng.forward(t)
        got, _ = eng.forward_multi([5], [t])
        assert _bits_equal(got[0], want), float(np.abs(got[0] - want).max())
        p.free()
        assert eng.prefix_total_bytes() == 0
    finally:
        eng.close()


@pytest.mark.parametrize("kv", [0, 1, 5, 7], ids=[KV_NAMES[k] for k in (0, 1, 5, 7)])
def test_one_prefix_forks_into_four_slots(pkg, kv):
    cfg = pkg.make_config("test-dense", max_seq_len=64)
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q4_K_M"), 64, kv_cache_type=kv)
    try:
        eng.batch_create(8)
        prompt = _tokens(cfg, 4, 24)
        for s in (4, 5, 6, 7):
            eng.batch_prefill(s, prompt)
        for s in (0, 1, 2, 3):
            eng.batch_prefill(s, _tokens(cfg, 10 + s, 3 + s))               # rows and positions in the way
        p = eng.prefix_save(slot=4)
        for s in (0, 1, 2, 3):
            eng.prefix_restore(p, slot=s)
            assert eng.batch_position(s) == 24
        toks = [3, 99, 500, 1023]
        for step in range(2):
            got, nxt = eng.forward_multi([0, 1, 2, 3], toks, greedy=True)
            want, nxt_w = eng.forward_multi([4, 5, 6, 7], toks, greedy=True)
            for i in range(4):
                assert _bits_equal(got[i], want[i]), (step, i, float(np.abs(got[i] - want[i]).max()))
            assert nxt.tolist() == nxt_w.tolist()
            toks = [int(x) for x in nxt]
        p.free()
    finally:
        eng.close()


# ---- 4. accounting and refusals ----
def _invalid(pkg, fn, *args, **kw):
    with pytest.raises(pkg.BackendError) as ei:
        fn(*args, **kw)
    assert ei.value.variant == "InvalidArgument", ei.value


@pytest.mark.parametrize("kv", [0, 1, 7], ids=["f32", "int8", "tq3-qjl"])
def test_prefix_bytes_follow_the_layout_and_stats_stay(pkg, kv):
    hb = pkg.hip_backend
    cfg = pkg.make_config("test-dense", max_seq_len=64)
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q4_K_M"), 64, kv_cache_type=kv)
    try:
        lay = hb.kv_cache_layout(kv, cfg.num_kv_heads, 64, cfg.head_dim)
        per_pos = cfg.num_kv_heads * (2 * (lay.row_bytes + lay.scale_bytes) + lay.qjl_bytes)
        for tok in _tokens(cfg, 5, 9):
            eng.prefill_token(tok)
        before = eng.stats()
        p9, p4 = eng.prefix_save(), eng.prefix_save(4)
        after = eng.stats()
        assert (after["kv_bytes"], after["scratch_bytes"]) == (before["kv_bytes"], before["scratch_bytes"])
        assert p9.nbytes == 9 * cfg.num_layers * per_pos and p4.nbytes == 4 * cfg.num_layers * per_pos
        assert p9.info().bytes == p9.nbytes and p9.info().struct_size == C.sizeof(hb.PrefixInfo)
        assert eng.prefix_total_bytes() == p9.nbytes + p4.nbytes
        p9.free()
        assert eng.prefix_total_bytes() == p4.nbytes
        p4.free()
        assert eng.prefix_total_bytes() == 0
    finally:
        eng.close()


def test_refusals_answer_invalid_argument_and_change_nothing(pkg):
    hb = pkg.hip_backend
    L = hb.load_library()
    cfg = pkg.make_config("test-dense", max_seq_len=32)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    eng = pkg.HipGpuInference.from_model(model, 32, kv_cache_type=hb.KV_INT8)
    other = pkg.HipGpuInference.from_model(model, 32, kv_cache_type=hb.KV_INT8)
    try:
        _invalid(pkg, eng.prefix_save)                                   # nothing to save
        for tok in _tokens(cfg, 6, 6):
            eng.prefill_token(tok)
            other.prefill_token(tok)
        _invalid(pkg, eng.prefix_save, slot=0)                           # any slot before lgh_batch_create
        p = eng.prefix_save()
        _invalid(pkg, eng.prefix_restore, p, slot=0)
        eng.batch_create(2)
        eng.batch_prefill(1, _tokens(cfg, 7, 3))
        foreign = other.prefix_save()
        h = C.c_void_p()
        cases = [
            lambda: eng.prefix_save(slot=2),                             # slot >= max_batch
            lambda: eng.prefix_save(slot=-2),
            lambda: eng.prefix_save(slot=0),                             # slot 0 is at position 0
            lambda: eng.prefix_save(7),                                  # beyond the position
            lambda: eng.prefix_save(4, slot=1),
            lambda: eng.prefix_restore(p, slot=2),
            lambda: eng.prefix_restore(p, n=7),                          # beyond the prefix's rows
            lambda: eng.prefix_restore(foreign),                         # another context's handle
            lambda: eng.prefix_restore(foreign, slot=1),
            lambda: eng._call(L.lgh_prefix_free(eng._h, foreign._h)),
            lambda: eng._call(L.lgh_prefix_get_info(eng._h, foreign._h, C.byref(hb.PrefixInfo()))),
            lambda: eng._call(L.lgh_prefix_export(eng._h, foreign._h, None, 0, C.byref(C.c_size_t()))),
            lambda: eng._call(L.lgh_prefix_save(eng._h, -1, 0, None)),   # NULL pointers
            lambda: eng._call(L.lgh_prefix_restore(eng._h, None, -1, 0)),
            lambda: eng._call(L.lgh_prefix_free(eng._h, None)),
            lambda: eng._call(L.lgh_prefix_get_info(eng._h, p._h, None)),
            lambda: eng._call(L.lgh_prefix_export(eng._h, p._h, None, 0, None)),
            lambda: eng._call(L.lgh_prefix_export(eng._h, p._h, C.byref(h), 8, None)),   # dst too small
            lambda: eng._call(L.lgh_prefix_import(eng._h, None, 64, C.byref(h))),
        ]
        total = eng.prefix_total_bytes()
        for i, case in enumerate(cases):
            _invalid(pkg, case)
            assert (eng.position(), eng.batch_position(0), eng.batch_position(1)) == (6, 0, 3), i
            assert eng.prefix_total_bytes() == total, i
        assert L.lgh_prefix_save(None, -1, 0, C.byref(h)) == 6 and L.lgh_prefix_total_bytes(None) == 0
        want = eng.forward(3)
        eng.prefix_restore(p)
        assert _bits_equal(eng.forward(3), want)                         # the refused calls left the rows alone too
        p.free()
        for case in (lambda: eng.prefix_restore(p), p.free, p.info, p.to_bytes):   # a freed handle
            _invalid(pkg, case)
        assert eng.position() == 7 and eng.prefix_total_bytes() == 0
        foreign.free()
    finally:
        eng.close()
        other.close()


# ---- 5. export / import ----
@pytest.mark.parametrize("kv", [0, 7], ids=["f32", "tq3-qjl"])
def test_export_import_round_trip_and_header_checks(pkg, kv):
    cfg = pkg.make_config("test-dense", max_seq_len=64)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    eng = pkg.HipGpuInference.from_model(model, 64, kv_cache_type=kv)
    other = pkg.HipGpuInference.from_model(model, 64, kv_cache_type=kv)     # same weights, same (stand-in) signs and QJL matrices
    try:
        _feed_prompt(eng, _tokens(cfg, 8, 17))
        p = eng.prefix_save()
        blob = p.to_bytes()
        assert len(blob) == 40 + p.nbytes
        head = np.frombuffer(blob[:32], dtype=np.uint32)
        assert head[2:].tolist() == [kv, cfg.num_kv_heads, cfg.head_dim, 0, cfg.num_layers, 17]
        assert int(np.frombuffer(blob[32:40], dtype=np.uint64)[0]) == p.nbytes
        want = eng.forward(21)
        for tok in _tokens(cfg, 9, 5):
            other.prefill_token(tok)
        q = other.prefix_from_bytes(blob)
        assert (q.n_rows, q.nbytes) == (17, p.nbytes) and other.prefix_total_bytes() == p.nbytes
        assert q.to_bytes() == blob
        other.prefix_restore(q)
        assert other.position() == 17
        assert _bits_equal(other.forward(21), want)

        def patched(word, value):
            b = bytearray(blob)
            b[4 * word:4 * word + 4] = int(value).to_bytes(4, "little")
            return bytes(b)
        bad = [blob[:-1], blob[:39], blob[:8], blob + b"\0", patched(2, (kv + 1) % 8), patched(4, 192 - cfg.head_dim), patched(0, 0),
               patched(1, 2), patched(3, cfg.num_kv_heads + 1), patched(5, 1), patched(6, 1), patched(7, 16), patched(7, 0), patched(7, 65)]
        for i, b in enumerate(bad):
            _invalid(pkg, other.prefix_from_bytes, b)
            assert other.prefix_total_bytes() == p.nbytes and other.position() == 18, i
        other.close()                                                    # frees q with the context
        p.free()
    finally:
        eng.close()
        other.close()
