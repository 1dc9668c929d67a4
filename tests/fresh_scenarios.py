"""What the children of tests/fresh_process.py run: plain functions `f(pkg, *args) -> json-able`, looked up by name.

Two families.  (i) The kernels an environment variable selects for the whole process (LGH_MVQB2_MIN, LGH_MVQB2_SEQ_GROUPS,
LGH_MOE_GROUP_MIN, LGH_PF_ATTN_VALU): the checks are those of test_gpu_matvec_multi.py, test_gpu_batch.py and test_gpu_attention.py,
called from here with the structure the variable forces — no reference and no tolerance is restated.  (ii) Cold captures (`cold_*`):
the path under test is the process's FIRST GPU work behind lgh_finalize / lgh_batch_create of its own context, then the same on a
FLAG_NO_GRAPH context (eager, never captured); a kernel first launched inside a capture is not replayed with the graph
(engine.hip: warm_kernels), which shows as other bits.  Arrays come back as SHA-256 digests of their bytes.

A parent may call the same functions in-process."""
import hashlib

import numpy as np


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _only_first_structure(gpu, before):
    after = gpu.mvqb_structures()
    moved = [int(a - b) for a, b in zip(after, before)]
    assert moved[0] > 0 and moved[1] == 0 and moved[2] == 0, "launches by structure (mvqb, mvqb2 split, mvqb2 seq): %s" % moved
    return moved


# ---------------------------------------------------------------------------------------------------------------------------------
# LGH_MVQB2_MIN=17: every multi-sequence launch takes mvqb_kernel<MASK, NB> (NB = 4, 8, 16) and mvqb_tail
# ---------------------------------------------------------------------------------------------------------------------------------
MVQB_SEQS = (2, 3, 4, 5, 8, 9, 16)                   # both ends of the buckets NB = 4 (2 .. 4), 8 (5 .. 8), 16 (9 .. 16)
MVQB_QKV = ((0, 0), (3, 1), (5, 2), (6, 3))          # (index in QKV_SHAPES, mix): one shape per mix, both head sizes, kv heads and widths


def mvqb_formats(pkg, tname):
    import test_gpu_matvec_multi as t
    gpu = pkg.hip_backend
    before = gpu.mvqb_structures()
    W = t.Worst()
    L = t.Linear(gpu, tname, 1024, 272, seed=100)
    for n_seq in MVQB_SEQS:
        L.check(W, n_seq, 16, t.MVQB, "mvqb %s store" % tname)
    W.done()
    return {"worst": W.w, "moved": _only_first_structure(gpu, before)}


def mvqb_epilogues(pkg):
    """The EPILOGUES table, the ragged output (1024, 130) and the CHAINS table."""
    import test_gpu_matvec_multi as t
    gpu = pkg.hip_backend
    before = gpu.mvqb_structures()
    W = t.Worst()
    for name, tname, k, n, role, xq_next, bias in t.EPILOGUES:
        L = t.Linear(gpu, tname, k, n, role=role, xq_next=xq_next, seed=500, norm=role == "swiglu", bias=bias)
        for n_seq, max_batch in ((3, 4), (16, 16)):
            L.check(W, n_seq, max_batch, t.MVQB, "mvqb %s %s" % (tname, name))
    L = t.Linear(gpu, "Q6_K", 1024, 130, seed=400)
    for n_seq in (5, 15, 16):
        L.check(W, n_seq, 16, t.MVQB, "mvqb Q6_K ragged store")
    W.done()
    for case in t.CHAINS:
        t.test_xq_chain(gpu, *case)
    return {"worst": W.w, "moved": _only_first_structure(gpu, before)}


def mvqb_qkv(pkg):
    import __graft_entry__ as graft
    import test_gpu_matvec_multi as t
    gpu = pkg.hip_backend
    before = gpu.mvqb_structures()
    for shape, mix in MVQB_QKV:
        t.fused_qkv_case(gpu, graft.load_oracle(), shape, mix, 0)
    return {"moved": _only_first_structure(gpu, before)}


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level: every sequence's logits bitwise those of the single-sequence engine, under LGH_MVQB2_MIN / LGH_MOE_GROUP_MIN
# ---------------------------------------------------------------------------------------------------------------------------------
def engine_bitwise(pkg, name, mix, B):
    """test_gpu_batch's bitwise test; -> the launches by structure it made and, by profiling class, the launches of one more step of B
    sequences (what test_step_launch_sequence_by_class reads)."""
    import test_gpu_batch as tb
    gpu = pkg.hip_backend
    before = gpu.mvqb_structures()
    tb.bitwise_logits_case(pkg, name, mix, B)
    moved = [int(a - b) for a, b in zip(gpu.mvqb_structures(), before)]
    cfg, model = tb._model(pkg, name, mix)
    eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len)
    try:
        eng.batch_create(B)
        eng.forward_multi(list(range(B)), [5 + s for s in range(B)])
        eng.set_profiling(True)
        eng.forward_multi(list(range(B)), [40 + s for s in range(B)], want_logits=False, greedy=True)
        eng.set_profiling(False)
        launches = {k: int(v["launches"]) for k, v in eng.stats()["kernels"].items()}
    finally:
        eng.close()
    return {"moved": moved, "launches": launches, "layers": int(cfg.num_layers)}


# ---------------------------------------------------------------------------------------------------------------------------------
# LGH_MVQB2_SEQ_GROUPS: 0 -> every launch on the SEQ grid; 1000000 -> every launch of more than one k-slice on the split grid
# ---------------------------------------------------------------------------------------------------------------------------------
def seq_groups(pkg, forced):
    """test_k_geometry's shapes for Q4_K and test_seq_grid_gate_up at k = 512.  The engine sizes the partial-sum buffer
    (batch_part_floats) with the rule mvqb_launch checks it with (mvqb_part_floats), so under the variable no launch may fall back to
    mvqb or be refused.  A launch of ONE k-slice (k = 256) is the SEQ grid by definition (mvqb2_seq_grid: `|| T == 1`)."""
    import test_gpu_matvec_multi as t
    assert forced in ("seq", "split")
    gpu = pkg.hip_backend
    W = t.Worst()
    for k, n in [(256, 48), (512, 64), (2816, 272), (5632, 96), (14336, 48)]:
        L = t.Linear(gpu, "Q4_K", k, n, seed=200)
        for n_seq in (3, 16):
            L.check(W, n_seq, 16, t.SEQ if forced == "seq" or k == 256 else t.SPLIT, "forced %s Q4_K k-slices" % forced)
    L = t.Linear(gpu, "Q4_K", 512, 10240, role="swiglu", xq_next=1, seed=300)
    for n_seq in (5, 16):
        L.check(W, n_seq, 16, t.SEQ if forced == "seq" else t.SPLIT, "forced %s Q4_K swiglu" % forced)
    W.done()
    return {"worst": W.w, "structures": gpu.mvqb_structures()}


# ---------------------------------------------------------------------------------------------------------------------------------
# LGH_PF_ATTN_VALU=1: the prompt pass's attention through attn_partial_kernel<D, G, 4, true>
# ---------------------------------------------------------------------------------------------------------------------------------
PF_KEEP = (5, 17, "normal")   # (pos0, m, kind) of the case whose output bits go to the parent, at (d, g) = (128, 4)


def prefill_attention(pkg, d, g):
    """test_gpu_attention.test_prefill's body for (d, g), with its attention_ref.prefill bound (f16 term included); -> the output bits
    of the case PF_KEEP at (128, 4)."""
    import test_gpu_attention as ta
    kept = ta.prefill_case(pkg.hip_backend, d, g, keep=PF_KEEP if (d, g) == (128, 4) else None)
    if kept is None:
        return {}
    bits = np.ascontiguousarray(kept, dtype=np.float32).view(np.uint32)
    return {"shape": list(bits.shape), "bits": [int(v) for v in bits.reshape(-1)]}


# ---------------------------------------------------------------------------------------------------------------------------------
# cold captures
# ---------------------------------------------------------------------------------------------------------------------------------
def _lens(B):
    return [3 + (5 * s) % 6 for s in range(B)]       # ragged histories of 3 .. 8 tokens


def _steps(eng, cfg, B, greedy):
    """All B sequences start together (the FIRST step has B sequences) and leave as their histories end."""
    import test_gpu_batch as tb
    lens = _lens(B)
    hist = [tb._history(cfg, s, lens[s]) for s in range(B)]
    logits_d, tokens = [], []
    for step in range(max(lens)):
        active = [s for s in range(B) if step < lens[s]]
        logits, nxt = eng.forward_multi(active, [hist[s][step] for s in active], want_logits=True, greedy=greedy)
        assert np.isfinite(logits).all()
        logits_d.append(_digest(logits))
        tokens.append(None if nxt is None else [int(v) for v in nxt])
    return {"logits": logits_d, "tokens": tokens}


def cold_forward_multi(pkg, name, mix, B, greedy, max_batch=0):
    """lgh_forward_multi with logits (greedy: mode 1, + arg-max; else mode 0) as the first GPU work behind its context's creation."""
    import test_gpu_batch as tb
    cfg, model = tb._model(pkg, name, mix)
    out = {}
    for key, flags in (("cold", 0), ("eager", pkg.hip_backend.FLAG_NO_GRAPH)):
        eng = pkg.HipGpuInference.from_model(model, cfg.max_seq_len, flags=flags)
        try:
            eng.batch_create(max_batch or B)
            out[key] = _steps(eng, cfg, B, greedy)
        finally:
            eng.close()
    return out


def cold_quantized_slots(pkg, name, mix, B, kv):
    """lgh_decode_greedy_multi, 8 steps of B sequences over int8 / TurboQuant slots, behind the slots' prompts (lgh_batch_prefill as in
    test_gpu_batch_kv8.py / test_turboquant_slots_bitwise: the prompt path's kernels and steps of one sequence, not the step of B
    sequences under test), then one more step with logits."""
    import test_gpu_batch as tb
    hb = pkg.hip_backend
    kvt = {"int8": hb.KV_INT8, "tq3": hb.KV_TQ3}[kv]
    cfg = pkg.make_config(name, max_seq_len=64)
    model = pkg.SynthModel(cfg, mix=mix)
    rng = np.random.default_rng(23)
    signs = np.where(rng.integers(0, 2, cfg.num_layers * cfg.num_kv_heads * 2 * cfg.head_dim) == 1, 1.0, -1.0).astype(np.float32) if kv == "tq3" else None
    lens = _lens(B)
    hist = [tb._history(cfg, 500 + s, lens[s]) for s in range(B)]
    out = {}
    for key, flags in (("cold", 0), ("eager", hb.FLAG_NO_GRAPH)):
        eng = pkg.HipGpuInference.from_model(model, 64, flags=flags, kv_cache_type=kvt, kv_rotation_signs=signs)
        try:
            eng.batch_create(B)
            for s in range(B):
                eng.batch_prefill(s, hist[s][:-1])
            toks = eng.decode_greedy_multi(list(range(B)), [h[-1] for h in hist], 8)
            logits, nxt = eng.forward_multi(list(range(B)), [int(t) for t in toks[-1]], want_logits=True, greedy=True)
            assert np.isfinite(logits).all()
            out[key] = {"tokens": toks.tolist() + [[int(v) for v in nxt]], "logits": [_digest(logits)]}
        finally:
            eng.close()
    return out


def cold_tensor_parallel(pkg):
    """HipTensorParallel over 2 ranks: a prompt through prefill_token, decode_greedy(3, 16), then one token's logits."""
    import test_gpu_batch as tb
    cfg = pkg.make_config("test-dense", max_seq_len=64)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    prompt = tb._history(cfg, 900, 9)
    out = {}
    for key, flags in (("cold", 0), ("eager", pkg.hip_backend.FLAG_NO_GRAPH)):
        tp = pkg.HipTensorParallel.from_model(model, 64, 2, flags=flags)
        try:
            for t in prompt:
                tp.prefill_token(t)
            toks = tp.decode_greedy(3, 16)
            logits = tp.forward(int(toks[-1]))
            assert np.isfinite(logits).all()
            out[key] = {"tokens": [int(v) for v in toks], "logits": [_digest(logits)], "graph_nodes": int(tp.graph_nodes())}
        finally:
            tp.close()
    assert out["cold"].pop("graph_nodes") > 0 and out["eager"].pop("graph_nodes") == 0
    return out


# ---- cold captures of BOTH decode-attention graphs (tests/switch_scenarios.py: the head form up to S rows, splits + merge beyond)
def cold_switch_single(pkg):
    """attn_direct=1 (the switch at 64 rows): 60 tokens through prefill_token, decode_greedy over 10 steps (positions 60 .. 69: the
    head graph is captured cold, then the split graph, inside one call), then one forward (the MODE_FORWARD split graph)."""
    import switch_scenarios as sw
    hb = pkg.hip_backend
    name, mix = sw.MAIN
    cfg = pkg.make_config(name, max_seq_len=sw.MAX_SEQ)
    model = pkg.SynthModel(cfg, mix=mix)
    V = cfg.vocab_size
    out = {}
    for key, flags in (("cold", 0), ("eager", hb.FLAG_NO_GRAPH)):
        eng = pkg.HipGpuInference.from_model(model, sw.MAX_SEQ, flags=flags | hb.FLAG_EXACT_PREFILL, attn_direct=sw.ATTN_DIRECT)
        try:
            (toks, logits), _ = sw.run(eng, sw.SCENARIOS["cold_switch"][1], V)
            assert np.isfinite(logits).all() and eng.position() == 71
            out[key] = {"tokens": toks, "logits": [_digest(logits)]}
        finally:
            eng.close()
    return out


def cold_split_first(pkg):
    """A default engine (the switch at 256 rows): forward_batch of 257 tokens, then decode_greedy over 4 steps — the split graph is
    captured cold and the head graph never."""
    import switch_scenarios as sw
    hb = pkg.hip_backend
    name, mix = sw.MAIN
    cfg = pkg.make_config(name, max_seq_len=sw.DEFAULT_MAX_SEQ)
    model = pkg.SynthModel(cfg, mix=mix)
    V = cfg.vocab_size
    out = {}
    for key, flags in (("cold", 0), ("eager", hb.FLAG_NO_GRAPH)):
        eng = pkg.HipGpuInference.from_model(model, sw.DEFAULT_MAX_SEQ, flags=flags)
        try:
            (toks,), _ = sw.run(eng, sw.DEFAULT_SCENARIOS["cold_split_first"][1], V, max_seq=sw.DEFAULT_MAX_SEQ)
            logits = eng.forward(toks[-1])                        # (what the loop left, read back through one more step)
            assert np.isfinite(logits).all() and eng.position() == 262
            out[key] = {"tokens": toks, "logits": [_digest(logits)]}
        finally:
            eng.close()
    return out


def cold_tensor_parallel_switch(pkg):
    """HipTensorParallel over 2 ranks with the switch at 64 rows (flags = 1 << 16): 60 prompt tokens, decode_greedy(.., 10) across the
    switch, then one token's logits."""
    import switch_scenarios as sw
    hb = pkg.hip_backend
    name, mix = sw.MAIN
    cfg = pkg.make_config(name, max_seq_len=sw.MAX_SEQ, intermediate_size=2048, num_kv_heads=4)   # test_gpu_tp.py's D128
    model = pkg.SynthModel(cfg, mix=mix)
    V = cfg.vocab_size
    out = {}
    for key, flags in (("cold", 0), ("eager", hb.FLAG_NO_GRAPH)):
        tp = pkg.HipTensorParallel.from_model(model, sw.MAX_SEQ, 2, flags=flags | sw.TP_FLAGS)
        try:
            (toks, logits), _ = sw.run(tp, sw.SCENARIOS["cold_switch"][1], V)
            assert np.isfinite(logits).all() and tp.position() == 71
            out[key] = {"tokens": toks, "logits": [_digest(logits)], "graph_nodes": int(tp.graph_nodes())}
        finally:
            tp.close()
    assert out["cold"].pop("graph_nodes") > 0 and out["eager"].pop("graph_nodes") == 0
    return out
