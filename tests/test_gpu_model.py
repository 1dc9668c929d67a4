"""End-to-end parity on the MI355X: the engine behind the C ABI (through the GpuInference / GpuModelWrapper
mirror) against the CPU oracle's LlamaModel::forward on identical synthetic weights.

Stated tolerance: final logits max|d| <= 2e-3 * max|logit| + 2e-3 (everything is f32; only the
summation order and the device exp differ).  Greedy tokens must be IDENTICAL whenever the oracle's top-1/top-2 gap
exceeds 4x the measured logit error; the test reports min_gap next to max|d|."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _pair(pkg, orc, name, mix, max_seq=64, **kw):
    cfg = pkg.make_config(name, max_seq_len=max_seq, **kw)
    model = pkg.SynthModel(cfg, mix=mix)
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    eng = pkg.HipGpuInference.from_model(model, max_seq)
    return cfg, ref, eng


def _tol(want):
    return 2e-3 * float(np.abs(want).max()) + 2e-3


CASES = [("test-dense", "Q4_K_M"), ("test-dense", "Q8_0"), ("test-dense", "Q4_0"), ("test-dense", "Q5_K_M"),
         ("test-dense", "Q6_K"), ("test-dense-d128", "Q4_K_M"), ("test-dense", "Q5_0"), ("test-moe", "Q5_K_M"),
         ("test-moe", "Q4_K_M")]


@pytest.mark.parametrize("name,mix", CASES)
def test_logits_and_greedy_tokens_match_oracle(pkg, orc, name, mix):
    cfg, ref, eng = _pair(pkg, orc, name, mix)
    wrap, ctx = pkg.GpuModelWrapper(eng), pkg.InferenceContext()
    prompt = [i % cfg.vocab_size for i in range(3, 3 + 9)]
    got, want = wrap.forward(prompt, ctx), ref.forward(prompt)          # prefill_token x8 + forward
    assert eng.position() == len(prompt) == ref.position
    errs, gaps = [float(np.abs(got - want).max())], []
    assert errs[0] <= _tol(want)
    tok_g, tok_r = orc.argmax_last(got), orc.argmax_last(want)
    for _ in range(24):                                                   # greedy decode, bench protocol
        srt = np.sort(want)
        gaps.append(float(srt[-1] - srt[-2]))
        if gaps[-1] > 4 * errs[-1]:
            assert tok_g == tok_r, f"greedy token diverged with gap {gaps[-1]:.3e} vs err {errs[-1]:.3e}"
        tok = tok_r                                                       # feed both the oracle's token
        got, want = wrap.forward([tok], ctx), ref.forward([tok])
        errs.append(float(np.abs(got - want).max()))
        assert errs[-1] <= _tol(want)
        tok_g, tok_r = orc.argmax_last(got), orc.argmax_last(want)
    print(f"{name}/{mix}: max|dlogit|={max(errs):.3e} tol={_tol(want):.3e} min_gap={min(gaps):.3e}")
    eng.close()


def test_hidden_state_after_last_layer(pkg, orc):
    cfg, ref, eng = _pair(pkg, orc, "test-dense-d128", "Q4_K_M")
    toks = [5, 900, 31, 7]
    for t in toks[:-1]:
        eng.prefill_token(t)
    eng.forward(toks[-1])
    ref.forward(toks)
    want, got = ref.last_hidden(), eng.read_hidden()
    assert np.abs(got - want).max() <= 1e-4 * (1 + np.abs(want).max())
    eng.close()


def test_device_argmax_and_greedy_loop_match_host_argmax(pkg, orc):
    """lgh_forward_argmax / lgh_decode_greedy (token fed back on device) == host arg-max over lgh_forward logits."""
    cfg, ref, eng = _pair(pkg, orc, "test-dense", "Q4_K_M", max_seq=96)
    prompt = list(range(10, 18))
    for t in prompt:
        eng.prefill_token(t)
    host = []
    tok = prompt[-1]
    for _ in range(20):
        tok = orc.argmax_last(eng.forward(tok))
        host.append(tok)
    eng.reset()
    assert eng.position() == 0
    for t in prompt:
        eng.prefill_token(t)
    dev = eng.decode_greedy(prompt[-1], 20).tolist()
    assert dev == host
    eng.reset()
    for t in prompt:
        eng.prefill_token(t)
    one = []
    tok = prompt[-1]
    for _ in range(20):
        tok = eng.forward_argmax(tok)
        one.append(tok)
    assert one == host
    eng.close()


def test_reset_rule_and_errors(pkg, orc):
    cfg, ref, eng = _pair(pkg, orc, "test-dense", "Q4_K", max_seq=8)
    wrap, ctx = pkg.GpuModelWrapper(eng), pkg.InferenceContext()
    a = wrap.forward([1, 2, 3], ctx)
    ctx2 = pkg.InferenceContext()                       # ctx.position == 0 and gpu.position() > 0 -> reset (mod.rs:334-336)
    b = wrap.forward([1, 2, 3], ctx2)
    assert np.array_equal(a, b) and eng.position() == 3
    with pytest.raises(ValueError):
        wrap.forward([], ctx2)                          # "No tokens to process" (mod.rs:338-342)
    with pytest.raises(pkg.BackendError) as ei:
        eng.forward(cfg.vocab_size)                     # token id exceeds vocab (llama.rs:296-302)
    assert ei.value.variant == "InvalidArgument"
    for t in range(5):
        eng.prefill_token(t)
    assert eng.position() == 8
    with pytest.raises(pkg.BackendError) as ei:
        eng.prefill_token(1)                            # pos >= max_seq_len: InvalidArgument, not an OOB write (quirk Q5)
    assert ei.value.variant == "InvalidArgument" and eng.position() == 8
    eng.close()


def test_graph_and_eager_paths_agree_bitwise(pkg, orc):
    cfg = pkg.make_config("test-dense", max_seq_len=32)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    outs = []
    for flags in (0, pkg.hip_backend.FLAG_NO_GRAPH):
        eng = pkg.HipGpuInference.from_model(model, 32, flags=flags)
        for t in (4, 5, 6):
            eng.prefill_token(t)
        outs.append(eng.forward(7))
        eng.close()
    assert np.array_equal(outs[0], outs[1])


def test_tied_output_and_bias(pkg, orc):
    cfg, ref, eng = _pair(pkg, orc, "test-dense", "Q8_0", tie_embeddings=True)
    got, want = eng.forward(9), ref.forward([9])
    assert np.abs(got - want).max() <= _tol(want)
    eng.close()
    cfg = pkg.make_config("test-dense", max_seq_len=16)
    model = pkg.SynthModel(cfg, mix="Q4_K_M", with_bias=True)
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    eng = pkg.HipGpuInference.from_model(model, 16)
    for t in (1, 2):
        eng.prefill_token(t)
    got, want = eng.forward(3), ref.forward([1, 2, 3])
    assert np.abs(got - want).max() <= _tol(want)
    eng.close()


def test_pipeline_stages_reproduce_single_stage(pkg, orc):
    """Two stage contexts on one GPU with the hidden vector handed over == one full context (bitwise)."""
    import ctypes as C
    cfg = pkg.make_config("test-dense-d128", max_seq_len=16)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    full = pkg.HipGpuInference.from_model(model, 16)
    s0 = pkg.HipGpuInference.from_model(model, 16, layer_range=(0, 2))
    s1 = pkg.HipGpuInference.from_model(model, 16, layer_range=(2, 3))
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for tok in (3, 4, 5):
        want = full.forward(tok)
        s0.stage_forward(tok)
        s0.synchronize()
        assert hip.hipMemcpy(s1.stage_hidden_ptr(), s0.stage_hidden_ptr(), cfg.hidden_size * 4, 3) == 0  # D2D
        assert hip.hipDeviceSynchronize() == 0   # a device-to-device hipMemcpy may return before it is done
        got = s1.stage_forward(0, want_logits=True)
        assert np.array_equal(got, want)
    for e in (full, s0, s1):
        e.close()


def test_profiling_stats(pkg, orc):
    cfg, ref, eng = _pair(pkg, orc, "test-dense", "Q4_K_M")
    eng.prefill_token(1)
    eng.set_profiling(True)
    eng.forward(2)
    eng.set_profiling(False)
    st = eng.stats()
    k = st["kernels"]
    # one fused QKV launch per layer when its three matrices share a kernel family (here: all on the matrix cores, Q4_K + Q6_K
    # in the mixed instantiation); two when they do not (a family per launch)
    assert cfg.num_layers <= k["qkv"]["launches"] <= 2 * cfg.num_layers and k["gate_up"]["launches"] == cfg.num_layers
    assert k["output"]["launches"] == 1 and all(v["time_us"] > 0 for v in k.values())
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    assert abs(st["step_alg_bytes"] - model.step_alg_bytes(eng.position() + 1)) <= 0.01 * st["step_alg_bytes"]
    eng.close()


def test_cpp_host_mirror(pkg, orc, tmp_path):
    """The C++ mirror of GpuInference / GpuModelWrapper (llama-gguf_amd/host/hip_gpu_inference.hpp), compiled with g++
    against the C-ABI libraries, gives the oracle's logits and greedy tokens."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "llama-gguf_amd", "lib")
    exe = str(tmp_path / "host_mirror_test")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "host_mirror_test.cpp"), "-o", exe,
                    "-L" + lib, "-lllama_gguf_hip", "-lllama_gguf_synth", "-Wl,-rpath," + lib], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    cfg = pkg.make_config("test-dense", max_seq_len=32)
    model = pkg.SynthModel(cfg, mix="Q4_K")
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    toks = [3, 17, 255, 9, 700]
    for step in range(4):
        head, vals = out[step].split(":")
        got = np.array([float.fromhex(v) for v in vals.split()], dtype=np.float32)
        want = ref.forward(toks)
        assert np.abs(got - want).max() <= _tol(want)
        assert int(head.split()[-1]) == orc.argmax_last(want) == orc.argmax_last(got)
        toks = [orc.argmax_last(want)]
    assert out[4] == "error-variant InvalidArgument"
    # BatchedEngine's device side through the mirror: slot 1 replays the single-sequence history token by token -> the step-0 logits
    # (to rounding), and its device-fed greedy tokens
    head, vals = out[5].split(":")
    got = np.array([float.fromhex(v) for v in vals.split()], dtype=np.float32)
    first = np.array([float.fromhex(v) for v in out[0].split(":")[1].split()], dtype=np.float32)
    assert head.split()[:4] == ["multi", "pos", "5", "3"]
    assert np.abs(got - first).max() <= 1e-4 * float(np.abs(first).max())
    assert int(head.split()[5]) == orc.argmax_last(got)
    greedy = [int(v) for v in out[6].split()[1:]]
    assert greedy[0] == int(out[1].split(":")[0].split()[-1]) and len(greedy) == 3


def test_full_size_llama3_8b_q4_k_m_matches_oracle(pkg, orc):
    """BASELINE.json's headline configuration at FULL size (32 layers, hidden 4096, ffn 14336, vocab 128256, Q4_K_M mix
    with its Q6_K matrices): logits of a short prompt and of three greedy steps against the CPU oracle (~0.3 s per token
    there), greedy tokens identical where the oracle's top-1/top-2 gap exceeds the measured error; then a size-independent
    property at the full decode length: 64 more device-fed greedy steps are deterministic run to run."""
    cfg = pkg.make_config("llama-3-8b", max_seq_len=128)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    ref = orc.Model(cfg.as_dict())
    eng = None
    try:
        for nm, t, ne, data in model.tensors():
            ref.add_tensor(nm, t, ne, data)
        ref.finalize()
        eng = pkg.HipGpuInference.from_model(model, 128)
        prompt = [i % cfg.vocab_size for i in (1, 128000, 77, 31999)]
        for t in prompt[:-1]:
            eng.prefill_token(t)
        got, want = eng.forward(prompt[-1]), ref.forward(prompt)
        for step in range(4):
            err = float(np.abs(got - want).max())
            assert err <= _tol(want), f"step {step}: max|dlogit| {err:.3e} > {_tol(want):.3e}"
            srt = np.sort(want)
            tok = orc.argmax_last(want)
            if float(srt[-1] - srt[-2]) > 4 * err:
                assert orc.argmax_last(got) == tok
            if step < 3:
                got, want = eng.forward(tok), ref.forward([tok])
        pos = eng.position()
        a = eng.decode_greedy(tok, 64).tolist()
        eng.reset()
        for t in prompt[:-1]:
            eng.prefill_token(t)
        tk = prompt[-1]
        for _ in range(pos - len(prompt) + 1):   # replay the same 3 fed tokens
            tk = orc.argmax_last(eng.forward(tk))
        assert eng.position() == pos
        b = eng.decode_greedy(tok, 64).tolist()
        assert a == b and len(set(a)) > 1
    finally:
        ref.close()
        if eng is not None:
            eng.close()


def test_the_bench_workload_itself_matches_the_oracle(pkg, orc):
    """The workload bench.py times, compared with the ORACLE at full size: Llama-3-8B Q4_K_M, the bench's
    128-token prompt (`i % 32000`, src/main.rs:1787) through prefill_token x 127 + forward — the f32 token-by-token path the
    timed decode starts from — then 8 greedy steps at kv 129..136 (src/main.rs:1812-1822, src/model/llama.rs:275-362).  Both
    sides are fed the ORACLE's greedy tokens; logits within 2e-3 * max|logit| + 2e-3 at every step, greedy tokens identical
    wherever the oracle's top-1 / top-2 gap exceeds 4x the measured error.  The same prompt through the BATCHED prompt path
    (f16 matrix-core GEMMs, the one place f16 rounding enters) against the same oracle logits: 1e-2 * max|logit| + 1e-2
    (SURVEY.md 8c).  ~40 s of oracle time for the 128-token prompt."""
    import os
    cfg = pkg.make_config("llama-3-8b", max_seq_len=160)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors():
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    prompt = [i % 32000 % cfg.vocab_size for i in range(128)]
    # the oracle parallelises over output columns like the reference's rayon loops (one task per output element, no cross-task
    # reduction: the result does not depend on the thread count) — 136 full-size tokens need the box's cores
    orc.set_threads(min(16, len(os.sched_getaffinity(0))))
    try:
        want = [ref.forward(prompt)]
        toks = []
        for _ in range(8):
            toks.append(orc.argmax_last(want[-1]))
            want.append(ref.forward([toks[-1]]))
    finally:
        orc.set_threads(1)
    ref.close()
    gaps = [float(np.sort(w)[-1] - np.sort(w)[-2]) for w in want]
    for label, batched, tol in (("exact prompt path", False, lambda w: 2e-3 * float(np.abs(w).max()) + 2e-3),
                                ("batched prompt path", True, lambda w: 1e-2 * float(np.abs(w).max()) + 1e-2)):
        eng = pkg.HipGpuInference.from_model(model, 160, flags=0 if batched else pkg.hip_backend.FLAG_EXACT_PREFILL)
        try:
            if batched:
                assert eng.prefill_is_batched()
                eng.forward_batch(prompt[:-1])
            else:
                for t in prompt[:-1]:
                    eng.prefill_token(t)
            errs, same = [], 0
            got = eng.forward(prompt[-1])
            for i in range(9):
                errs.append(float(np.abs(got - want[i]).max()))
                assert errs[-1] <= tol(want[i]), f"{label}, step {i} (kv {128 + i}): max|dlogit| {errs[-1]:.3e} > {tol(want[i]):.3e}"
                if gaps[i] > 4 * errs[-1]:
                    assert orc.argmax_last(got) == orc.argmax_last(want[i]), f"{label}, step {i}: greedy token diverged (gap {gaps[i]:.3e}, err {errs[-1]:.3e})"
                    same += 1
                if i < 8:
                    got = eng.forward(toks[i])
            assert eng.position() == 136
            print(f"bench workload vs oracle, {label}: max|dlogit| = {max(errs):.3e} (tol {tol(want[0]):.3e}), min gap {min(gaps):.3e}, "
                  f"{same}/9 tokens decided and identical")
        finally:
            eng.close()


def test_single_launch_and_split_attention_agree_across_the_switch(pkg, orc):
    """Decode attention runs as one launch per layer up to a context threshold and as split + combine beyond it (two
    graph variants, picked by the host-side position; the default threshold is 256 rows).  One engine is told to switch at 64
    rows (attn_direct=1) and does so in mid-sequence, one never uses the single launch (255), one has the default threshold spelled
    out (4: 256 rows, above this cache) and always does; all three must follow the oracle.  tests/test_gpu_attn_switch.py takes
    every state operation across the switch."""
    cfg = pkg.make_config("test-dense-d128", max_seq_len=160)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    engs = [pkg.HipGpuInference.from_model(model, 160, flags=pkg.hip_backend.FLAG_EXACT_PREFILL, attn_direct=a) for a in (1, 255, 4)]
    toks = [(13 * i + 5) % cfg.vocab_size for i in range(100)]
    worst = 0.0
    for i, t in enumerate(toks):
        want = ref.forward([t])
        got = [e.forward(t) for e in engs]
        if i in (0, 31, 62, 63, 64, 65, 99):            # around the switch at 64 rows, and the ends
            for g in got:
                worst = max(worst, float(np.abs(g - want).max()))
                assert np.abs(g - want).max() <= _tol(want)
    print(f"max|dlogit| over the three attention variants: {worst:.3e}")
    for e in engs:
        e.close()


def test_kv_shift_left_and_truncate_follow_the_reference_cache(pkg, orc):
    """KVCache::shift_left / truncate (model/mod.rs:130-172) mirrored on the device cache: the chat engine trims the
    oldest tokens when the context fills up (engine.rs:1394-1411).  Rows keep their old RoPE rotation on both sides."""
    cfg, ref, eng = _pair(pkg, orc, "test-dense-d128", "Q4_K_M", max_seq=96)
    toks = [(17 * i + 3) % cfg.vocab_size for i in range(40)]
    for t in toks:
        eng.prefill_token(t)
    ref.forward(toks)
    for e in (eng, ref):
        e.kv_shift_left(15)
    assert eng.position() == ref.position == 25
    for t in (7, 300, 12):
        got, want = eng.forward(t), ref.forward([t])
        assert np.abs(got - want).max() <= _tol(want)
    eng.kv_truncate(10)
    ref.kv_truncate(10)
    eng.kv_truncate(50)                                   # longer than the cache: no-op (model/mod.rs:131)
    assert eng.position() == ref.position == 10
    got, want = eng.forward(5), ref.forward([5])
    assert np.abs(got - want).max() <= _tol(want)
    eng.kv_shift_left(0)                                  # the reference clears the cache on a shift by 0 (model/mod.rs:143-146)
    ref.kv_shift_left(0)
    assert eng.position() == ref.position == 0
    got, want = eng.forward(9), ref.forward([9])
    assert np.abs(got - want).max() <= _tol(want)
    eng.kv_shift_left(100)                                # more than there is: cleared
    assert eng.position() == 0
    eng.close()


def test_stage_contexts_decode_correctly_in_a_fresh_process():
    """Every rank of a real multi-GPU run is a fresh process.  A kernel first launched inside a hipGraph capture was not
    replayed with the graph (ROCm 7.0), which only stages behind the first exposed — and only in a fresh process, so no
    in-process test could see it.  `lgh_finalize` now warms the kernels; this runs the reproduction in a subprocess."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for args in (("0", "1", "5"), ("255", "2", "9")):
        out = subprocess.run([sys.executable, os.path.join(root, "tools", "diag_stage_first_capture.py"), *args], check=True,
                             capture_output=True, text=True, timeout=300).stdout.strip().splitlines()
        assert out and out[-1].startswith("rep 0") and out[-1].endswith("max|d|=0.000e+00"), out


@pytest.mark.parametrize("name,layers,mix,world,batched", [("test-dense-d128", 3, "Q4_K_M", 2, False), ("test-dense-d128", 3, "Q4_K_M", 3, True),
                                                          ("llama-3-8b", 4, "Q4_K_M", 2, True)])
def test_multi_process_pipeline_rehearsal_on_one_gpu(pkg, name, layers, mix, world, batched):
    """The multi-process layer pipeline with REAL stage engines: `world` ranks, each a fresh process holding its layer range
    on device 0 (RCCL refuses two ranks on one device, so the hidden vector and the fed-back token hop through the host over
    gloo: pipeline.HostStagedComm — same HipStage, same PipelineDecoder.prefill / decode_device calls as a run on `world`
    GPUs).  The greedy tokens must equal the single-context decode of the same model token for token (per-token prompt: the
    hidden vector crosses the boundary as f32, bit-exact; batched prompt blocks: the same f16 GEMM path on both sides)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n_prompt, steps = 40, 24
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tools", "pp_rehearse.py"), name, str(layers), mix, str(n_prompt),
                                       str(steps)] + (["batched"] if batched else []), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    got = json.loads(outs[0][0].strip().splitlines()[-1])
    cfg = pkg.make_config(name, max_seq_len=n_prompt + steps + 16, num_layers=layers)
    one = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix=mix), cfg.max_seq_len)
    try:
        prompt = [(31 * i + 7) % cfg.vocab_size for i in range(n_prompt)]
        if batched and one.prefill_is_batched():
            one.forward_batch(prompt[:-1])
        else:
            for t in prompt[:-1]:
                one.prefill_token(t)
        want = one.decode_greedy(prompt[-1], steps + 4).tolist()
        assert got["tokens"] == want and got["position"] == one.position()
    finally:
        one.close()


class _PerExpert:
    """Hands the experts over one tensor at a time, as the reference's loader renames them
    (`blk.N.ffn_gate.E.weight`, src/model/loader.rs:1171-1173), optionally leaving some out."""

    def __init__(self, model, drop=()):
        self._m, self.config, self._drop = model, model.config, set(drop)

    def tensors(self, layers=None):
        ne_exp = self.config.num_experts
        for name, t, ne, data in self._m.tensors(layers):
            if "_exps." not in name:
                yield name, t, ne, data
                continue
            per = data.nbytes // ne_exp
            for e in range(ne_exp):
                nm = name.replace("_exps.weight", f".{e}.weight")
                if nm not in self._drop:
                    yield nm, t, ne[:2], data[e * per:(e + 1) * per]


def test_per_expert_upload_matches_stacks_and_a_missing_expert_fails_finalize(pkg, orc):
    """Experts uploaded one at a time fill the same device stacks as the 3-D tensors; a model that lacks one expert tensor
    must fail `lgh_finalize` with InitializationFailed naming it, instead of decoding from uninitialised memory."""
    cfg = pkg.make_config("test-moe", max_seq_len=16)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    a = pkg.HipGpuInference.from_model(model, 16)
    b = pkg.HipGpuInference.from_model(_PerExpert(model), 16)
    for t in (3, 4):
        a.prefill_token(t)
        b.prefill_token(t)
    assert np.array_equal(a.forward(5), b.forward(5))
    a.close()
    b.close()
    with pytest.raises(pkg.BackendError) as ei:
        pkg.HipGpuInference.from_model(_PerExpert(model, drop={"blk.1.ffn_up.3.weight"}), 16)
    assert ei.value.variant == "InitializationFailed" and "blk.1.ffn_up.{3}.weight" in str(ei.value)


def test_generic_attention_shapes_and_top_k_follow_the_oracle(pkg, orc):
    """Shapes outside the templated attention kernels (the reference's kernel takes any head_dim / group size,
    kernels.rs:1395-1458) run the one-workgroup-per-head kernel; MoE layers with more than two selected experts run them two
    at a time (moe.rs:321-413).  Qwen2-7B's 7 query heads per kv head, head_dim 96, top-3 and top-4 routing."""
    cases = [("test-dense", "Q8_0", dict(num_heads=14, num_kv_heads=2, head_dim=64, hidden_size=896)),           # G = 7, k % 256 != 0
             ("test-dense", "Q4_0", dict(num_heads=14, num_kv_heads=2, head_dim=64, hidden_size=896)),           # Q4_0 on mv_kernel
             ("test-dense", "Q4_K_M", dict(num_heads=8, num_kv_heads=4, head_dim=96, hidden_size=768, intermediate_size=1536)),   # head_dim 96
             ("test-dense", "Q4_K_M", dict(num_heads=6, num_kv_heads=2, head_dim=128, hidden_size=768, intermediate_size=1536)),  # G = 3
             ("test-moe", "Q4_K_M", dict(num_experts=6, num_experts_per_token=3)),
             ("test-moe", "Q5_K_M", dict(num_experts=8, num_experts_per_token=4))]
    for name, mix, kw in cases:
        cfg, ref, eng = _pair(pkg, orc, name, mix, max_seq=48, **kw)
        toks = [(31 * i + 2) % cfg.vocab_size for i in range(20)]
        worst = 0.0
        for i, t in enumerate(toks):
            got, want = eng.forward(t), ref.forward([t])
            worst = max(worst, float(np.abs(got - want).max()))
            assert np.abs(got - want).max() <= _tol(want), (name, kw, i)
        pos = eng.position()
        dev = eng.decode_greedy(3, 10).tolist()
        eng.kv_truncate(pos)
        host, tok = [], 3
        for _ in range(10):
            tok = orc.argmax_last(eng.forward(tok))
            host.append(tok)
        assert dev == host
        print(f"{name}/{mix} {kw}: max|dlogit|={worst:.3e}")
        eng.close()
        ref.close()


def test_decode_matvec_geometries_follow_the_oracle(pkg, orc):
    """Widths whose decode mat-vecs run in 5- and 7-slice workgroups (320 / 448 threads) or in 8 uneven slices with idle waves
    (tests/matvec_ref.py: mvq_geometry): hidden 1792 / ffn 2304, hidden 1280 / ffn 3328, hidden 2560 / ffn 3584; 2 layers, 24 tokens."""
    cases = [("Q4_K_M", True, dict(num_heads=14, num_kv_heads=2, head_dim=128, hidden_size=1792, intermediate_size=2304, use_neox_rope=True)),
             ("Q5_K_M", False, dict(num_heads=10, num_kv_heads=10, head_dim=128, hidden_size=1280, intermediate_size=3328)),
             ("Q8_0", False, dict(num_heads=20, num_kv_heads=4, head_dim=128, hidden_size=2560, intermediate_size=3584))]
    for mix, with_bias, kw in cases:
        cfg = pkg.make_config("test-dense", max_seq_len=32, **kw)
        assert cfg.num_layers == 2
        model = pkg.SynthModel(cfg, mix=mix, with_bias=with_bias)
        ref = orc.Model(cfg.as_dict())
        for nm, t, ne, data in model.tensors(keep=True):
            ref.add_tensor(nm, t, ne, data)
        ref.finalize()
        eng = pkg.HipGpuInference.from_model(model, 32)
        worst = 0.0
        for i in range(24):
            t = (31 * i + 2) % cfg.vocab_size
            got, want = eng.forward(t), ref.forward([t])
            worst = max(worst, float(np.abs(got - want).max()))
            assert np.all(np.isfinite(got)) and np.abs(got - want).max() <= _tol(want), (mix, kw, i)
        print(f"test-dense/{mix} {kw}: max|dlogit|={worst:.3e}")
        eng.close()
        ref.close()


def test_generic_attention_refuses_contexts_that_do_not_fit_lds(pkg):
    """The generic attention kernel keeps max_seq_len scores in LDS: a longer context is refused by lgh_create with
    Unsupported and a message naming the shape (not by a launch error in finalize)."""
    cfg = pkg.make_config("test-dense", max_seq_len=50000, num_heads=14, num_kv_heads=2, hidden_size=896)
    with pytest.raises(pkg.BackendError) as ei:
        pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q8_0"), 50000)
    assert ei.value.variant == "Unsupported"


@pytest.mark.parametrize("name,mix,stages", [("test-dense-d128", "Q4_K_M", 2), ("test-dense-d128", "Q4_K_M", 3), ("test-moe", "Q5_K_M", 2)])
def test_in_library_pipeline_equals_single_context(pkg, orc, name, mix, stages):
    """lgh_pipeline_*: `stages` stage contexts in ONE process (here all on one device: the peer copy degenerates to a
    device-to-device copy), hidden vector and greedy token hopped on the device.  Logits and greedy tokens must equal the
    single context's bit for bit (src/distributed/pipeline.rs:50-96 partitioning), and GpuModelWrapper drives the pipeline
    handle unchanged."""
    cfg = pkg.make_config(name, max_seq_len=64)
    model = pkg.SynthModel(cfg, mix=mix)
    one = pkg.HipGpuInference.from_model(model, 64)
    pipe = pkg.HipPipeline.from_model(model, 64, stages)
    assert pipe.stages() == stages
    try:
        wrap, ctx = pkg.GpuModelWrapper(pipe), pkg.InferenceContext()
        prompt = [3, 900 % cfg.vocab_size, 31, 7]
        for t in prompt[:-1]:
            one.prefill_token(t)
        assert np.array_equal(wrap.forward(prompt, ctx), one.forward(prompt[-1]))
        assert pipe.position() == one.position() == 4
        assert pipe.decode_greedy(5, 24).tolist() == one.decode_greedy(5, 24).tolist()
        assert np.array_equal(pipe.forward(9), one.forward(9))
        pipe.reset()
        one.reset()
        assert pipe.position() == 0
        assert np.array_equal(pipe.forward(2), one.forward(2))
        with pytest.raises(pkg.BackendError) as ei:
            pipe.forward(cfg.vocab_size)
        assert ei.value.variant == "InvalidArgument"
    finally:
        one.close()
        pipe.close()


@pytest.mark.parametrize("name,mix,n_tok,kv", [("test-dense", "Q4_K_M", 70, 1), ("test-dense-d128", "Q4_K_M", 70, 1), ("test-moe", "Q5_K_M", 40, 1),
                                               ("test-dense", "Q8_0", 4000, 1), ("test-dense", "Q4_K_M", 70, 2), ("test-dense-d128", "Q4_K_M", 70, 3),
                                               ("test-moe", "Q5_K_M", 40, 2), ("test-dense", "Q8_0", 4000, 3), ("test-dense-d128", "Q6_K", 300, 2)])
def test_quantized_kv_cache_follows_the_reference_formats(pkg, orc, name, mix, n_tok, kv):
    """The reference's QuantizedKVCache (src/model/kv_quantized.rs) on the device, all three of its byte formats
    (lgh_model_desc.kv_cache_type; LGH_FLAG_KV_INT8 is the older spelling of type 1).  Int8 (:143-300, 385-410): int8 rows + one
    scale per (kv head, position), scale = max|x| / 127, round half away from zero, read back as scale * q.  FP8 E4M3 / E5M2
    (:413-565): one byte per element, mantissa truncated, no scales.  Against the oracle with the same format switched on,
    context 1 ... 4000; the cache is a quarter of the f32 one; shift_left / truncate move rows (and scales) together (:330-380).
    Tolerance: the decode path's (2e-3 relative) for int8; 4x that for FP8 — the encoders themselves are bit-exact
    (test_gpu_ops.py::test_kv_cache_formats_bit_exact), but they TRUNCATE to 2-3 mantissa bits, so a K/V element that differs
    in its last f32 bit between device and oracle can land on either side of a step of 12.5-25 % of its value (measured: one
    position in 300 at 1.06x the f32 tolerance)."""
    ktol = 1.0 if kv == 1 else 4.0
    max_seq = n_tok + 24
    cfg = pkg.make_config(name, max_seq_len=max_seq)
    model = pkg.SynthModel(cfg, mix=mix)
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    if kv == 1:
        ref.set_kv_int8(True)
        eng = pkg.HipGpuInference.from_model(model, max_seq, flags=pkg.hip_backend.FLAG_KV_INT8)
    else:
        ref.set_kv_fp8(kv - 1)
        eng = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=kv)
    f32 = pkg.HipGpuInference.from_model(model, max_seq)
    assert eng.stats()["kv_bytes"] * 3 < f32.stats()["kv_bytes"]
    f32.close()
    try:
        toks = [(41 * i + 7) % cfg.vocab_size for i in range(n_tok)]
        check = set(range(8)) | {n_tok // 2, n_tok - 2, n_tok - 1} | set(range(60, 68))
        worst = 0.0
        if n_tok > 500:                                   # long context: the bulk goes in as a prompt on both sides
            bulk = toks[:n_tok - 6]
            for t in bulk:
                eng.prefill_token(t)
            ref.forward(bulk[:-1])
            want = ref.forward(bulk[-1:])                 # (logits of the last prompt token on the oracle only)
            toks = toks[n_tok - 6:]
            check = set(range(6))
        for i, t in enumerate(toks):
            got, want = eng.forward(t), ref.forward([t])
            if i in check:
                worst = max(worst, float(np.abs(got - want).max()))
                assert np.abs(got - want).max() <= ktol * _tol(want), (i, float(np.abs(got - want).max()))
        print(f"{name}/{mix} KV format {kv}, {eng.position()} rows: max|dlogit|={worst:.3e}")
        if n_tok <= 500:
            for e in (eng, ref):
                e.kv_shift_left(11)
            assert eng.position() == ref.position
            for t in (5, 6, 7):
                got, want = eng.forward(t), ref.forward([t])
                assert np.abs(got - want).max() <= ktol * _tol(want)
            eng.kv_truncate(20)
            ref.kv_truncate(20)
            got, want = eng.forward(9), ref.forward([9])
            assert np.abs(got - want).max() <= ktol * _tol(want)
            pos = eng.position()
            dev = eng.decode_greedy(3, 8).tolist()
            eng.kv_truncate(pos)
            host, tok = [], 3
            for _ in range(8):
                tok = orc.argmax_last(eng.forward(tok))
                host.append(tok)
            assert dev == host
    finally:
        eng.close()
        ref.close()




@pytest.mark.parametrize("name,mix,n_tok,bits", [("test-dense", "Q4_K_M", 70, 2), ("test-dense-d128", "Q4_K_M", 70, 2), ("test-dense-d128", "Q4_K_M", 70, 3),
                                                 ("test-moe", "Q5_K_M", 40, 3), ("test-dense-d128", "Q4_K_M", 700, 2), ("test-dense", "Q8_0", 4000, 3)])
def test_turboquant_kv_cache_follows_the_reference(pkg, orc, name, mix, n_tok, bits):
    """KVCacheType::TurboQuantMSE { bits } — what the reference's `--kv-cache-type tq2 | tq3` selects (src/config.rs:808-817) — on
    the device: K / V rows stored as rotated Lloyd-Max codes (src/model/turboquant/), attention over the codes
    (src/model/kv_turboquant.rs:88-201 behind Backend::attention_turboquant, src/backend/mod.rs:240-264), against the oracle's
    restatement with the SAME sign vectors on both sides (lgh_set_kv_rotation_signs <-> HadamardRotation::signs()), context 1 ...
    4000.  The codes themselves are bit-exact (test_gpu_ops.py::test_turboquant_codes_bit_exact); a K / V element that differs
    in its last f32 bits between device and oracle can fall into the neighbouring cell (a step of ~0.5-1 sigma of the rotated
    coordinate), so the logit tolerance is 4x the f32 path's, as for the reference's FP8 caches.  The cache is 1/16 (2 bits) or
    3/32 (3 bits) of the f32 one; shift_left / truncate move code rows (kv_turboquant.rs:236-266)."""
    ktol = 4.0
    max_seq = n_tok + 24
    cfg = pkg.make_config(name, max_seq_len=max_seq)
    model = pkg.SynthModel(cfg, mix=mix)
    rng = np.random.default_rng(7 + bits)
    signs = np.where(rng.integers(0, 2, cfg.num_layers * cfg.num_kv_heads * 2 * cfg.head_dim) == 1, 1.0, -1.0).astype(np.float32)
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    ref.set_kv_turboquant(bits, signs)
    kv_type = pkg.hip_backend.KV_TQ2 if bits == 2 else pkg.hip_backend.KV_TQ3
    eng = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=kv_type, kv_rotation_signs=signs)
    f32 = pkg.HipGpuInference.from_model(model, max_seq)
    assert eng.stats()["kv_bytes"] * 32 == f32.stats()["kv_bytes"] * bits
    f32.close()
    try:
        toks = [(41 * i + 7) % cfg.vocab_size for i in range(n_tok)]
        check = set(range(8)) | {n_tok // 2, n_tok - 2, n_tok - 1} | set(range(60, 68))
        worst = 0.0
        if n_tok > 500:
            bulk = toks[:n_tok - 6]
            for t in bulk:
                eng.prefill_token(t)
            ref.forward(bulk[:-1])
            ref.forward(bulk[-1:])
            toks = toks[n_tok - 6:]
            check = set(range(6))
        for i, t in enumerate(toks):
            got, want = eng.forward(t), ref.forward([t])
            if i in check:
                worst = max(worst, float(np.abs(got - want).max()) / _tol(want))
                assert np.abs(got - want).max() <= ktol * _tol(want), (i, float(np.abs(got - want).max()), _tol(want))
        print(f"{name}/{mix} TurboQuant {bits}-bit KV, {eng.position()} rows: max|dlogit| = {worst:.4f} x the f32 tolerance")
        if n_tok <= 500:
            for e in (eng, ref):
                e.kv_shift_left(11)
            assert eng.position() == ref.position
            for t in (5, 6, 7):
                got, want = eng.forward(t), ref.forward([t])
                assert np.abs(got - want).max() <= ktol * _tol(want)
            eng.kv_truncate(20)
            ref.kv_truncate(20)
            got, want = eng.forward(9), ref.forward([9])
            assert np.abs(got - want).max() <= ktol * _tol(want)
            pos = eng.position()
            dev = eng.decode_greedy(3, 8).tolist()                    # graph replays == the host loop
            eng.kv_truncate(pos)
            host, tok = [], 3
            for _ in range(8):
                tok = orc.argmax_last(eng.forward(tok))
                host.append(tok)
            assert dev == host
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("name,mix,n_tok,bits", [("test-dense", "Q4_K_M", 70, 2), ("test-dense-d128", "Q4_K_M", 70, 3), ("test-moe", "Q5_K_M", 40, 2),
                                                 ("test-dense-d128", "Q4_K_M", 700, 2)])
def test_turboquant_prod_kv_cache_follows_the_reference(pkg, orc, name, mix, n_tok, bits):
    """KVCacheType::TurboQuantProd { bits } — `--kv-cache-type tq2-qjl | tq3-qjl` (src/config.rs:808-817): the TurboQuant codes plus
    the QJL correction of the attention scores (src/model/turboquant/qjl.rs, quant.rs:133-168) — against the oracle's restatement
    with the SAME sign vectors and the SAME projection matrices on both sides (lgh_set_kv_qjl_matrices <-> QjlProjector's matrix).
    Stored rows are bit-exact (test_gpu_ops.py::test_turboquant_qjl_rows_bit_exact); logits to the TurboQuant tolerance.  The K rows
    carry head_dim / 8 + 4 more bytes (quant.rs:176-186; the reference also stores such bits for V rows and never reads them — they
    are not kept here); shift_left / truncate move them with the codes."""
    ktol = 4.0
    max_seq = n_tok + 24
    cfg = pkg.make_config(name, max_seq_len=max_seq)
    model = pkg.SynthModel(cfg, mix=mix)
    rng = np.random.default_rng(17 + bits)
    signs = np.where(rng.integers(0, 2, cfg.num_layers * cfg.num_kv_heads * 2 * cfg.head_dim) == 1, 1.0, -1.0).astype(np.float32)
    qjl = rng.standard_normal(cfg.num_layers * cfg.num_kv_heads * cfg.head_dim * cfg.head_dim).astype(np.float32)
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    ref.set_kv_turboquant(bits, signs)
    ref.set_kv_turboquant_qjl(qjl)
    hb = pkg.hip_backend
    eng = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=hb.KV_TQ2_QJL if bits == 2 else hb.KV_TQ3_QJL, kv_rotation_signs=signs,
                                         kv_qjl_matrices=qjl)
    mse = pkg.HipGpuInference.from_model(model, max_seq, kv_cache_type=hb.KV_TQ2 if bits == 2 else hb.KV_TQ3, kv_rotation_signs=signs)
    n_rows = cfg.num_layers * cfg.num_kv_heads * max_seq
    assert eng.stats()["kv_bytes"] == mse.stats()["kv_bytes"] + n_rows * (cfg.head_dim // 8 + 4)
    try:
        toks = [(41 * i + 7) % cfg.vocab_size for i in range(n_tok)]
        check = set(range(8)) | {n_tok // 2, n_tok - 2, n_tok - 1} | set(range(60, 68))
        worst, moved = 0.0, 0.0
        if n_tok > 500:
            bulk = toks[:n_tok - 6]
            for t in bulk:
                eng.prefill_token(t)
                mse.prefill_token(t)
            ref.forward(bulk[:-1])
            ref.forward(bulk[-1:])
            toks = toks[n_tok - 6:]
            check = set(range(6))
        for i, t in enumerate(toks):
            got, want, plain = eng.forward(t), ref.forward([t]), mse.forward(t)
            if i in check:
                worst = max(worst, float(np.abs(got - want).max()) / _tol(want))
                moved = max(moved, float(np.abs(got - plain).max()) / _tol(want))
                assert np.abs(got - want).max() <= ktol * _tol(want), (i, float(np.abs(got - want).max()), _tol(want))
        print(f"{name}/{mix} TurboQuant-prod {bits}-bit KV, {eng.position()} rows: max|dlogit| = {worst:.4f} x the f32 tolerance; "
              f"the QJL correction moves the logits by up to {moved:.1f} x that tolerance")
        assert moved > 1.0                                            # the correction is not a no-op
        if n_tok <= 500:
            for e in (eng, ref):
                e.kv_shift_left(11)
            assert eng.position() == ref.position
            for t in (5, 6, 7):
                got, want = eng.forward(t), ref.forward([t])
                assert np.abs(got - want).max() <= ktol * _tol(want)
            eng.kv_truncate(20)
            ref.kv_truncate(20)
            got, want = eng.forward(9), ref.forward([9])
            assert np.abs(got - want).max() <= ktol * _tol(want)
            pos = eng.position()
            dev = eng.decode_greedy(3, 8).tolist()                    # graph replays == the host loop
            eng.kv_truncate(pos)
            host, tok = [], 3
            for _ in range(8):
                tok = orc.argmax_last(eng.forward(tok))
                host.append(tok)
            assert dev == host
    finally:
        eng.close()
        mse.close()
        ref.close()


def test_turboquant_qjl_matrix_contract(pkg):
    """lgh_set_kv_qjl_matrices: exactly [layers][kv heads][head_dim][head_dim] finite values, only on a TurboQuantProd context, only
    before finalize; without it the context decodes with its deterministic stand-in."""
    hb = pkg.hip_backend
    cfg = pkg.make_config("test-dense-d128", max_seq_len=16)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    n = cfg.num_layers * cfg.num_kv_heads * cfg.head_dim * cfg.head_dim
    bad_nan = np.ones(n, np.float32)
    bad_nan[5] = np.nan
    for bad in (np.ones(n - 1, np.float32), bad_nan):
        with pytest.raises(pkg.BackendError) as ei:
            pkg.HipGpuInference.from_model(model, 16, kv_cache_type=hb.KV_TQ2_QJL, kv_qjl_matrices=bad)
        assert ei.value.variant == "InvalidArgument"
    with pytest.raises(pkg.BackendError):
        pkg.HipGpuInference.from_model(model, 16, kv_cache_type=hb.KV_TQ2, kv_qjl_matrices=np.ones(n, np.float32))   # an MSE context
    eng = pkg.HipGpuInference.from_model(model, 16, kv_cache_type=hb.KV_TQ3_QJL)                                      # stand-ins
    a = eng.forward(3)
    b = eng.forward(4)
    eng.reset()
    assert np.array_equal(a, eng.forward(3)) and np.array_equal(b, eng.forward(4)) and np.all(np.isfinite(b))
    eng.close()


def test_turboquant_sign_vector_contract(pkg):
    """lgh_set_kv_rotation_signs: only +-1, exactly [layers][kv heads][2][head_dim] values, only on a TurboQuant context and only
    before finalize; without it the context decodes with its deterministic stand-in; head sizes the butterfly cannot take are
    refused at lgh_create."""
    hb = pkg.hip_backend
    cfg = pkg.make_config("test-dense-d128", max_seq_len=16)
    model = pkg.SynthModel(cfg, mix="Q4_K_M")
    n = cfg.num_layers * cfg.num_kv_heads * 2 * cfg.head_dim
    for bad in (np.ones(n - 1, np.float32), np.full(n, 0.5, np.float32)):
        with pytest.raises(pkg.BackendError) as ei:
            pkg.HipGpuInference.from_model(model, 16, kv_cache_type=hb.KV_TQ2, kv_rotation_signs=bad)
        assert ei.value.variant == "InvalidArgument"
    with pytest.raises(pkg.BackendError):
        pkg.HipGpuInference.from_model(model, 16, kv_rotation_signs=np.ones(n, np.float32))      # an f32-cache context
    eng = pkg.HipGpuInference.from_model(model, 16, kv_cache_type=hb.KV_TQ3)                      # stand-in signs
    a = eng.forward(3)
    eng.reset()
    assert np.array_equal(a, eng.forward(3)) and np.all(np.isfinite(a))
    eng.close()
    with pytest.raises(pkg.BackendError) as ei:
        pkg.HipGpuInference.from_model(pkg.SynthModel(pkg.make_config("test-dense", max_seq_len=16, head_dim=96), mix="Q4_K_M"), 16,
                                       kv_cache_type=hb.KV_TQ2)
    assert ei.value.variant in ("Unsupported", "InvalidArgument")


@pytest.mark.parametrize("kv", range(8), ids=["f32", "int8", "fp8_e4m3", "fp8_e5m2", "tq2", "tq3", "tq2_qjl", "tq3_qjl"])
def test_kv_bytes_are_the_layout_querys_slots(pkg, kv):
    """What a context allocates for its caches is what lgh_kv_cache_layout says a host should expect, to the byte: one slot per layer
    for the context's own sequence, and max_batch more per layer for the multi-sequence engine's."""
    cfg = pkg.make_config("test-dense", max_seq_len=64)
    slot = pkg.hip_backend.kv_cache_layout(kv, cfg.num_kv_heads, 64, cfg.head_dim).slot_bytes
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q4_K_M"), 64, kv_cache_type=kv)
    try:
        own = eng.stats()["kv_bytes"]
        assert own == cfg.num_layers * slot
        eng.batch_create(3)
        assert eng.stats()["kv_bytes"] - own == 3 * cfg.num_layers * slot
    finally:
        eng.close()
