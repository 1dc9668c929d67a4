"""bench.py --dump-outputs: what the timed decode returned, written as .npy so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(*args):
    return subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=600)


def test_dump_outputs_refuses_the_paths_it_does_not_cover(tmp_path):
    out = tmp_path / "dump"
    bad = _bench("--gpus", "2", "--fake-stage", "--steps", "3", "--dump-outputs", str(out))
    assert bad.returncode != 0 and "--dump-outputs" in bad.stderr and not bad.stdout.strip()
    assert not out.exists()
    zero = _bench("--steps", "0")
    assert zero.returncode != 0 and "--steps" in zero.stderr


def test_dump_outputs_types_and_size_limit(tmp_path):
    import bench
    bench.dump_outputs(str(tmp_path / "d"), {"tokens": np.array([1, 2, 4000000000], np.uint32),
                                             "last_logits": np.array([0.5, -1.25], np.float32)})
    t, lg = np.load(tmp_path / "d" / "tokens.npy"), np.load(tmp_path / "d" / "last_logits.npy")
    assert t.dtype == np.float64 and t.tolist() == [1.0, 2.0, 4e9]
    assert lg.dtype == np.float32 and lg.tolist() == [0.5, -1.25]
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "big").exists()


@pytest.mark.gpu
def test_dump_outputs_are_what_the_timed_decode_returned(gpu, pkg, tmp_path):
    K, W, P = 6, 2, 8
    common = ["--gpus", "1", "--model", "test-dense", "--mix", "Q4_K_M", "--steps", str(K), "--warmup", str(W), "--prompt", str(P),
              "--cpu-seconds", "0", "--profile-steps", "0"]
    dumps = []
    for name in ("a", "b"):
        r = _bench(*common, "--dump-outputs", str(tmp_path / name))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1
        rec = json.loads(lines[0])
        assert rec["steps"] == K and rec["ms_per_step"] > 0
        dumps.append({n: np.load(tmp_path / name / f"{n}.npy") for n in ("tokens", "last_logits")})
    a, b = dumps
    cfg = pkg.make_config("test-dense")
    assert a["tokens"].dtype == np.float64 and a["tokens"].shape == (K,)
    assert a["last_logits"].dtype == np.float32 and a["last_logits"].shape == (cfg.vocab_size,)
    for n in a:
        assert np.array_equal(a[n], b[n]), f"{n} differs between two runs with the same arguments"
    logits = a["last_logits"]
    assert len(logits) - 1 - int(np.argmax(logits[::-1])) == int(a["tokens"][-1])
    # the bench protocol through the engine directly: prompt, W warm-up steps, then K timed steps
    eng = pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q4_K_M"), cfg.max_seq_len)
    try:
        prompt = [(i % 32000) % cfg.vocab_size for i in range(P)]
        for t in prompt[:-1]:
            eng.prefill_token(t)
        eng.forward(prompt[-1])
        warm = eng.decode_greedy(prompt[-1], W)
        want = eng.decode_greedy(int(warm[-1]), K)
    finally:
        eng.close()
    assert a["tokens"].astype(np.int64).tolist() == want.astype(np.int64).tolist()
