"""attn_group_kernel<D, NW> (csrc/attention_group.hip): decode attention with the up-to-16 query heads of a kv group as the N index of
the f32 matrix instruction, for group sizes the split kernels have no instantiation for.  The kernel through lgh_op_attention_decode
path 4 against the float64 restatement under the bound every decode kernel is held to; the engine with LGH_ATTN_GROUP_MATRIX against the
CPU oracle (decode, batched prompt pass, a context past the any-shape kernel's 38400 rows)."""
import numpy as np
import pytest

import attention_ref as ar
from test_gpu_attention import _f32_case

pytestmark = pytest.mark.gpu

# (max_seq, pos): the first row, around a 16-row tile edge, a long context (4 waves), the last row of a cache in the 8-wave range
POS = [(1024, 0), (1024, 15), (1024, 16), (1024, 17), (1024, 1000), (4096, 4095)]
SPLITS = (1, 7, 32)   # 32: more splits than tiles at every position but the last two


@pytest.mark.parametrize("g", (1, 3, 5, 7, 16))   # 1 pads fifteen head columns, 16 none
@pytest.mark.parametrize("d", (64, 128))
def test_group_kernel_against_float64(gpu, d, g):
    worst, fails = 0.0, []
    for ci, (max_seq, pos) in enumerate(POS):
        for kind in ("normal", "dominant", "hot"):
            q, k, v, scale = _f32_case(np.random.default_rng([d, g, ci, len(kind), 4]), kind, g, d, max_seq, pos)   # rows past pos: NaN
            n = pos + 1
            ref = ar.decode(q, k, v, scale, n)
            S, vmax = ar.magnitude(q, k, scale, n), float(np.abs(v[:, :n]).max())
            for s in SPLITS:
                r = ar.worst_ratio(gpu.op_attention_decode(gpu.ATTN_GROUP, q, k, v, scale, pos, s), ref, S, vmax, n)
                worst = max(worst, r)
                if not r <= 1.0:
                    fails.append(f"kind={kind} max_seq={max_seq} pos={pos} splits={s}: err / bound = {r:.3g}")
    print(f"WORST attn_group d={d} g={g}: err / bound = {worst:.4f}")
    assert not fails, "\n".join(fails[:20])


def test_group_path_refusals(gpu, pkg):
    for path, n_heads, d, want in ((gpu.ATTN_GROUP, 34, 128, "Unsupported"), (gpu.ATTN_GROUP, 6, 96, "Unsupported"), (5, 6, 128, "InvalidArgument")):
        q, kv = np.ones((n_heads, d), np.float32), np.ones((2, 64, d), np.float32)
        with pytest.raises(pkg.BackendError) as ei:
            gpu.op_attention_decode(path, q, kv, kv, 0.1, 3, 4)
        assert ei.value.variant == want, (path, n_heads, d)


def _pair(pkg, orc, mix, max_seq, flags=0, attn_policy=1, **kw):
    cfg = pkg.make_config("test-dense", max_seq_len=max_seq, **kw)
    model = pkg.SynthModel(cfg, mix=mix)
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    return cfg, model, ref, pkg.HipGpuInference.from_model(model, max_seq, flags=flags, attn_policy=attn_policy)


def _close(got, want, rel):
    assert float(np.abs(got - want).max()) <= rel * float(np.abs(want).max()) + rel


@pytest.mark.parametrize("mix,kw", [
    ("Q4_K_M", dict(num_heads=6, num_kv_heads=2, head_dim=128, hidden_size=768, intermediate_size=1536)),     # G = 3
    ("Q4_K_M", dict(num_heads=14, num_kv_heads=2, head_dim=128, hidden_size=1792, intermediate_size=2304)),   # G = 7
    ("Q8_0", dict(num_heads=20, num_kv_heads=4, head_dim=64, hidden_size=1280, intermediate_size=3328)),      # G = 5
], ids=["g3", "g7", "g5"])
def test_engine_with_group_policy(pkg, orc, mix, kw):
    hb = pkg.hip_backend
    cfg, model, ref, exact = _pair(pkg, orc, mix, 64, flags=hb.FLAG_EXACT_PREFILL, **kw)
    eng = pkg.HipGpuInference.from_model(model, 64, attn_policy=hb.ATTN_GROUP_MATRIX)
    plain = pkg.HipGpuInference.from_model(model, 64)
    assert eng.prefill_is_batched() and not plain.prefill_is_batched() and not exact.prefill_is_batched()
    plain.close()
    toks = [(7 * i + 3) % cfg.vocab_size for i in range(40)]   # the kv length crosses 16 and 32
    for t in toks:
        _close(exact.forward(t), ref.forward([t]), 2e-3)
    exact.set_profiling(True)
    exact.forward(5)
    exact.set_profiling(False)
    sym = exact.stats()["symbols"]
    assert sym["lgh::attn_group_kernel"]["launches"] == cfg.num_layers
    assert "lgh::attn_partial_kernel" not in sym   # the symbol attn_decode_any_kernel's launches are counted under
    exact.close()
    # the batched prompt pass (f16 GEMMs: test_gpu_prefill.py's tolerance), then a decode step over the rows it stored
    ref.reset()
    eng.forward_batch(toks[:36])
    _close(eng.forward(toks[36]), ref.forward(toks[:37]), 1e-2)
    eng.close()


def test_long_context_past_the_generic_row_limit(pkg, orc):
    cfg, _, ref, eng = _pair(pkg, orc, "Q8_0", 50000, num_heads=14, num_kv_heads=2, hidden_size=896)
    for t in (3, 17, 255):
        _close(eng.forward(t), ref.forward([t]), 2e-3)
    eng.close()
