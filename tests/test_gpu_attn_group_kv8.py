"""attn_group_kv8_kernel<D, NW, FMT> (csrc/attention_group_kv8.hip): decode attention over an int8 / FP8 cache for the group sizes the
split kernels have no instantiation for.  The kernel through lgh_op_attention_kv8, which picks it from the shape, against the float64
restatement over the STORED values under the bound every decode kernel is held to, the row it stores bit for bit against the oracle's
encoders; the engine with LGH_ATTN_GROUP_MATRIX and a byte cache against the CPU oracle with the same format switched on."""
import numpy as np
import pytest

import attention_ref as ar
from test_gpu_attention import N_KV, SPLITS, Worst, _dominant_row, _kv8_encode, _queries

pytestmark = pytest.mark.gpu

# (max_seq, pos): no cached row, one, the staged row as the last row of a tile / the first of a fresh tile / after it, the 4-wave kernel
# deep into a cache, the last row of an 8-wave cache
POS = [(1024, p) for p in (0, 1, 15, 16, 17, 1000)] + [(4096, 4095)]


@pytest.mark.parametrize("g", (3, 7, 16))
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("kv_type", (1, 2, 3), ids=["int8", "fp8_e4m3", "fp8_e5m2"])
def test_group_kv8_kernel_against_float64(gpu, orc, kv_type, d, g):
    """Rows 0 .. pos-1 read from the byte cache, row pos quantized from k_new / v_new, stored as the oracle encodes it and attended
    through its stored values; every row at or past pos holds NaN (scale NaN, byte 0x7F) before the call and is never read."""
    W = Worst(f"group_kv8 type={kv_type} d={d} g={g}")
    i8 = kv_type == 1
    table = None if i8 else ar.fp8_table(orc, kv_type)
    finite = None if i8 else np.flatnonzero(np.isfinite(table) & (np.abs(table) <= 4.0))
    values = (lambda b, s: ar.int8_values(b, s)) if i8 else (lambda b, s: table[b])
    scale = 1.0 / np.sqrt(d)
    for ci, (max_seq, pos) in enumerate(POS):
        for ki, kind in enumerate(("normal", "dominant", "hot")):
            rng = np.random.default_rng([kv_type, d, g, ci, ki, 8])
            q = _queries(rng, kind, N_KV * g, g, d)
            ks = vs = None
            if i8:
                kb, vb = (rng.integers(-127, 128, (N_KV, max_seq, d)).astype(np.int8).view(np.uint8) for _ in range(2))
                ks, vs = (rng.uniform(0.005, 0.03, (N_KV, max_seq)).astype(np.float32) for _ in range(2))
                ks[:, pos:] = vs[:, pos:] = np.nan
            else:
                kb, vb = (rng.choice(finite, (N_KV, max_seq, d)).astype(np.uint8) for _ in range(2))
                kb[:, pos:] = vb[:, pos:] = 0x7F
            k_new, v_new = (rng.standard_normal((N_KV, d)).astype(np.float32) for _ in range(2))
            if kind == "dominant":   # kv head 0: the new row dominates; kv head 1: the last cached row
                k_new[0] = _dominant_row(rng, q[:g], d, scale, 40.0)
                if pos > 0:
                    kb[1, pos - 1], s = _kv8_encode(orc, kv_type, _dominant_row(rng, q[g:2 * g], d, scale, 40.0))
                    if i8:
                        ks[1, pos - 1] = s
            want = [a.copy() if a is not None else None for a in (kb, vb, ks, vs)]   # what the cache must hold after the call
            for h in range(N_KV):
                for bytes_x, scales_x, row in ((want[0], want[2], k_new[h]), (want[1], want[3], v_new[h])):
                    bytes_x[h, pos], s = _kv8_encode(orc, kv_type, row)
                    if i8:
                        scales_x[h, pos] = s
            n = pos + 1
            kv_vals = values(want[0][:, :n], want[2][:, :n] if i8 else None)
            vv_vals = values(want[1][:, :n], want[3][:, :n] if i8 else None)
            s_split = SPLITS[(ci + ki) % 3]
            out, *got = gpu.op_attention_kv8(kv_type, q, kb, vb, ks, vs, k_new, v_new, scale, pos, s_split)
            case = f"kind={kind} max_seq={max_seq} pos={pos} splits={s_split}"
            for nm, a, b in zip(("K bytes", "V bytes", "K scales", "V scales"), got, want):
                if b is not None:   # bit for bit (the scales past pos are NaN)
                    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"{nm} {case}")
            ref = ar.decode(q, kv_vals, vv_vals, scale, n)
            S, vmax = ar.magnitude(q, kv_vals, scale, n), float(np.abs(vv_vals).max())
            W.add("group_kv8", ar.worst_ratio(out, ref, S, vmax, n), case)
    W.check()


@pytest.mark.parametrize("mix,kw,kv", [
    ("Q4_K_M", dict(num_heads=6, num_kv_heads=2, head_dim=128, hidden_size=768, intermediate_size=1536), 1),     # G = 3, int8
    ("Q4_K_M", dict(num_heads=14, num_kv_heads=2, head_dim=128, hidden_size=1792, intermediate_size=2304), 2),   # G = 7, FP8 E4M3
    ("Q8_0", dict(num_heads=20, num_kv_heads=4, head_dim=64, hidden_size=1280, intermediate_size=3328), 3),      # G = 5, FP8 E5M2
], ids=["g3_int8", "g7_e4m3", "g5_e5m2"])
def test_engine_with_group_policy_and_byte_cache(pkg, orc, mix, kw, kv):
    """Tolerance: the decode path's 2e-3 for int8, four times that for FP8 (the truncating encoders:
    test_gpu_model.py::test_quantized_kv_cache_follows_the_reference_formats)."""
    hb = pkg.hip_backend
    cfg = pkg.make_config("test-dense", max_seq_len=64, **kw)
    model = pkg.SynthModel(cfg, mix=mix)
    ref = orc.Model(cfg.as_dict())
    for nm, t, ne, data in model.tensors(keep=True):
        ref.add_tensor(nm, t, ne, data)
    ref.finalize()
    if kv == 1:
        ref.set_kv_int8(True)
    else:
        ref.set_kv_fp8(kv - 1)
    eng = pkg.HipGpuInference.from_model(model, 64, attn_policy=hb.ATTN_GROUP_MATRIX, kv_cache_type=kv)
    ktol = 1.0 if kv == 1 else 4.0

    def close(got, want):
        assert float(np.abs(got - want).max()) <= ktol * (2e-3 * float(np.abs(want).max()) + 2e-3)

    assert not eng.prefill_is_batched()
    eng.set_prefill_policy(hb.PREFILL_BATCH_BYTE_KV)
    assert not eng.prefill_is_batched()
    for i in range(40):   # the kv length crosses 16 and 32
        t = (7 * i + 3) % cfg.vocab_size
        close(eng.forward(t), ref.forward([t]))
    eng.kv_truncate(20)
    ref.kv_truncate(20)
    close(eng.forward(9), ref.forward([9]))
    eng.set_profiling(True)
    eng.forward(5)
    eng.set_profiling(False)
    sym = eng.stats()["symbols"]
    assert sym["lgh::attn_group_kernel"]["launches"] == cfg.num_layers
    assert "lgh::attn_partial_kernel" not in sym
    eng.close()
    ref.close()
