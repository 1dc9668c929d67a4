"""lgh_kv_cache_layout on the CPU (no device needed): the one place that knows how large a KV cache format is.  Its answers against
the counts of the reference's constructors, written out here: the f32 cache 4 bytes per element (gpu_only.rs:555-572);
QuantizedKVCache::new a byte per element, plus an f32 scale per int8 row (kv_quantized.rs:57-102; the FP8 formats have no scales,
:31-35); TurboQuantKVCache::new head_dim / 4 bytes per row for 2 bits and head_dim / 8 * 3 for 3 bits (kv_turboquant.rs:36-86), and
for TurboQuantProd head_dim / 8 + 4 more bytes per K row (sign bits + the residual's norm, quant.rs:176-186)."""
import pytest

KV_TYPES = range(8)   # f32, int8, fp8_e4m3, fp8_e5m2, tq2, tq3, tq2_qjl, tq3_qjl


def _row_scale_qjl(kv, d):
    row = {0: 4 * d, 1: d, 2: d, 3: d, 4: d // 4, 5: d // 8 * 3, 6: d // 4, 7: d // 8 * 3}[kv]
    return row, (4 if kv == 1 else 0), (d // 8 + 4 if kv in (6, 7) else 0)


@pytest.mark.parametrize("n_kv,max_seq", [(1, 1), (2, 48), (8, 4096)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("kv", KV_TYPES)
def test_layout_matches_the_reference_constructors(pkg, kv, d, n_kv, max_seq):
    lay = pkg.hip_backend.kv_cache_layout(kv, n_kv, max_seq, d)
    row, scale, qjl = _row_scale_qjl(kv, d)
    rows = n_kv * max_seq
    assert lay.kv_cache_type == kv
    assert (lay.row_bytes, lay.scale_bytes, lay.qjl_bytes, lay.rows) == (row, scale, qjl, rows)
    assert (lay.k_bytes, lay.v_bytes) == (rows * row, rows * row)
    assert (lay.k_scale_bytes, lay.v_scale_bytes) == (rows * scale, rows * scale)
    assert lay.k_qjl_bytes == rows * qjl
    assert lay.slot_bytes == rows * (2 * row + 2 * scale + qjl)


def test_legacy_flag_spelling_answers_as_int8(pkg):
    hb = pkg.hip_backend
    old, new = hb.kv_cache_layout(hb.KV_F32, 2, 48, 64, flags=hb.FLAG_KV_INT8), hb.kv_cache_layout(hb.KV_INT8, 2, 48, 64)
    assert old.kv_cache_type == hb.KV_INT8
    for name, _ in hb.KvLayout._fields_:
        assert getattr(old, name) == getattr(new, name), name
    assert old.slot_bytes == 2 * 2 * 48 * (64 + 4)
    # a type of its own is not overridden by the flag
    assert hb.kv_cache_layout(hb.KV_TQ3, 2, 48, 64, flags=hb.FLAG_KV_INT8).row_bytes == 64 // 8 * 3


def test_unknown_cache_type_is_refused(pkg):
    with pytest.raises(pkg.BackendError) as ei:
        pkg.hip_backend.kv_cache_layout(8, 2, 48, 64)
    assert ei.value.variant == "InvalidArgument"
