"""lgh_model_desc.attn_policy as lgh_create and lgh_kv_cache_layout read it, answered before a device is looked for (no GPU needed;
device 9999 exists on no machine, so a descriptor that passes every check answers NotAvailable)."""
import ctypes as C

import pytest


def _variant(pkg, attn_policy):
    """The 14 / 2-head model at 50000 rows: past attn_decode_any_kernel's 38400 (tests/test_gpu_model.py pins its refusal)."""
    cfg = pkg.make_config("test-dense", max_seq_len=50000, num_heads=14, num_kv_heads=2, hidden_size=896)
    with pytest.raises(pkg.BackendError) as ei:
        pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q8_0"), 50000, device=9999, attn_policy=attn_policy)
    return ei.value.variant


def test_policy_word_at_create(pkg):
    assert _variant(pkg, 2) == "InvalidArgument"                                   # a bit that is not assigned
    assert _variant(pkg, 0) == "Unsupported"                                       # the any-shape kernel's row limit
    assert _variant(pkg, pkg.hip_backend.ATTN_GROUP_MATRIX) == "NotAvailable"      # past the shape check


@pytest.mark.parametrize("missing", (1, 2), ids=["before_attn_policy", "before_kv_cache_type"])
def test_older_descriptor_sizes_are_still_read(pkg, missing):
    hb = pkg.hip_backend
    d, out = hb.ModelDesc(), hb.KvLayout()
    d.struct_size = C.sizeof(hb.ModelDesc) - 4 * missing
    d.num_kv_heads, d.max_seq_len, d.head_dim, d.kv_cache_type, d.attn_policy = 2, 64, 128, hb.KV_INT8, 2   # beyond struct_size: not read
    assert hb.load_library().lgh_kv_cache_layout(C.byref(d), C.byref(out)) == 0
    assert out.kv_cache_type == (hb.KV_F32 if missing == 2 else hb.KV_INT8)
