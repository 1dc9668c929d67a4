"""lgh_model_desc.attn_policy with a quantized cache as lgh_create reads it, answered before a device is looked for (no GPU needed; device
9999 exists on no machine, so a descriptor that passes every check answers NotAvailable)."""
import pytest


def _variant(pkg, kv_cache_type, attn_policy, flags=0):
    """14 / 2 heads, 7 per kv head: no split kernel."""
    cfg = pkg.make_config("test-dense", max_seq_len=64, num_heads=14, num_kv_heads=2, hidden_size=896)
    with pytest.raises(pkg.BackendError) as ei:
        pkg.HipGpuInference.from_model(pkg.SynthModel(cfg, mix="Q8_0"), 64, device=9999, flags=flags, kv_cache_type=kv_cache_type,
                                       attn_policy=attn_policy)
    return ei.value.variant


@pytest.mark.parametrize("kv,flags", [("KV_INT8", 0), ("KV_FP8_E4M3", 0), ("KV_FP8_E5M2", 0), ("KV_F32", "FLAG_KV_INT8")])
def test_byte_caches_need_the_group_policy(pkg, kv, flags):
    hb = pkg.hip_backend
    kv, flags = getattr(hb, kv), getattr(hb, flags) if flags else 0
    assert _variant(pkg, kv, 0, flags) == "Unsupported"
    assert _variant(pkg, kv, hb.ATTN_GROUP_MATRIX, flags) == "NotAvailable"   # past the shape check


def test_turboquant_caches_stay_refused(pkg):
    assert _variant(pkg, pkg.hip_backend.KV_TQ3, pkg.hip_backend.ATTN_GROUP_MATRIX) == "Unsupported"
