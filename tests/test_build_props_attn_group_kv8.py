"""Build-level properties of the group decode attention over byte caches (cross-compiled here, no GPU needed):
attn_group_kv8_kernel<D, NW, FMT>, D 64 / 128 x NW 4 / 8 x FMT int8 / FP8 E4M3 / FP8 E5M2.  None per group size; none may touch scratch
or spill."""
from test_build_props import _usage


def test_group_kv8_attention_has_twelve_clean_instantiations():
    att = _usage("attention_group_kv8.hip")
    assert len(att) == 12 and all("attn_group_kv8_kernel" in fn for fn in att), sorted(att)
    for fn, u in att.items():
        print(fn, u)
        assert u.get("ScratchSize", 0) == 0, (fn, u)
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (fn, u)
