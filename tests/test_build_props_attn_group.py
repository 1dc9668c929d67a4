"""Build-level properties of the group decode attention (cross-compiled here, no GPU needed): attn_group_kernel<D, NW>, D 64 / 128 x
NW 4 (caches below 2048 rows) / 8.  One kernel per head size and wave count, none per group size; none may touch scratch or spill."""
from test_build_props import _usage


def test_group_attention_has_four_clean_instantiations():
    att = _usage("attention_group.hip")
    want = {f"_ZN3lgh17attn_group_kernelILi{d}ELi{nw}EEEvPKfS2_S2_jjfPKijPfS5_" for d in (64, 128) for nw in (4, 8)}
    assert set(att) == want, sorted(att)
    for fn, u in att.items():
        print(fn, u)
        assert u.get("ScratchSize", 0) == 0, (fn, u)
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (fn, u)
