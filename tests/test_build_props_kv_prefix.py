"""Build-level properties of the prompt cache's copy kernel (cross-compiled here, no GPU needed): both instantiations of
kv_prefix_copy_kernel — save and restore — keep their staged loads in registers: no scratch, no spills, and no LDS.  Read from the
compiler's resource-usage remarks, as tests/test_build_props.py does for the decode path."""
from test_build_props import _usage


def test_both_copy_instantiations_use_no_scratch_lds_or_spills():
    usage = {fn: u for fn, u in _usage("kv_prefix.hip").items() if "kv_prefix_copy_kernel" in fn}
    assert len(usage) == 2, sorted(usage)   # <false> save, <true> restore
    for fn, u in usage.items():
        assert u.get("ScratchSize", 0) == 0, f"{fn} uses {u['ScratchSize']} B/lane of scratch"
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (fn, u)
        assert u.get("LDS Size", 0) == 0, (fn, u)
