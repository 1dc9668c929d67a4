"""Build-level properties of the prompt pass's block attention on the matrix cores (cross-compiled here, no GPU needed):
attn_pf_mfma_kernel<D, 8, TQ>, D 64 / 128 over an f32 cache (TQ false) or the TurboQuant scratch (TQ true).  With
test_build_props_kv8_prefill.py's six attn_pf_kv8_kernel instantiations these are the kernels that share csrc/attn_block.h: none may touch
scratch memory or spill."""
from test_build_props_kv8_prefill import _instances


def test_block_attention_has_four_clean_instantiations():
    att = _instances("attn_pf_mfma_kernel")
    # (Li<D>ELi<NW>ELb<TQ>E)
    want = {f"attn_pf_mfma_kernelILi{d}ELi8ELb{tq}EE" for d in (64, 128) for tq in (0, 1)}
    assert {next((w for w in want if w in fn), fn) for fn in att} == want and len(att) == 4, sorted(att)
    for fn, u in att.items():
        print(fn, u)
        assert u.get("ScratchSize", 0) == 0, (fn, u)
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (fn, u)
