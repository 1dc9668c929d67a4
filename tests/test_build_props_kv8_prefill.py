"""Build-level properties of the batched prompt pass over the byte KV caches (cross-compiled here, no GPU needed): the block attention
attn_pf_kv8_kernel<D, 8, FMT> and the row store kv8_pf_store_kernel<D, FMT>, D 64 / 128 x int8 / FP8 E4M3 / FP8 E5M2.

The store keeps a row in registers from its 16-byte load to its dword store: no LDS.  Neither kernel may touch scratch memory or spill."""
import functools

from test_build_props import _usage


@functools.lru_cache(maxsize=None)
def _attention():
    return _usage("attention.hip")


def _instances(stem):
    # (an instantiation's mangled name spells its template arguments: Li<D>ELi<NW>ELi<FMT>E, or Li<D>ELi<FMT>E)
    return {fn: u for fn, u in _attention().items() if stem in fn}


def test_block_attention_over_bytes_has_six_clean_instantiations():
    att = _instances("attn_pf_kv8_kernel")
    want = {f"attn_pf_kv8_kernelILi{d}ELi8ELi{fmt}EE" for d in (64, 128) for fmt in (1, 2, 3)}
    assert {next((w for w in want if w in fn), fn) for fn in att} == want and len(att) == 6, sorted(att)
    for fn, u in att.items():
        print(fn, u)
        assert u.get("ScratchSize", 0) == 0, (fn, u)
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (fn, u)


def test_row_store_uses_no_lds_no_scratch():
    store = _instances("kv8_pf_store_kernel")
    want = {f"kv8_pf_store_kernelILi{d}ELi{fmt}EE" for d in (64, 128) for fmt in (1, 2, 3)}
    assert {next((w for w in want if w in fn), fn) for fn in store} == want and len(store) == 6, sorted(store)
    for fn, u in store.items():
        print(fn, u)
        assert u.get("ScratchSize", 0) == 0, (fn, u)
        assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (fn, u)
        assert u.get("LDS Size", 0) == 0, (fn, u)
