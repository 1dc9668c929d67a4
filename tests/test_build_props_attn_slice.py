"""Build-level budgets of attn_slice_kernel<D, G, S> (csrc/attention_slice.hip), the single-launch decode attention for contexts of at
most 256 rows with S workgroups per query head, on the ISA hipcc emits with the Makefile's own flags (cross-compiled here, no GPU needed).

Held here, for the one S per head size that the launcher uses and all 8 (D, G):
  * the instantiations exist, and no other;
  * zero scratch and no spilled register;
  * at most 128 VGPRs, so that the 16 waves of a workgroup fit on a CU (4 per SIMD, 512 VGPRs each);
  * leading arguments preloaded in SGPRs;
  * the kernel has no row loop: every global load stands in straight-line code in front of the first barrier (two chunks of K on every
    wave, the V slice on the V waves), with the query's 5 D / 32 of them in the text;
  * every exponential stands between the first and the second barrier (the pass that computes p once per row)."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft
import test_build_props_entry as bpe
from test_build_props_attn_head import loops

S_KEPT = {64: 4, 128: 4}   # attention_slice.hip: kAttnSliceS
SHAPES = {(d, g, S_KEPT[d]) for d in (64, 128) for g in (1, 2, 4, 8)}


@pytest.fixture(scope="module")
def kernels():
    """-> {mangled name: dict(body = lines of the function, meta = parse_isa's record, spills = (sgpr, vgpr) of the code object's metadata)}"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(graft.PKG_DIR, "csrc", "attention_slice.hip")
    text = subprocess.run([hipcc, *bpe.makefile_flags(), "--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True, check=True).stdout
    meta = bpe.parse_isa(text)
    ks = {}
    for m in re.finditer(r"^(_Z\w*attn_slice_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end", text, re.M | re.S):
        name = m.group(1)
        y = re.search(r"\.name:\s+%s\n.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)" % re.escape(name), text, re.S)
        ks[name] = dict(body=m.group(2).splitlines(), meta=meta[name], spills=(int(y.group(1)), int(y.group(2))))
    shapes = {tuple(int(x) for x in re.search(r"attn_slice_kernelILi(\d+)ELi(\d+)ELi(\d+)E", n).groups()) for n in ks}
    assert len(ks) == 8 and shapes == SHAPES, sorted(ks)
    return ks


def test_registers_scratch_and_preload(kernels):
    for name, k in kernels.items():
        meta, ins = k["meta"]["meta"], loops(k["body"])[0]
        print(f"{name}: {meta['NumVgprs']} VGPRs, scratch {meta['ScratchSize']}, spills {k['spills']}, preload {k['meta']['preload']} dwords")
        assert meta["ScratchSize"] == 0 and k["spills"] == (0, 0), (name, meta, k["spills"])
        assert not any(s.startswith("scratch_") for s in ins), (name, "scratch access")
        assert meta["NumVgprs"] <= 128, (name, meta)
        assert k["meta"]["preload"] > 0, (name, "no preloaded arguments")


def test_loads_at_entry_and_exponentials_only_in_the_softmax_pass(kernels):
    for name, k in kernels.items():
        ins, spans = loops(k["body"])
        d = int(re.search(r"attn_slice_kernelILi(\d+)E", name).group(1))
        bars = [i for i, s in enumerate(ins) if s == "s_barrier"]
        assert len(bars) == 3, (name, bars)
        loads = [i for i, s in enumerate(ins) if s.startswith("global_load")]
        # the query (D / 32), two chunks of K (2 D / 32), the V slice of both chunks (2 D / 32): once each in the text
        assert len(loads) == 5 * d // 32 and all(i < bars[0] for i in loads), (name, loads, bars)
        assert not any(a <= i <= b for i in loads for a, b in spans), (name, "a global load inside a loop")
        exps = [i for i, s in enumerate(ins) if s.startswith("v_exp")]
        assert exps and all(bars[0] < i < bars[1] for i in exps), (name, exps, bars)
        valu = [sum(1 for s in ins[a:b] if s.startswith("v_")) for a, b in zip([0] + bars, bars + [len(ins)])]
        print(f"{name}: static VALU entry..barrier 1 {valu[0]}, softmax pass {valu[1]}, barrier 2..3 {valu[2]}, epilogue {valu[3]}")
