"""Build-level properties of the two row-wise kernels of a tensor-parallel prompt block (csrc/tp_prefill.hip), on the ISA hipcc emits
with the Makefile's own flags (cross-compiled here, no GPU needed): tp_pf_partial_kernel and all eight instantiations of
tp_pf_reduce_kernel<N> have zero scratch, no spilled register and leading arguments preloaded in SGPRs.  tp_pf_reduce_kernel<8>
holds 16 partial-block loads, the residual and the norm weights in flight at once (20 x 4 VGPRs); a spill there would put scratch
traffic into a kernel whose whole point is to move each byte once.

The reduce kernel's loads are also counted: 2 N + 4 sixteen-byte loads per thread (N partial blocks, the residual, the norm weights,
two each), all of them requested before the first vector-memory wait."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft
import test_build_props_entry as bpe


@pytest.fixture(scope="module")
def kernels():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(graft.PKG_DIR, "csrc", "tp_prefill.hip")
    r = subprocess.run([hipcc, *bpe.makefile_flags(), "--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True, check=True)
    meta = bpe.parse_isa(r.stdout)
    out = {}
    for name, k in meta.items():
        if "tp_pf_" not in name:
            continue
        y = re.search(r"\.name:\s+%s\n.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)" % re.escape(name), r.stdout, re.S)
        out[name] = dict(k, spills=(int(y.group(1)), int(y.group(2))))
    return out


def _reduce_n(name):
    m = re.search(r"tp_pf_reduce_kernelILi(\d+)E", name)
    return int(m.group(1)) if m else None


def test_both_kernels_and_every_rank_count_are_built(kernels):
    assert sum("tp_pf_partial_kernel" in n for n in kernels) == 1, sorted(kernels)
    assert sorted(_reduce_n(n) for n in kernels if _reduce_n(n)) == list(range(1, 9)), sorted(kernels)
    assert len(kernels) == 9, sorted(kernels)


def test_no_scratch_no_spills_preloaded_arguments(kernels):
    for name, k in kernels.items():
        meta = k["meta"]
        print(f"{name}: {meta['NumVgprs']} VGPRs, scratch {meta['ScratchSize']}, spills {k['spills']}, preload {k['preload']} dwords")
        assert meta["ScratchSize"] == 0 and k["spills"] == (0, 0), (name, meta, k["spills"])
        assert not any(s.startswith("scratch_") for s in k["ins"]), (name, "scratch access")
        assert meta["NumVgprs"] <= 128, (name, meta)   # two workgroups of 4 waves per SIMD at the least
        assert k["preload"] > 0, (name, "no preloaded arguments")


def test_reduce_requests_its_loads_before_it_waits(kernels):
    for name, k in kernels.items():
        n = _reduce_n(name)
        if not n:
            continue
        body = bpe.from_entry(k["ins"])
        loads = [i for i, s in enumerate(body) if s.startswith("global_load_dwordx4")]
        assert len(loads) == 2 * n + 4, (name, len(loads))
        waits = [i for i, s in enumerate(body) if s.startswith("s_waitcnt") and "vmcnt" in s]
        assert waits, name
        before = sum(1 for i in loads if i < waits[0])
        print(f"{name}: {len(loads)} 16-byte loads, {before} requested before the first vector-memory wait")
        assert before == len(loads), (name, before)
