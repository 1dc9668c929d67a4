"""Build-level properties of the ENTRY of the decode kernels (cross-compiled here, no GPU needed): the static-plan mat-vec
(mvqs_kernel, csrc/matvec_mfma.hip) and the decode instantiations of attn_partial_kernel (csrc/attention.hip).

Every node of the decode graph is one link of a serial chain, so what a wave does before its first memory request is paid once per
node and overlaps nothing.  mvqs_kernel takes what its first requests need as leading arguments, which arrive preloaded in SGPRs,
and reads the position word with a plain load that nothing waits for until the requests are out.  Held here, on the ISA text
hipcc emits with the Makefile's own flags:
  * the kernel descriptor reports a non-zero argument preload length (both kernels);
  * mvqs_kernel: from the kernel's entry, in text order, no s_waitcnt with an lgkmcnt term stands before the first vector-memory
    load.

The entry: a kernel with preloaded arguments begins with a header for firmware that does not preload — scalar loads of those
arguments, a wait, a branch — and firmware that preloads enters behind it (256 bytes in); the header is not on the path measured
on the MI355X and is skipped here.

attn_partial_kernel is NOT held to the second property: it waits for the position word before its first K / V request.  Requesting
the first rows ahead of the position measured no gain (profiles/r05_entry_loads.md) and was not kept."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft
import test_build_props as bp

CSRC = os.path.join(graft.PKG_DIR, "csrc")
CODEGEN_NEUTRAL = {"-Wall", "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c"}


def makefile_flags():
    """HIPFLAGS of the product Makefile with its defaults (no EXTRA_HIPFLAGS, ARCH = gfx950)."""
    text = open(os.path.join(graft.PKG_DIR, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    line = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", text, re.M).group(1)
    return line.replace("$(EXTRA_HIPFLAGS)", "").replace("$(ARCH)", arch).split()


def parse_isa(text):
    """-> {mangled kernel name: dict(ins=[instructions from the function label], preload=int, meta={comment fields})}"""
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            kernels[cur] = dict(ins=[], preload=0, meta={}, done=False)
            continue
        st = line.strip()
        m = re.match(r"\.amdhsa_kernel (\S+)", st)
        if m:
            cur = m.group(1)
            continue
        if cur is None:
            continue
        k = kernels.get(cur)
        if k is None:
            continue
        m = re.match(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", st)
        if m:
            k["preload"] = int(m.group(1))
        m = re.match(r"; (ScratchSize|NumVgprs|Occupancy|VGPRs spilled|SGPRs spilled|sgpr_spill_count|vgpr_spill_count): (\d+)", st)
        if m:
            k["meta"][m.group(1)] = int(m.group(2))
        if st.startswith(".Lfunc_end"):
            k["done"] = True
        if k["done"] or not st or st[0] in ";." or st.endswith(":"):
            continue
        k["ins"].append(st.split(";")[0].strip())
    return kernels


def from_entry(ins):
    """The instructions from where firmware that preloads the arguments enters (module docstring)."""
    for i, s in enumerate(ins[:16]):
        if s.startswith("s_branch"):
            return ins[i + 1:]
        if not (s.startswith("s_load_dword") or s.startswith("s_waitcnt")):
            break
    return ins


def scalar_waits_before_first_vector_load(ins):
    body = from_entry(ins)
    first = next((i for i, s in enumerate(body) if re.match(r"(global|buffer)_load", s)), None)
    assert first is not None, "no vector-memory load in the kernel"
    return [i for i, s in enumerate(body[:first]) if s.startswith("s_waitcnt") and "lgkmcnt" in s], first


@pytest.fixture(scope="module")
def isa():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = {}
    for src in ("matvec_mfma.hip", "attention.hip"):
        r = subprocess.run([hipcc, *makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", "-"], capture_output=True,
                           text=True, check=True)
        out[src] = parse_isa(r.stdout)
    return out


def _decode_attn(kernels):
    """attn_partial_kernel<D, G, NW, PF, DIRECT, MULTI> with PF = false -> {name: (nw, direct, multi)}"""
    res = {}
    for name in kernels:
        m = re.search(r"attn_partial_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])E", name)
        if m and m.group(4) == "0":
            res[name] = (int(m.group(3)), m.group(5) == "1", m.group(6) == "1")
    return res


def test_static_plans_request_before_any_scalar_wait(isa):
    mvqs = {n: k for n, k in isa["matvec_mfma.hip"].items() if "mvqs_kernel" in n}
    assert 1 <= len(mvqs) <= 8, sorted(mvqs)
    for name, k in mvqs.items():
        assert k["preload"] > 0, (name, "no preloaded arguments")
        waits, first = scalar_waits_before_first_vector_load(k["ins"])
        print(f"{name}: preload {k['preload']} dwords, {first} instructions before the first vector load, scalar waits at {waits}")
        assert not waits, (name, waits, first)


def test_decode_attention_has_preloaded_arguments(isa):
    attn = _decode_attn(isa["attention.hip"])
    # split with 4 and 8 waves, DIRECT (16 waves) and MULTI with 4 and 8 waves, for 2 head sizes x 4 group sizes
    assert len(attn) == 8 * 5, sorted(attn)
    assert {(nw, d, m) for nw, d, m in attn.values()} == {(4, False, False), (8, False, False), (16, True, False), (4, False, True), (8, False, True)}
    for name in attn:
        assert isa["attention.hip"][name]["preload"] > 0, (name, "no preloaded arguments")


def test_entry_kernels_keep_their_registers_at_the_makefile_flags(isa):
    """tests/test_build_props.py compiles with flags of its own; where the Makefile's differ in anything that reaches code generation,
    the kernels of this file are held to zero scratch, no spills and <= 256 VGPRs at the Makefile's flags as well."""
    mine = [f for f in makefile_flags() if f not in CODEGEN_NEUTRAL]
    theirs = [f for f in bp.FLAGS if f not in CODEGEN_NEUTRAL]
    if mine == theirs:
        return   # the same code: test_build_props.py and test_build_props_static.py hold it
    mvqs = [n for n in isa["matvec_mfma.hip"] if "mvqs_kernel" in n]
    for src, names in (("matvec_mfma.hip", mvqs), ("attention.hip", list(_decode_attn(isa["attention.hip"])))):
        for n in names:
            meta = isa[src][n]["meta"]
            assert meta.get("ScratchSize", 0) == 0, (n, meta)
            assert meta.get("vgpr_spill_count", 0) == 0 and meta.get("VGPRs spilled", 0) == 0, (n, meta)
            assert "NumVgprs" in meta and meta["NumVgprs"] <= 256, (n, meta)
