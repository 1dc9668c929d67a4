"""Build-level budgets of attn_head_kernel<D, G> (csrc/attention.hip), the single-launch decode attention with one workgroup of 16
waves per query head, on the ISA hipcc emits with the Makefile's own flags (cross-compiled here, no GPU needed).

The kernel this one replaces in the engine (attn_partial_kernel<D, G, 16, false, true>) was bound by vector issue: about 16 vector-ALU
instructions per (row, head) in its row loop, every lane of a row repeating the online-softmax update, plus merges full of
exponentials.  Held here, for all 8 instantiations:
  * zero scratch and no spilled register;
  * at most 128 VGPRs, so that the 16 waves of a workgroup fit on a CU (4 per SIMD, 512 VGPRs each);
  * leading arguments preloaded in SGPRs;
  * at most 8 vector-ALU instructions per (row, head) in the steady-state row loops.  The kernel has two, the score loop over K and
    the accumulation loop over V (the loops that contain global loads); one pass of either consumes four 128-row chunks, 32 rows per
    wave, so (VALU of the K loop + VALU of the V loop) / 32 is the figure per row of the head.  Every v_* instruction between a loop's
    first label and its last backward branch counts, address arithmetic and compares included;
  * every exponential of the kernel stands between the first and the second barrier (the pass that computes p once per row): none in
    the score pass, none in the accumulation, none in a merge.

What the 8-instruction budget does NOT cover: those two loops run from 5 chunks (513 rows) on.  Up to 512 rows the kernel runs its
straight-line entry (query, addresses, the first four requests), the tails behind the loops (at most four chunks each) and the
epilogue, all of them once per launch and none of them per row beyond 16 K rows and 16 V rows per wave and 256 rows; their static
VALU counts are printed by test_exponentials_only_in_the_softmax_pass for the record and held to no bound, since they hold the
one-time set-up of the launch and both the short and the long path's code."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft
import test_build_props_entry as bpe

ROWS_PER_PASS = 32   # per wave: 4 chunks x 8 K rows; 4 chunks x (D / 32 sweeps) x (256 / D rows)
SHAPES = {(d, g) for d in (64, 128) for g in (1, 2, 4, 8)}


def split_kernels(text):
    """-> {mangled name: dict(body = lines of the function, meta = parse_isa's record, spills = (sgpr, vgpr) of the code object's metadata)}"""
    meta = bpe.parse_isa(text)
    out = {}
    for m in re.finditer(r"^(_Z\w*attn_head_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end", text, re.M | re.S):
        name = m.group(1)
        y = re.search(r"\.name:\s+%s\n.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)" % re.escape(name), text, re.S)
        out[name] = dict(body=m.group(2).splitlines(), meta=meta[name], spills=(int(y.group(1)), int(y.group(2))))
    return out


def loops(lines):
    """The loops of a function body as merged [first, last] instruction ranges; -> (instructions, ranges)"""
    ins, labels = [], {}
    for line in lines:
        st = line.strip()
        m = re.match(r"^(\.LBB\w+):", st)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if not st or st[0] in ";." or st.endswith(":"):
            continue
        ins.append(st.split(";")[0].strip())
    spans = []
    for i, s in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", s)
        if m and m.group(1) in labels and labels[m.group(1)] <= i:
            spans.append([labels[m.group(1)], i])
    spans.sort()
    merged = []
    for a, b in spans:
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    return ins, merged


@pytest.fixture(scope="module")
def kernels():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(graft.PKG_DIR, "csrc", "attention.hip")
    r = subprocess.run([hipcc, *bpe.makefile_flags(), "--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True, check=True)
    ks = split_kernels(r.stdout)
    shapes = {tuple(int(x) for x in re.search(r"attn_head_kernelILi(\d+)ELi(\d+)E", n).groups()) for n in ks}
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


def test_row_loops_stay_inside_the_vector_budget(kernels):
    for name, k in kernels.items():
        ins, spans = loops(k["body"])
        row_loops = [(a, b) for a, b in spans if any(s.startswith("global_load") for s in ins[a:b + 1])]
        assert len(row_loops) == 2, (name, spans)   # scores over K, accumulation over V
        valu = [sum(1 for s in ins[a:b + 1] if s.startswith("v_")) for a, b in row_loops]
        loads = [sum(1 for s in ins[a:b + 1] if s.startswith("global_load")) for a, b in row_loops]
        d = int(re.search(r"attn_head_kernelILi(\d+)E", name).group(1))
        assert loads == [4 * d // 32, 4 * d // 32], (name, loads)   # four chunks' requests per pass of either loop
        per_row = sum(valu) / ROWS_PER_PASS
        print(f"{name}: K loop {valu[0]} + V loop {valu[1]} VALU per {ROWS_PER_PASS} rows = {per_row:.2f} per (row, head)")
        assert per_row <= 8.0, (name, valu)


def test_exponentials_only_in_the_softmax_pass(kernels):
    for name, k in kernels.items():
        ins, spans = loops(k["body"])
        bars = [i for i, s in enumerate(ins) if s == "s_barrier"]
        assert len(bars) == 3, (name, bars)
        exps = [i for i, s in enumerate(ins) if s.startswith("v_exp")]
        assert exps and all(bars[0] < i < bars[1] for i in exps), (name, exps, bars)
        row_loops = [(a, b) for a, b in spans if any(s.startswith("global_load") for s in ins[a:b + 1])]

        def valu(a, b):   # outside the two row loops
            return sum(1 for i in range(a, b) if ins[i].startswith("v_") and not any(x <= i <= y for x, y in row_loops))
        print(f"{name}: static VALU outside the row loops: entry..barrier 1 {valu(0, bars[0])}, softmax pass {valu(bars[0], bars[1])}, "
              f"barrier 2..3 {valu(bars[1], bars[2])}, epilogue {valu(bars[2], len(ins))}")
