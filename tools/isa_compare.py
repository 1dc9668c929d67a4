#!/usr/bin/env python3
"""Compare two gfx950 ISA listings of one source file, kernel by kernel: has a change that should not alter code generation altered it?

    hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only csrc/attention.hip -o parent.s     (at the parent commit)
    hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only csrc/attention.hip -o change.s     (at the change)
    python tools/isa_compare.py parent.s change.s [parent2.s change2.s ...] [--md out.md] [--brief]

Per kernel: scratch bytes, occupancy, LDS bytes, VGPR / AGPR counts, and the histogram of the mnemonics that do arithmetic or reach
memory — vector floating point, matrix, vector memory — with the encoding suffixes (_e32, _e64, _dpp, _sdwa) stripped and v_fmac_*
counted as v_fma_* (the two-address encoding of the same operation, chosen after register allocation).  Mnemonics are classified by
general prefixes only.  Integer, scalar, select, move, wait and nop instructions are not counted: a compiler reorders and re-encodes
those freely for the same arithmetic.  LDS instructions are counted and shown, but not compared: how many static copies of a
ds_write a kernel holds follows from how its branches were laid out.

Exit status 1 when a kernel is missing on one side or fails: scratch above 0, occupancy lower, LDS bytes different, a histogram
different.  Register counts may move.
"""
import argparse
import collections
import re
import shutil
import subprocess
import sys

META = {"ScratchSize": "scratch", "Occupancy": "occ", "LDSByteSize": "lds", "NumVgprs": "vgpr", "NumAgprs": "agpr"}
SUFFIX = re.compile(r"(_e32|_e64|_dpp|_sdwa)+$")
FLOAT = re.compile(r"^v_.*(_f16|_f32|_f64|_bf16)")


def classify(mnemonic):
    """-> 'matrix' | 'vmem' | 'lds' | 'vfloat' | None"""
    if mnemonic.startswith(("v_mfma", "v_smfmac")):
        return "matrix"
    if mnemonic.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mnemonic.startswith("ds_"):
        return "lds"
    if FLOAT.match(mnemonic):
        return "vfloat"
    return None


def parse(path):
    """-> {mangled kernel name: dict(scratch, occ, lds, vgpr, agpr, hist=Counter of (class, mnemonic))}"""
    kernels, cur, body = {}, None, False
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, body = m.group(1), True
            kernels[cur] = dict(hist=collections.Counter())
            continue
        if cur is None:
            continue
        st = line.strip()
        if st.startswith(".Lfunc_end"):
            body = False
            continue
        m = re.match(r"; (\w+): (\d+)", st)
        if m and m.group(1) in META and META[m.group(1)] not in kernels[cur]:
            kernels[cur][META[m.group(1)]] = int(m.group(2))
            continue
        if not body or not st or st[0] in ";." or st.endswith(":"):
            continue
        mnemonic = SUFFIX.sub("", st.split()[0]).replace("v_fmac_", "v_fma_").replace("v_pk_fmac_", "v_pk_fma_")
        cls = classify(mnemonic)
        if cls:
            kernels[cur]["hist"][(cls, mnemonic)] += 1
    return {k: v for k, v in kernels.items() if "occ" in v}   # device functions that are not kernels carry no occupancy line


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d)
        depth, cut = 0, len(d)
        for i, c in enumerate(d):   # drop the argument list: the first '(' outside the template brackets
            depth += c == "<"
            depth -= c == ">"
            if c == "(" and depth == 0:
                cut = i
                break
        short[n] = d[:cut].replace("lgh::", "")
    return short


def compare(parent_path, change_path):
    """-> (rows for the table, failure strings)"""
    a, b = parse(parent_path), parse(change_path)
    rows, fails = [], []
    names = demangle(sorted(set(a) | set(b)))
    for n in sorted(set(a) | set(b), key=lambda n: names[n]):
        if n not in a or n not in b:
            fails.append(f"{names[n]}: only in the {'parent' if n in a else 'change'}")
            continue
        p, c = a[n], b[n]
        bad = []
        if c.get("scratch", 0) != 0:
            bad.append(f"scratch {c['scratch']}")
        if c["occ"] < p["occ"]:
            bad.append(f"occupancy {p['occ']} -> {c['occ']}")
        if c.get("lds", 0) != p.get("lds", 0):
            bad.append(f"LDS {p.get('lds', 0)} -> {c.get('lds', 0)}")
        ph, ch = ({k: v for k, v in x["hist"].items() if k[0] != "lds"} for x in (p, c))
        if ph != ch:
            d = {k: (ph.get(k, 0), ch.get(k, 0)) for k in set(ph) | set(ch) if ph.get(k, 0) != ch.get(k, 0)}
            bad.append("histogram " + ", ".join(f"{k[1]} {v[0]} -> {v[1]}" for k, v in sorted(d.items())))
        per_class = collections.Counter()
        for (cls, _), cnt in c["hist"].items():
            per_class[cls] += cnt
        rows.append((names[n], p, c, per_class, bad))
        fails += [f"{names[n]}: {x}" for x in bad]
    return rows, fails


def fmt(p, c, key):
    x, y = p.get(key, 0), c.get(key, 0)
    return str(x) if x == y else f"{x} -> {y}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listings", nargs="+", help="parent.s change.s pairs")
    ap.add_argument("--md", help="write the report here as well")
    ap.add_argument("--brief", action="store_true", help="rows only for kernels that fail or whose register counts moved")
    args = ap.parse_args()
    if len(args.listings) % 2:
        ap.error("listings come in (parent, change) pairs")
    lines, all_fails = [], []
    for parent_path, change_path in zip(args.listings[::2], args.listings[1::2]):
        rows, fails = compare(parent_path, change_path)
        all_fails += fails
        moved = [r for r in rows if r[1].get("vgpr") != r[2].get("vgpr") or r[1].get("agpr") != r[2].get("agpr")]
        lines += [f"## {change_path.split('/')[-1]} against {parent_path.split('/')[-1]}", "",
                  f"{len(rows)} kernels; {len(fails)} failures; register counts moved in {len(moved)}"
                  + ("; the kernels not listed have the parent's figures in every column." if args.brief else "."), "",
                  "| kernel | scratch | occupancy | LDS bytes | VGPRs | AGPRs | vfloat / matrix / vmem (lds) | verdict |", "|---|---|---|---|---|---|---|---|"]
        for name, p, c, per_class, bad in rows:
            if args.brief and not bad and (name, p, c, per_class, bad) not in moved:
                continue
            hist = " / ".join(str(per_class[k]) for k in ("vfloat", "matrix", "vmem")) + f" ({per_class['lds']})"
            lines.append(f"| `{name}` | {fmt(p, c, 'scratch')} | {fmt(p, c, 'occ')} | {fmt(p, c, 'lds')} | {fmt(p, c, 'vgpr')} | {fmt(p, c, 'agpr')} | "
                         f"{hist} | {'FAIL: ' + '; '.join(bad) if bad else 'same'} |")
        lines.append("")
    lines += ["## Verdict", "", "FAIL:" if all_fails else "Every kernel: scratch 0, occupancy not lower, LDS bytes equal, histograms identical."]
    lines += [f"- {f}" for f in all_fails]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.md:
        open(args.md, "w").write(text)
    return 1 if all_fails else 0


if __name__ == "__main__":
    sys.exit(main())
