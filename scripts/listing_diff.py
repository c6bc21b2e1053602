#!/usr/bin/env python3
"""Kernel by kernel, the device listings of two checkouts compared, without a GPU: `hipcc -S --cuda-device-only` of csrc/render.hip
and csrc/adaptive.hip (or the files of --files) with the build's flags (scripts/kernel_asm.py's compile, one per file and tree), then for every kernel whether
the instruction stream is the same text (comments dropped, labels renumbered) and what the compiler reports for it.  A stream that
differs only in the immediate offsets of scalar loads and the kernel-argument size -- what a kernel-argument block that grew moves --
is reported as "kernarg size and s_load offsets only", with the numbers that changed.
usage: scripts/listing_diff.py <parent checkout> [<branch checkout>] [--keep dir] [--files a.hip,b.hip] > table.md
   --keep dir: keep the listings and the remarks there (and reuse the ones already there)
   --files:    the files of flux_amd/csrc to compare instead of render.hip,adaptive.hip
Exit status 1 if a kernel exists in one tree only."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import importlib.util
spec = importlib.util.spec_from_file_location("_b", os.path.join(ROOT, "flux_amd", "build.py"))
b = importlib.util.module_from_spec(spec)
spec.loader.exec_module(b)

FILES = ("render.hip", "adaptive.hip")
KEYS = (("vgprs", r"^VGPRs: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"),
        ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"))


def listing(tree, name, keep):
    """(assembly text, remarks) of tree/flux_amd/csrc/name"""
    csrc = os.path.join(os.path.abspath(tree), "flux_amd", "csrc")
    asm, rem = os.path.join(keep, name + ".s"), os.path.join(keep, name + ".remarks")
    if not (os.path.exists(asm) and os.path.exists(rem)):
        flags = [f for f in b.HIP_FLAGS if f not in ("-shared", "-fPIC")]
        p = subprocess.run([b._hipcc()] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", asm,
                                                   os.path.join(csrc, name)], capture_output=True, text=True, cwd=csrc)
        if p.returncode:
            sys.exit(p.stderr[-4000:])
        with open(rem, "w") as f:
            f.write(p.stderr)
    return open(asm).read(), open(rem).read()


def kernels(tree, keep, files):
    """demangled name -> (normalised instruction stream, resources)"""
    out = {}
    for name in files:
        text, remarks = listing(tree, name, keep)
        syms = re.findall(r"^\s*\.globl\s+(_Z\S+)", text, flags=re.M)
        dem = subprocess.run(["c++filt"] + syms, capture_output=True, text=True).stdout.splitlines()
        res, cur = {}, None
        for line in remarks.splitlines():
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                cur = res.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
            if m and cur is not None:
                for key, pat in KEYS:
                    v = re.search(pat, m.group(1).strip())
                    if v:
                        cur[key] = int(v.group(1))
        for sym, d in zip(syms, dem):
            start = text.index(f"\n{sym}:")
            body = text[start + 1:text.index(".Lfunc_end", start)]
            lines = []
            for ln in body.splitlines()[1:]:
                ln = re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), ln.split(";")[0]).strip()
                if ln:
                    lines.append(ln)
            out[d.split("(")[0]] = ("\n".join(lines), len([ln for ln in lines if not ln.endswith(":") and not ln.startswith(".")]), res.get(sym, {}))
    return out


SLOAD = re.compile(r"^(s_load_\w+\s+.*,\s*|\.amdhsa_kernarg_size\s+)(0x[0-9a-f]+|\d+)$")


def masked(stream):
    """(the stream with every scalar load's immediate offset and the kernel-argument size masked, those numbers in order)"""
    lines, offs = [], []
    for ln in stream.splitlines():
        m = SLOAD.match(ln)
        if m:
            offs.append(m.group(2))
            ln = m.group(1) + "IMM"
        lines.append(ln)
    return "\n".join(lines), offs


def verdict(pa, ba):
    if pa == ba:
        return "identical"
    (pm, po), (bm, bo) = masked(pa), masked(ba)
    if pm != bm:
        return "DIFFERS"
    moved = sorted({f"{a} -> {b}" for a, b in zip(po, bo) if a != b})
    return "kernarg size and s_load offsets only (" + ", ".join(moved) + ")"


def main():
    args = sys.argv[1:]
    keep = None
    if "--keep" in args:
        k = args.index("--keep")
        keep = os.path.abspath(args[k + 1])
        del args[k:k + 2]
    files = FILES
    if "--files" in args:
        k = args.index("--files")
        files = args[k + 1].split(",")
        del args[k:k + 2]
    trees = [args[0], args[1] if len(args) > 1 else ROOT]
    with tempfile.TemporaryDirectory() as td:
        sides = []
        for side, tree in zip(("parent", "branch"), trees):
            d = os.path.join(keep or td, side)
            os.makedirs(d, exist_ok=True)
            sides.append(kernels(tree, d, files))
    parent, branch = sides
    fmt = lambda r, n: "{} / {} / {} / {} / {} / {}".format(r.get("vgprs"), r.get("vgpr_spill"), r.get("sgpr_spill"), r.get("scratch"), r.get("occupancy"), n)  # noqa: E731
    print("| kernel | stream | parent: VGPRs / VGPR spills / SGPR spills / scratch B / occupancy / instructions | branch: the same |")
    print("|---|---|---|---|")
    same = offsets = 0
    for name in sorted(set(parent) | set(branch)):
        if name not in parent or name not in branch:
            print(f"| `{name}` | only in {'parent' if name in parent else 'branch'} | | |")
            continue
        (pa, pn, pr), (ba, bn, br) = parent[name], branch[name]
        v = verdict(pa, ba)
        same += v == "identical"
        offsets += v.startswith("kernarg")
        print(f"| `{name}` | {v} | {fmt(pr, pn)} | {fmt(br, bn)} |")
    print(f"\n{len(parent)} kernels in the parent, {len(branch)} in the branch, {same} with an identical instruction stream, "
          f"{offsets} that differ in the kernel-argument size and scalar-load offsets only.")
    return 0 if set(parent) == set(branch) else 1


if __name__ == "__main__":
    sys.exit(main())
