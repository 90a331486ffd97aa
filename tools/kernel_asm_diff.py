#!/usr/bin/env python3
"""Device-code diff of two source trees: every meant_amd/csrc/*.hip of each tree is compiled to gfx950 assembly with the
Makefile's flags, the assembly is split per kernel symbol across the whole library (kernels may move between files), and
each kernel's instruction text and .amdhsa_kernel descriptor are compared by name after comments are stripped and the
function ordinal in local labels is normalised.

    tools/kernel_asm_diff.py OLD_TREE NEW_TREE [-j JOBS]

Prints the kernels only in OLD, only in NEW, and the ones that differ; exit status 1 if any list is non-empty.  A host-side
refactor must leave all three lists empty.  A kernel only in OLD and one only in NEW whose text and descriptor are equal once each
kernel's own symbol is replaced by a placeholder (a kernel that gained a template argument keeps its code under a new mangled name)
are listed as "renamed, same code" instead and do not count.  The comparison is textual: no instruction is looked for or interpreted."""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# CXXFLAGS of meant_amd/csrc/Makefile, then what turns the compile into a device-only listing
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-S", "--cuda-device-only"]
NO_SLP = ("attn_bf16.hip", "attn_bwd1.hip")            # as in the Makefile

_ORDINAL = re.compile(r"\.(LBB|Ltmp|Lfunc_[A-Za-z]+)\d+")
_TYPE = re.compile(r"^\s*\.type\s+([^\s,]+)\s*,\s*@function")
_LABEL = re.compile(r"^([^\s:]+):\s*$")
_SIZE = re.compile(r"^\s*\.size\s+([^\s,]+)\s*,")
_DESC_BEGIN = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_DESC_END = re.compile(r"^\s*\.end_amdhsa_kernel")


def _clean(line):
    """one line without its ';' comment and trailing blanks, local-label ordinals replaced; '' if nothing is left"""
    line = line.split(";", 1)[0].rstrip()
    if not line.strip():
        return ""
    return _ORDINAL.sub(lambda m: "." + m.group(1) + "#", " ".join(line.split()))


def split_kernels(text):
    """{symbol: (body lines, descriptor lines)} of one assembly listing; __hip_cuid_* symbols and everything outside a function
    or a descriptor (file-level directives, the metadata list) are left out"""
    bodies, descs = {}, {}
    pending, cur, desc = None, None, None
    for raw in text.splitlines():
        m = _DESC_BEGIN.match(raw)
        if m:
            desc = m.group(1)
            descs[desc] = []
            continue
        if desc is not None:
            if _DESC_END.match(raw):
                desc = None
            elif _clean(raw):
                descs[desc].append(_clean(raw))
            continue
        m = _TYPE.match(raw)
        if m:
            pending = m.group(1)
            continue
        m = _LABEL.match(raw.split(";", 1)[0].rstrip())
        if m and pending is not None and m.group(1) == pending:
            cur, pending = m.group(1), None
            bodies[cur] = []
            continue
        m = _SIZE.match(raw)
        if m and m.group(1) == cur:
            cur = None
            continue
        if cur is not None and _clean(raw):
            bodies[cur].append(_clean(raw))
    names = (set(bodies) | set(descs))
    return {n: (bodies.get(n, []), descs.get(n, [])) for n in names if not n.startswith("__hip_cuid_")}


def diff_kernels(old, new):
    """(only in old, only in new, differing) symbol lists of two split_kernels() results (or unions of them)"""
    only_old = sorted(set(old) - set(new))
    only_new = sorted(set(new) - set(old))
    differ = sorted(n for n in set(old) & set(new) if old[n] != new[n])
    return only_old, only_new, differ


def pair_renamed(old, new, only_old, only_new):
    """[(old symbol, new symbol)]: kernels of the two one-sided lists whose code is equal apart from their own symbol (which the
    body names in its `.section .text.<symbol>` line and the descriptor in its operands); equal candidates pair in sorted order"""
    def anonymous(name, entry):
        return tuple(tuple(line.replace(name, "<self>") for line in part) for part in entry)
    by_code = {}
    for n in only_new:
        by_code.setdefault(anonymous(n, new[n]), []).append(n)
    pairs = []
    for o in only_old:
        same = by_code.get(anonymous(o, old[o]))
        if same:
            pairs.append((o, same.pop(0)))
    return pairs


def first_difference(a, b):
    """the first differing line pair of two (body, descriptor) entries, for the report"""
    for part, (x, y) in zip(("text", "descriptor"), zip(a, b)):
        for i in range(max(len(x), len(y))):
            l, r = (x[i] if i < len(x) else "<end>"), (y[i] if i < len(y) else "<end>")
            if l != r:
                return f"{part} line {i}: `{l}` -> `{r}`"
    return ""


def compile_to_asm(path):
    cmd = [HIPCC] + FLAGS + (["-fno-slp-vectorize"] if os.path.basename(path) in NO_SLP else []) + [path, "-o", "-"]
    return subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=os.path.dirname(path)).stdout


def tree_kernels(tree, pool):
    files = sorted(glob.glob(os.path.join(tree, "meant_amd", "csrc", "*.hip")))
    if not files:
        sys.exit(f"{tree}: no meant_amd/csrc/*.hip")
    return files, [pool.submit(compile_to_asm, f) for f in files]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-j", "--jobs", type=int, default=16)
    args = ap.parse_args()
    sides = []
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(args.jobs, 16))) as pool:
        pending = [tree_kernels(os.path.abspath(t), pool) for t in (args.old, args.new)]
        for files, futures in pending:
            kernels = {}
            for f, fut in zip(files, futures):
                for name, entry in split_kernels(fut.result()).items():
                    if name in kernels and kernels[name] != entry:
                        sys.exit(f"{f}: {name} is defined twice with different code")
                    kernels[name] = entry
            sides.append(kernels)
    old, new = sides
    only_old, only_new, differ = diff_kernels(old, new)
    renamed = pair_renamed(old, new, only_old, only_new)
    only_old = [n for n in only_old if n not in {o for o, _ in renamed}]
    only_new = [n for n in only_new if n not in {c for _, c in renamed}]
    print(f"renamed, same code: {len(renamed)}")
    for o, c in renamed:
        print(f"  {o} -> {c}")
    for title, names in (("only in old", only_old), ("only in new", only_new)):
        print(f"{title}: {len(names)}")
        for n in names:
            print("  " + n)
    print(f"differ: {len(differ)}")
    for n in differ:
        print(f"  {n}: {first_difference(old[n], new[n])}")
    print(f"kernel_asm_diff: {len(old)} kernels old, {len(new)} new, {len(renamed)} renamed with the same code, {len(only_old)} only old, "
          f"{len(only_new)} only new, {len(differ)} differ")
    return 1 if (only_old or only_new or differ) else 0


if __name__ == "__main__":
    sys.exit(main())
