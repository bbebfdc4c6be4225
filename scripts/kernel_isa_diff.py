#!/usr/bin/env python3
"""Compare the gfx950 code that two source trees compile to, kernel by
kernel — the check for a refactor that must not change device code.

  python scripts/kernel_isa_diff.py PARENT_TREE RESULT_TREE > profiles/...md

Every bdbnn_amd/csrc/*.hip of both trees is compiled to assembly
(--cuda-device-only -S), the text is split by function symbol, and
comments, directives and the per-function index of local labels are
stripped.  Per symbol the report says SAME, or DIFF with both instruction
counts and the resource figures the compiler prints next to the kernel;
symbols that only one tree has are listed separately.  A symbol is known
by its demangled name without the parameter list, so renaming the type of
a kernel argument does not orphan the kernel.  It compares trees and
nothing else.  Runs on a CPU-only builder (hipcc cross-compiles).
"""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only",
         "-S", "-o", "-"]

# resource figures the compiler writes as comments after each kernel
RES = [("VGPR", r"; NumVgprs: (\d+)"), ("SGPR", r"; TotalNumSgprs: (\d+)"),
       ("scratch", r"; ScratchSize: (\d+)"),
       ("LDS", r"; LDSByteSize: (\d+)"), ("waves", r"; Occupancy: (\d+)")]


def sources(tree, only):
    src = glob.glob(os.path.join(tree, "bdbnn_amd/csrc/*.hip"))
    return {os.path.basename(s): s for s in src
            if not s.endswith("_hip.hip")
            and (not only or os.path.basename(s) in only)}


def compile_asm(path):
    p = subprocess.run([HIPCC] + FLAGS + [path], capture_output=True,
                       text=True, cwd=os.path.dirname(path))
    if p.returncode != 0:
        sys.exit(f"{path}: compile failed\n{p.stderr[-2000:]}")
    return p.stdout


def split_functions(asm):
    """{symbol: (normalised instruction lines, resource dict)}"""
    funcs, cur, name = {}, None, None
    lines = asm.splitlines()
    for n, raw in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", raw)
        if m and cur is None and not raw.startswith(".L"):
            if any(re.match(rf"\s*\.type\s+{re.escape(m.group(1))},@function",
                            l) for l in lines[max(0, n - 8):n]):
                name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", raw):
            res = {}
            for l in lines[n:n + 80]:
                for key, pat in RES:
                    mm = re.match(pat, l)
                    if mm and key not in res:
                        res[key] = mm.group(1)
            funcs[name] = (cur, res)
            cur = None
            continue
        line = raw.split(";")[0].strip()
        if not line or (line.startswith(".") and not line.startswith(".L")):
            continue
        # .LBB<function index>_<block> -> .LBB_<block>
        cur.append(re.sub(r"\.L([A-Za-z]+)\d+_(\d+)", r".L\1_\2", line))
    return funcs


def tree_functions(tree, jobs, only):
    srcs = sources(tree, only)
    with ThreadPoolExecutor(jobs) as ex:
        asms = list(ex.map(compile_asm, srcs.values()))
    out = {}
    for f, asm in zip(srcs, asms):
        for sym, v in split_functions(asm).items():
            out[(f, sym)] = v
    return out


def demangle(syms):
    filt = (shutil.which("llvm-cxxfilt", path="/opt/rocm/lib/llvm/bin")
            or shutil.which("llvm-cxxfilt") or shutil.which("c++filt"))
    if not syms or not filt:
        return {s: s for s in syms}
    p = subprocess.run([filt], input="\n".join(syms), capture_output=True,
                       text=True)
    names = p.stdout.splitlines()
    return {s: re.sub(r"^void ", "", re.sub(r"\(.*\)$", "", d))
            for s, d in zip(syms, names)}


def n_instr(body):
    return sum(1 for l in body if not l.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("result")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--only", nargs="*", metavar="FILE.hip",
                    help="compare these source files only")
    a = ap.parse_args()
    A = tree_functions(os.path.abspath(a.parent), a.j, a.only)
    B = tree_functions(os.path.abspath(a.result), a.j, a.only)
    dm = demangle(sorted({k[1] for k in list(A) + list(B)}))
    A = {(f, dm[sym]): v for (f, sym), v in A.items()}
    B = {(f, dm[sym]): v for (f, sym), v in B.items()}
    both = sorted(set(A) & set(B))
    same = [k for k in both if A[k][0] == B[k][0]]
    diff = [k for k in both if A[k][0] != B[k][0]]
    print("# Kernel ISA diff (gfx950, hipcc -O3 --cuda-device-only -S)\n")
    print(f"{len(both)} symbols in both trees: {len(same)} SAME, "
          f"{len(diff)} DIFF.\n")
    for title, keys in (("Only in the parent", sorted(set(A) - set(B))),
                        ("Only in the result", sorted(set(B) - set(A)))):
        print(f"## {title}\n")
        for f, s in keys:
            print(f"- {f}: `{s}`")
        if not keys:
            print("none")
        print()
    print("## DIFF (parent -> result)\n")
    if diff:
        print("| file | kernel | instructions | VGPR | SGPR | scratch | LDS "
              "| waves/SIMD |")
        print("|---|---|---|---|---|---|---|---|")
    else:
        print("none\n")
    for k in diff:
        (ba, ra), (bb, rb) = A[k], B[k]
        cols = [f"{ra.get(key, '?')} -> {rb.get(key, '?')}"
                if ra.get(key) != rb.get(key) else f"{ra.get(key, '?')}"
                for key, _ in RES]
        print(f"| {k[0]} | `{k[1]}` | {n_instr(ba)} -> {n_instr(bb)} | "
              + " | ".join(cols) + " |")
    print("\n## SAME\n")
    print("| file | kernel | instructions |")
    print("|---|---|---|")
    for k in same:
        print(f"| {k[0]} | `{k[1]}` | {n_instr(A[k][0])} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
