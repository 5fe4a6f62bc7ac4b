#!/usr/bin/env python
"""Compare two gfx950 assembly listings of one translation unit function by function (no GPU: a compile is not a run).

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S sweep.hip -o side.s      (once per side)
    python tools/asm_compare.py parent.s branch.s [substring of the kernels to tabulate, ...]

Per function the instruction stream is what is left after comments, directives and blank lines are dropped and the
function's number is taken out of its block labels (.LBB<n>_<k> -> .LBB_<k>).  Prints how many functions are identical,
names every function that is not, and for those whose demangled name contains one of the substrings a table: lines,
VGPR / SGPR / scratch / LDS (the .amdhsa_ lines of the kernel descriptor) and the mnemonics whose counts differ."""
import collections
import re
import shutil
import subprocess
import sys

RES = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("scratch", "private_segment_fixed_size"),
       ("lds", "group_segment_fixed_size"))


def functions(path):
    """{name: (instruction lines, {resource: value})}"""
    out, res, cur, kern = {}, collections.defaultdict(dict), None, None
    for raw in open(path):
        line = raw.split(";")[0].strip()
        if not line:
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kern = m.group(1)
        m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", line)
        if m and kern:
            res[kern][m.group(1)] = m.group(2)
        m = re.match(r"(\w+):$", line)
        if m and not line.startswith(".L"):
            cur = m.group(1)
            out[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        if cur is None or (line.startswith(".") and not line.endswith(":")):
            continue
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return {k: (v, res.get(k, {})) for k, v in out.items() if v}


def mnemonics(lines):
    return collections.Counter(l.split()[0] for l in lines if not l.endswith(":"))


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    want = sys.argv[3:]
    names = sorted(set(a) | set(b))
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")      # (without one the names stay mangled)
    dem = dict(zip(names, subprocess.run([filt], input="\n".join(names), capture_output=True,
                                         text=True).stdout.splitlines() if filt else names))
    short = lambda n: re.sub(r"^void |\(.*$", "", dem[n])
    same = [n for n in names if n in a and n in b and a[n][0] == b[n][0]]
    print("functions: %d in the first listing, %d in the second, %d identical" % (len(a), len(b), len(same)))
    for n in names:
        if n in same:
            continue
        if n not in a or n not in b:
            print("ONLY IN ONE LISTING  %s" % short(n))
            continue
        tab = any(w in dem[n] for w in want)
        print("%s  %s" % ("differs" if tab else "DIFFERS (not expected)", short(n)))
        if not tab:
            continue
        ca, cb = mnemonics(a[n][0]), mnemonics(b[n][0])
        print("    lines %d -> %d   %s" % (len(a[n][0]), len(b[n][0]), "   ".join(
            "%s %s -> %s" % (k, a[n][1].get(f, "?"), b[n][1].get(f, "?")) for k, f in RES)))
        d = ["%s %+d" % (k, cb[k] - ca[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]]
        print("    mnemonics: %s" % (", ".join(d) if d else "the same count of every mnemonic (registers or order differ)"))
    print("tabulated kernels that are identical:")
    for n in same:
        if any(w in dem[n] for w in want):
            print("    %s  lines %d   %s" % (short(n), len(a[n][0]), "   ".join(
                "%s %s" % (k, a[n][1].get(f, "?")) for k, f in RES)))


if __name__ == "__main__":
    main()
