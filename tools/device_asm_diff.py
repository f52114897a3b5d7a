"""Show that two csrc trees compile to the same gfx950 device code: device_asm_diff.py OLD_CSRC NEW_CSRC.

Every device translation unit of both trees is compiled to assembly with its Makefile's CXXFLAGS plus
--cuda-device-only -S, once as the product build (-DOAZ_AB=0) and once as the A/B build (-DOAZ_AB=1). What
differs between two compilations of the same code is taken out: the per-compilation __hip_cuid_ symbol, and
the mangled names, which change with a template parameter or a type's name and shift the substitution
indices inside other names, so each is replaced by its order of first appearance. The rest must be equal line
for line. Exit status 0: all ten comparisons equal; 1: a difference, its first lines printed per file.
--per-kernel splits a unit that differs at its function symbols and says of every kernel and device function
whether it is identical, different, only in the old or only in the new build (a unit that loses a kernel reads
"DIFFERENT" as a whole).
The assembly is read only to compare two builds."""
import argparse
import concurrent.futures
import os
import re
import shlex
import subprocess
import sys
import tempfile
from pathlib import Path

UNITS = ("oaz_gpu.hip", "oaz_train.hip", "oaz_pure_mcts.hip", "oaz_alphabeta.hip", "oaz_arena.hip")
MANGLED = re.compile(r"_Z[A-Za-z0-9_]+")
# .LBB<function>_<block>, .Lfunc_end<function> and a comment's BB<function>_<block>: the function's number in the unit
LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?|\bBB\d+_\d+")
BEGIN = re.compile(r"-- Begin function (\S+)")
META_NAME = re.compile(r"    \.name:\s+(\S+)")


def normalise(asm):
    """The lines of `asm` without those naming __hip_cuid_, every mangled name replaced by @<order of first
    appearance>."""
    order = {}
    return [MANGLED.sub(lambda m: "@%d" % order.setdefault(m.group(0), len(order)), line)
            for line in asm.splitlines() if "__hip_cuid_" not in line]


def compare(old_asm, new_asm, context=3):
    """None when the two assemblies are equal after normalise(); else a report of the first difference:
    its line number and the next `context` lines of either side."""
    a, b = normalise(old_asm), normalise(new_asm)
    if a == b:
        return None
    i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    out = ["first difference at normalised line %d (%d lines old, %d new)" % (i + 1, len(a), len(b))]
    out += ["  old| " + s for s in a[i:i + context]] + ["  new| " + s for s in b[i:i + context]]
    return "\n".join(out)


def split_functions(asm):
    """{symbol: lines} of `asm`, one entry per function (kernel or device function): its text from the section
    directive before its "-- Begin function" line to the next one's, and, for a kernel, its entry of the code
    object's metadata (the argument layout). "(rest of unit)" is what belongs to no function: the head and the tail of the file."""
    out, rest, cur, entry = {}, [], None, None
    for line in asm.splitlines():
        if "__hip_cuid_" in line:
            continue
        m = BEGIN.search(line)
        if m or (cur is not None and line.startswith(("\t.p2alignl", "\t.amdgpu_metadata"))):  # (else: the tail)
            prev = rest if cur is None else cur
            cur = out.setdefault(m.group(1), []) if m else None
            if prev and prev[-1].startswith(("\t.text", "\t.section")):  # the section directive of what follows
                (rest if cur is None else cur).append(prev.pop())
        if entry is not None and not line.startswith("    "):  # an entry of amdhsa.kernels ends: to its kernel
            out.setdefault(next(m.group(1) for m in map(META_NAME.match, entry) if m), []).extend(entry)
            entry = None
        if cur is None and line.startswith("  - ."):
            entry = []
        (entry if entry is not None else rest if cur is None else cur).append(line)
    out["(rest of unit)"] = rest
    return out


def function_key(sym):
    """What names the same function in both builds: the qualified name without its parameter types (which a
    changed signature changes), with the template arguments where they are integers: tr::k_conv<0,2,2>."""
    m = re.match(r"_ZN?", sym)
    if not m:
        return sym
    i, parts = m.end(), []
    while sym[i:i + 1].isdigit():
        n = re.match(r"\d+", sym[i:]).group(0)
        parts.append(sym[i + len(n):i + len(n) + int(n)])
        i += len(n) + int(n)
    if not parts:
        return sym
    t = re.match(r"I((?:L[a-z]\d+E)+)E", sym[i:])
    if t:
        return "::".join(parts) + "<" + ",".join(re.findall(r"L[a-z](\d+)E", t.group(1))) + ">"
    return "::".join(parts) + (" " + sym[i:] if sym[i:i + 1] == "I" else "")


def normalise_function(lines):
    """As normalise(), within one function: local labels are numbered by first appearance as well, and the
    padding in front of a comment, which follows a label's length, is one blank."""
    order = {}
    number = lambda m: "@%d" % order.setdefault(m.group(0), len(order))
    return [re.sub(r"\s+;", " ;", LOCAL.sub(number, MANGLED.sub(number, line))) for line in lines]


def compare_functions(old_asm, new_asm):
    """[(function, "identical" | "different" | "only in old" | "only in new")] in the old build's order, the
    new build's own functions last."""
    a = {function_key(k): normalise_function(v) for k, v in split_functions(old_asm).items()}
    b = {function_key(k): normalise_function(v) for k, v in split_functions(new_asm).items()}
    out = [(k, "only in old" if k not in b else "identical" if a[k] == b[k] else "different") for k in a]
    return out + [(k, "only in new") for k in b if k not in a]


def cxxflags(csrc, ab, extra):
    """CXXFLAGS of csrc/Makefile with its ARCH default, AB = ab and EXTRA = extra."""
    mk = (Path(csrc) / "Makefile").read_text()
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", mk, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    for var, val in (("ARCH", arch), ("AB", str(ab)), ("EXTRA", extra)):
        flags = flags.replace("$(%s)" % var, val)
    assert "$(" not in flags, flags
    return shlex.split(flags)


def compile_asm(hipcc, csrc, unit, ab, extra, out):
    cmd = [hipcc, *cxxflags(csrc, ab, extra), "--cuda-device-only", "-S", "-Wno-unused-command-line-argument", unit,
           "-o", str(out)]
    subprocess.run(cmd, cwd=csrc, check=True)
    return out.read_text()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_csrc")
    ap.add_argument("new_csrc")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--extra", default="", help="the Makefile's EXTRA (-D tunables) for both trees")
    ap.add_argument("--per-kernel", action="store_true", help="report every function of a unit that differs")
    ap.add_argument("-j", "--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    trees = {"old": os.path.abspath(a.old_csrc), "new": os.path.abspath(a.new_csrc)}
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        asm = {(side, unit, ab): pool.submit(compile_asm, a.hipcc, csrc, unit, ab, a.extra,
                                             Path(tmp) / ("%s_ab%d_%s.s" % (side, ab, unit)))
               for side, csrc in trees.items() for ab in (0, 1) for unit in UNITS}
        bad = 0
        for ab in (0, 1):
            for unit in UNITS:
                old, new = asm["old", unit, ab].result(), asm["new", unit, ab].result()
                diff = compare(old, new)
                print("%-20s -DOAZ_AB=%d  %s" % (unit, ab, "DIFFERENT" if diff else "identical"), flush=True)
                if diff:
                    print(diff, flush=True)
                    for name, verdict in compare_functions(old, new) if a.per_kernel else ():
                        print("    %-14s %s" % (verdict, name), flush=True)
                    bad += 1
    print("%d of %d comparisons differ" % (bad, 2 * len(UNITS)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
