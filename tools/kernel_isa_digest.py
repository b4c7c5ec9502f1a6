#!/usr/bin/env python3
"""Per-kernel digests of the gfx950 ISA of every unit in csrc/, to show that a change which only MOVES code (between translation
units, into headers) left every kernel's machine code as it was.  No GPU needed.

  tools/kernel_isa_digest.py digest [csrc dir] -o digest.json [-j N]
      compiles every *.hip of the directory (default: this tree's csrc/) with the Makefile's CXXFLAGS plus `--cuda-device-only -S`,
      twice: as the product ("plain") and with -DDVQ_TUNING ("tuning"); cuts the assembly at every kernel symbol -- its code from
      `name:` to the function's `.Lfunc_end`, and its `.amdhsa_kernel` descriptor block -- drops what depends only on the
      position in the file (the function number in local labels such as .LBB12_3, comments) and hashes the rest (sha256).
      A kernel symbol that two units define is an error.
  tools/kernel_isa_digest.py compare before.json after.json -o table.json
      the table, a row per kernel symbol: the unit it lives in after and, per build, the hash before and after; exit status 1
      unless the two symbol sets are equal and every hash is.

It hashes and compares; it looks for no particular instruction."""
import argparse
import concurrent.futures
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"plain": [], "tuning": ["-DDVQ_TUNING"]}


def makefile_flags(csrc):
    out = subprocess.check_output(["make", "-s", "-C", csrc, "--eval", "print-flags: ; @echo $(HIPCC) $(CXXFLAGS)", "print-flags"], text=True)
    return out.split()


def kernels_of(asm):
    """{symbol: sha256 of the kernel's normalised code and descriptor}"""
    lines = asm.split("\n")
    start = {}
    for i, l in enumerate(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):", l)
        if m and not l.startswith(".L"):
            start[m.group(1)] = i
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        name = m.group(1)
        j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
        s = start[name]
        e = next(k for k in range(s, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[k]))
        text = []
        for t in lines[s:e + 1] + lines[i:j + 1]:
            t = t.split(";")[0].strip()                       # (a comment behind a label is padded to a column: position again)
            if not t or t.startswith("//"):
                continue
            text.append(re.sub(r"(\.L[A-Za-z_]*[A-Za-z])\d+", r"\1#", t))
        assert name not in out, name
        out[name] = hashlib.sha256("\n".join(text).encode()).hexdigest()
    return out


def compile_unit(cmd, src, extra):
    with tempfile.TemporaryDirectory() as td:
        s = os.path.join(td, "unit.s")
        subprocess.check_call(cmd + extra + ["--cuda-device-only", "-S", "-o", s, src], stderr=subprocess.DEVNULL)
        return kernels_of(open(s).read())


def digest(csrc, jobs):
    cmd = makefile_flags(csrc)
    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    res = {mode: {} for mode in MODES}
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        futs = {pool.submit(compile_unit, cmd, os.path.join(csrc, u), extra): (mode, u)
                for mode, extra in MODES.items() for u in units}
        for fut in concurrent.futures.as_completed(futs):
            mode, u = futs[fut]
            for sym, h in fut.result().items():
                if sym in res[mode]:
                    sys.exit("%s build: %s is defined by %s and by %s" % (mode, sym, res[mode][sym]["unit"], u))
                res[mode][sym] = {"sha256": h, "unit": u}
    return res


def compare(before, after):
    """one row per kernel symbol: the unit it lives in after, and per build [hash before, hash after] (the first 16 hex digits)"""
    rows, ok = [], True
    for sym in sorted({s for d in (before, after) for m in MODES for s in d[m]}):
        row = {"symbol": sym, "unit": next((after[m][sym]["unit"] for m in MODES if sym in after[m]), None)}
        for m in MODES:
            row[m] = [d[m][sym]["sha256"][:16] if sym in d[m] else None for d in (before, after)]
            if row[m][0] != row[m][1]:
                ok = False
                print("%s build: %s differs (%s -> %s)" % (m, sym, row[m][0], row[m][1]))
        rows.append(row)
    for m in MODES:
        print("%s build: %d kernels, %d identical" % (m, sum(r[m] != [None, None] for r in rows),
                                                       sum(r[m][0] == r[m][1] and r[m][0] is not None for r in rows)))
    return rows, ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("digest")
    d.add_argument("csrc", nargs="?", default=os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc"))
    d.add_argument("-o", required=True)
    d.add_argument("-j", type=int, default=8)
    c = sub.add_parser("compare")
    c.add_argument("before")
    c.add_argument("after")
    c.add_argument("-o", required=True)
    a = ap.parse_args()
    if a.cmd == "digest":
        json.dump(digest(a.csrc, a.j), open(a.o, "w"), indent=1, sort_keys=True)
        return
    table, ok = compare(json.load(open(a.before)), json.load(open(a.after)))
    with open(a.o, "w") as f:                                # a row per line
        f.write("[\n" + ",\n".join(json.dumps(r) for r in table) + "\n]\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
