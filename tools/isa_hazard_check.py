#!/usr/bin/env python3
"""ISA check for the hand-issued asynchronous loads of the conv prologue (vq_assign_filter_kernel<256, SEL, true, false, RES> and the
small-batch vq_assign_filter_split_kernel<256, SEL, true, false, false, RES>; one report line per kernel and SEL covers both seed
forms RES): the x values of
k-step g are loaded with `asm volatile("global_load_dword ... nt")` three k-steps before they are used and waited for with a COUNTED
s_waitcnt; hipcc believes the destination registers are defined at the asm statement, so nothing it schedules between the load and
its covering wait may read, copy, spill or overwrite them.  The 8 loads of group g are covered by the (g + 1)-th vmcnt wait after
the first load (compiler-inserted waits in between only make the counted ones stricter).  Run by __graft_entry__.build().
  python tools/isa_hazard_check.py [file.s]      (without an argument: compiles the two D = 256 pass-1 units, csrc/vq_pass1_d256.hip and
                                                  csrc/vq_pass1_d256_res.hip, which hold these kernels, to gfx950 assembly first)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assemble(out_path):
    """the assembly of both units, one behind the other, in out_path (the two compiles run side by side)"""
    units = ["vq_pass1_d256.hip", "vq_pass1_d256_res.hip"]
    procs = [subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                               "--cuda-device-only", "-S", "-o", out_path + "." + u,
                               os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc", u)], stderr=subprocess.DEVNULL) for u in units]
    for u, p in zip(units, procs):
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, p.args)
    with open(out_path, "w") as out:
        for u in units:
            out.write(open(out_path + "." + u).read())


def regs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def check(path):
    s = open(path).read()
    names = [l.split(":")[0] for l in s.splitlines()
             if re.match(r"_Z23vq_assign_filter_kernelILi256ELi[01]ELb1ELb0ELb[01]EE.*:", l)]   # <256, SEL, CONV = true, FOLD = false, RES>
    assert len(names) == 4, "expected the SEL = 0 / 1 CONV instantiations of vq_assign_filter_kernel in both seed forms, found %r" % names
    split = sorted({l.split(":")[0] for l in s.splitlines()               # the small-batch form with the same prologue
                    if re.match(r"_Z29vq_assign_filter_split_kernelILi256ELi[01]ELb1ELb0ELb0ELb[01]EE.*:", l)})   # <256, SEL, CONV, !FOLD, !FLAT, RES>
    assert len(split) == 4, "expected the SEL = 0 / 1 CONV instantiations of vq_assign_filter_split_kernel in both seed forms, found %r" % split
    names = sorted(names) + split
    report = []
    for name in names:
        i = s.index("\n" + name + ":")
        j = s.index(".Lfunc_end", i)
        body = [l.split("//")[0].split(";")[0].strip() for l in s[i:j].splitlines()]
        body = [l for l in body if l and not l.startswith(".")]
        loads = [k for k, l in enumerate(body) if re.match(r"global_load_dword \S+ \S+ off nt", l.replace(",", ""))]
        assert len(loads) == 128, (name, len(loads))
        waits = [k for k, l in enumerate(body) if l.startswith("s_waitcnt") and "vmcnt" in l and k > loads[0]]
        bad = 0
        for idx, k in enumerate(loads):
            cover = waits[idx // 8]
            assert cover > k, (name, idx)
            dst = regs(body[k].split()[1].rstrip(","))
            for l2 in body[k + 1:cover]:
                touched = set()
                for o in l2.replace(",", " ").split()[1:]:
                    touched |= regs(o)
                if touched & dst:
                    print("HAZARD in %s: %s -> %s" % (name[:48], body[k], l2))
                    bad += 1
        counted = [body[w] for w in waits[:16]]
        ok_counts = counted == ["s_waitcnt vmcnt(24)"] * 14 + ["s_waitcnt vmcnt(12)", "s_waitcnt vmcnt(0)"]
        if not ok_counts:
            print("unexpected wait sequence in %s: %s" % (name[:48], counted))
        report.append((name, bad, ok_counts))
    # one line per kernel and SEL: its two seed forms (the last template argument) share the prologue under test, and the report's
    # readers (tests/test_abi_and_host.py, build()) count one line per kernel and SEL; every hazard and every unexpected wait
    # sequence was printed above with its own kernel's name
    family = {}
    for name, bad, okc in report:
        key = re.sub(r"ELb[01]EE", "ELb*EE", name, count=1)
        b0, o0 = family.get(key, (0, True))
        family[key] = (b0 + bad, o0 and okc)
    return [(k, b, o) for k, (b, o) in sorted(family.items())]


def main():
    if len(sys.argv) > 1:
        rep = check(sys.argv[1])
    else:
        with tempfile.TemporaryDirectory() as td:
            p = os.path.join(td, "vq_pass1_d256.s")
            assemble(p)
            rep = check(p)
    for name, bad, okc in rep:
        print("%s: %d hazards, counted waits %s" % (name[:60], bad, "as placed" if okc else "NOT as placed"))
    sys.exit(1 if any(b or not o for _, b, o in rep) else 0)


if __name__ == "__main__":
    main()
