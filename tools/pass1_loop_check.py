#!/usr/bin/env python3
"""ISA check and instruction counts of the code loop bodies of the staged routed pass 1 at D = 256 (csrc/pass1_loop.h as included by
csrc/dvq_pass1.h: vq_assign_filter_kernel / vq_assign_filter_cached_kernel <256, 2, ...>: the long form, the short form of a wave
that scores one column group, and the form of a wave with no column group, which keeps the ring's protocol alone).  The A fragments and the accumulator seeds are read with `asm volatile("ds_read_b128 ...")` ahead of
their use and waited for with COUNTED `s_waitcnt lgkmcnt(n)`; hipcc believes the destination registers are defined at the asm
statement, so nothing it schedules between a read and the wait that covers it may touch them.  LDS reads of a wave return in order:
a wait for lgkmcnt(n) leaves the n youngest outstanding.  The scan walks every innermost loop block that holds v_mfma, keeps the
list of outstanding reads, and reports an instruction that names a register of one of them; a body must end with none outstanding.
  python tools/pass1_loop_check.py [file.s] [-o out.json]    (without a file: compiles csrc/vq_pass1_d256_res.hip and
                                                              csrc/vq_pass1_d256.hip to gfx950 assembly first)
A workgroup's waves take different forms, and a barrier that one wave skips hangs the workgroup: every body must hold exactly ONE
s_barrier and the same counted vmcnt wait in front of it, and every barrier in front of the loop (the prologue: branch images, one per
k-step pair of the operand exchange, the ring hand-over) must sit where all waves pass -- full exec mask, not jumped over by a branch.
Prints a JSON object {kernel symbol: {"bodies": [per loop body: counts, hazards], "prologue_barriers": n, ...}}; exit status 1 on a
hazard, a body without exactly one barrier, or a prologue barrier under a narrowed exec mask / behind a forward branch."""
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_hazard_check import assemble, regs  # noqa: E402


def loop_bodies(s, name):
    i = s.index("\n" + name + ":")
    j = s.index(".Lfunc_end", i)
    lines = [l.split(";")[0].split("//")[0].strip() for l in s[i:j].splitlines()]
    blocks, cur = [], None
    for l in lines:
        if not l:
            continue
        if re.match(r"\.LBB\d+_\d+:", l):
            cur = [l[:-1]]
            blocks.append(cur)
        elif cur is not None and not l.startswith("."):
            cur.append(l)
    return [b[1:] for b in blocks if any(l == "s_barrier" for l in b) and
            any(l.startswith("s_cbranch") and l.split()[-1] == b[0] for l in b)]


def prologue_barriers(s, name):
    """the barriers in front of the first tile barrier (the first one behind a counted `s_waitcnt vmcnt(n)`, n > 0):
    -> (count, under a narrowed exec mask, jumped over by a forward branch that does not come back in front of them)"""
    i = s.index("\n" + name + ":")
    j = s.index(".Lfunc_end", i)
    lines = [l.split(";")[0].split("//")[0].strip() for l in s[i:j].splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or re.match(r"\.LBB\d+_\d+:", l))]
    label = {l[:-1]: k for k, l in enumerate(lines) if l.endswith(":")}
    first_tile = None
    for k, l in enumerate(lines):
        if l == "s_barrier" and any(re.match(r"s_waitcnt vmcnt\([1-9]\d*\)$", x) for x in lines[max(0, k - 3):k]):
            first_tile = k
            break
    assert first_tile is not None, "no tile barrier in " + name
    depth, masked, bars = 0, 0, []
    for k, l in enumerate(lines[:first_tile]):
        if "saveexec" in l and "andn2_saveexec" not in l and "or_saveexec" not in l:
            depth += 1
        elif re.match(r"s_or_b64 exec, exec,", l):
            depth = max(0, depth - 1)
        elif l == "s_barrier":
            bars.append(k)
            masked += depth > 0
    def comes_back(t, limit):
        for l in lines[t:]:                                           # the target block up to its unconditional exit
            if l.startswith("s_branch"):
                return label[l.split()[-1]] <= limit
            if l.startswith("s_endpgm"):
                return False
        return False
    skipped = 0
    for b in bars:
        for k, l in enumerate(lines[:b]):
            if l.startswith(("s_cbranch", "s_branch")):
                t = label[l.split()[-1]]
                if t > b and not comes_back(t, b):
                    skipped += 1
    return len(bars), masked, skipped


def check(path):
    s = open(path).read()
    out, bad = {}, 0
    for name in sorted(set(re.findall(r"^(_Z\d+vq_assign_filter(?:_cached)?_kernelILi256ELi2E\w+):", s, re.M))):
        rows = []
        for body in loop_bodies(s, name):
            outstanding, haz = [], 0
            for l in body:
                ops = l.replace(",", " ").split()
                touched = set()
                for o in ops[1:]:
                    touched |= regs(o)
                for dst, src in outstanding:
                    if touched & dst:
                        print("HAZARD in %s: %s -> %s" % (name[:48], src, l), file=sys.stderr)
                        haz += 1
                if ops[0].startswith("ds_read"):
                    outstanding.append((regs(ops[1]), l))
                m = re.search(r"lgkmcnt\((\d+)\)", l)
                if ops[0] == "s_waitcnt" and m:
                    n = int(m.group(1))
                    outstanding = outstanding[len(outstanding) - n:] if n else []
            rows.append({"total": len(body), "global_load_lds": sum("global_load_lds" in l for l in body),
                         "s_barrier": sum(l == "s_barrier" for l in body),
                         "vmcnt_waits": [int(m.group(1)) for l in body for m in [re.match(r"s_waitcnt vmcnt\((\d+)\)$", l)] if m],
                         "salu": sum(l.startswith("s_") for l in body),
                         "valu_non_mfma": sum(l.startswith("v_") and not l.startswith("v_mfma") for l in body),
                         "mfma": sum(l.startswith("v_mfma") for l in body),
                         "ds_read_b128": sum(l.startswith("ds_read_b128") for l in body),
                         "hazards": haz, "outstanding_at_end": len(outstanding)})
            bad += haz + len(outstanding) + (rows[-1]["s_barrier"] != 1)
        assert sorted(r["mfma"] for r in rows) == [0, 16, 32], \
            "expected the loop bodies of 0, 1 and 2 column groups in %s, found %r" % (name, [r["mfma"] for r in rows])
        assert len({tuple(r["vmcnt_waits"]) for r in rows}) == 1 and len({r["global_load_lds"] for r in rows}) == 1, \
            "the forms of %s differ in their counted waits or DMA pieces" % name
        nbar, masked, skipped = prologue_barriers(s, name)
        bad += masked + skipped
        out[name] = {"bodies": rows, "prologue_barriers": nbar, "prologue_barriers_under_exec_mask": masked,
                     "prologue_barriers_behind_a_forward_branch": skipped}
    assert len(out) == 8, "expected the 8 SEL == 2 kernels of the two D = 256 units, found %d" % len(out)
    return out, bad


def main():
    args = [a for a in sys.argv[1:]]
    dst = None
    if "-o" in args:
        dst = args[args.index("-o") + 1]
        del args[args.index("-o"):args.index("-o") + 2]
    if args:
        rep, bad = check(args[0])
    else:
        with tempfile.TemporaryDirectory() as td:
            p = os.path.join(td, "vq_pass1_d256.s")
            assemble(p)
            rep, bad = check(p)
    text = json.dumps(rep, indent=1)
    print(text)
    if dst:
        open(dst, "w").write(text + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
