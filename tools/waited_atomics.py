"""Returning global atomics and the full waits behind them in the batched path's kernels, from the gfx950 assembly.

usage: python tools/waited_atomics.py [--all] [--lines KERNEL] [--csrc DIR] [--asm FILE --remarks FILE] [--flags "..."]

Makes the device-only assembly build of tools/late_scalar_loads.py (the Makefile's flags, line tables, resource remarks) and prints
per kernel:
  returning = global / flat atomics that return a value (gfx950 marks them sc0)
  | waited = those followed, in the order of the text, by `s_waitcnt vmcnt(0)` before the next returning atomic (or the kernel's end)
  | at once = those whose vmcnt(0) stands within the next five instructions: a trip to memory that nothing overlaps
and the compiler's remark: VGPRs, SGPRs, scratch, occupancy.
A returning atomic that is waited for at once is a dependent trip of its wave; several in a row are as many trips (DESIGN.md §5:
returning atomics of one phase leave in one instruction and are issued ahead of their use).  The order of the text is not the order
of execution across branches: --lines KERNEL lists every returning atomic with its source line to read the cases by hand.
--csrc DIR builds another tree's mlmapping_amd/csrc (a checkout of the parent commit) with that tree's Makefile flags.
"""
import argparse
import re

import late_scalar_loads as lsl


def parse_kernel(body):
    insts = []  # (mnemonic, text, source location)
    loc = ""
    for line in body:
        s = line.strip()
        if not s or s.startswith(";"):
            continue
        if s.startswith(".loc"):
            c = s.split(";", 1)
            loc = c[1].strip() if len(c) > 1 else ""
            continue
        if s.startswith(".") or s.endswith(":"):
            continue
        text = s.split(";", 1)[0].strip()
        insts.append((text.split()[0], text, loc))

    def returning(op, text):
        return (op.startswith("global_atomic_") or op.startswith("flat_atomic_")) and re.search(r"\bsc0\b", text) is not None

    def full_wait(op, text):
        return op == "s_waitcnt" and "vmcnt(0)" in text

    at = [i for i, (op, text, _) in enumerate(insts) if returning(op, text)]
    waited = at_once = 0
    rows = []
    for n, i in enumerate(at):
        end = at[n + 1] if n + 1 < len(at) else len(insts)
        dist = next((j - i for j in range(i + 1, end) if full_wait(insts[j][0], insts[j][1])), None)
        waited += dist is not None
        at_once += dist is not None and dist <= 5
        rows.append(("%s %s" % ("*" if dist is not None and dist <= 5 else "w" if dist is not None else " ", insts[i][1]), insts[i][2]))
    return {"returning": len(at), "waited": waited, "at_once": at_once, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true", help="every kernel of the library, not only the batched path's")
    ap.add_argument("--lines", action="append", default=[], help="list the returning atomics of this kernel by source line (* = waited for at once, w = waited)")
    ap.add_argument("--csrc", help="another tree's mlmapping_amd/csrc")
    ap.add_argument("--asm")
    ap.add_argument("--remarks")
    ap.add_argument("--flags", default="", help="extra compiler flags (an experiment build's ALT_FLAGS)")
    a = ap.parse_args()
    if a.csrc:
        lsl.CSRC = a.csrc
    if a.asm:
        asm, rem = open(a.asm).read(), open(a.remarks).read() if a.remarks else ""
    else:
        asm, rem = lsl.compile_asm(a.flags.split())
    remarks = lsl.parse_remarks(rem)
    lines = asm.split("\n")
    amdhsa = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    kernels = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m and m.group(1) in amdhsa:
            j = i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            kernels[m.group(1)] = lines[i + 1:j]
            i = j
        i += 1
    names = lsl.demangle(list(kernels))
    print("%-34s %9s %7s %8s | %5s %5s %8s %5s" % ("kernel", "returning", "waited", "at once", "VGPRs", "SGPRs", "scratch", "occ"))
    for mangled, body in kernels.items():
        dn = names[mangled]
        if dn.startswith("void "):
            dn = dn[5:]
        if not a.all and not any(dn.startswith(b) for b in lsl.BATCHED):
            continue
        k = parse_kernel(body)
        r = remarks.get(mangled, {})
        print("%-34s %9d %7d %8d | %5s %5s %8s %5s" % (dn.split("(")[0], k["returning"], k["waited"], k["at_once"], r.get("VGPRs", "?"), r.get("TotalSGPRs", "?"),
                                                     r.get("ScratchSize [bytes/lane]", "?"), r.get("Occupancy [waves/SIMD]", "?")))
        if any(w in dn for w in a.lines):
            for text, loc in k["rows"]:
                print("      %-56s %s" % (text, loc))


if __name__ == "__main__":
    main()
