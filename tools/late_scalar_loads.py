"""Scalar loads and the waits behind them in the batched path's kernels, from the gfx950 assembly.

usage: python tools/late_scalar_loads.py [--all] [--lines KERNEL] [--asm FILE --remarks FILE] [--flags "..."]

Compiles mlmapping_amd/csrc/mlmap_hip.hip to device assembly with the Makefile's flags (plus line tables and the compiler's
resource remarks) and prints per kernel:
  instructions | s_load | late = an s_load outside the entry block with `s_waitcnt lgkmcnt(0)` within the next five instructions
  | all lgkmcnt(0) waits | s_load behind the kernel's first s_barrier
and the compiler's remark: VGPRs, SGPRs, spills, scratch, occupancy.
--lines KERNEL (a substring of the demangled name) also lists every s_load outside the entry block with the source line it was
emitted for (innermost inlined location first) and the loop depth of its block; * = late, > = behind the first barrier.  Scalar loads and waits only: nothing else of the code is judged.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
BATCHED = ["k_bin_sectors<0, 1>", "k_bin_sectors<1, 1>", "k_bin_sectors<2, 1>", "k_sector<false, 256>", "k_rank<false>", "k_chain_lanes<1>",
           "k_tile(", "k_apply_tiles("]


def makefile_flags():
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"CXXFLAGS\s*\?=\s*(.*)", line)
        if m:
            return m.group(1).split()
    raise SystemExit("no CXXFLAGS in the Makefile")


def compile_asm(extra):
    tmp = tempfile.mkdtemp(prefix="late_sload_")
    asm = os.path.join(tmp, "mlmap_hip.s")
    cmd = [os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "--cuda-device-only", "-S"] + makefile_flags() + extra + [
        "-gline-tables-only", "-Rpass-analysis=kernel-resource-usage", "mlmap_hip.hip", "-o", asm]
    r = subprocess.run(cmd, cwd=CSRC, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit("compilation failed")
    return open(asm).read(), r.stderr


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True)
    return dict(zip(names, r.stdout.split("\n")))


def parse_remarks(text):
    out, cur = {}, None
    for line in text.split("\n"):
        m = re.search(r"remark:\s+(Function Name|[A-Za-z ]+(?:\[[^\]]*\])?):\s*(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def parse_kernel(body):
    """body: the lines between a kernel's label and its .Lfunc_end"""
    insts = []  # (mnemonic, text, source location + loop depth of the block, in entry block)
    loc, entry, depth, head = "", True, 0, False
    for line in body:
        s = line.strip()
        if head and "Depth=" in s:  # (the compiler's block comments: "=>This Inner Loop Header: Depth=1", "in Loop: Header=BB1_2 Depth=2")
            depth = max(depth, int(re.search(r"Depth=(\d+)", s).group(1)))
        if not s or s.startswith(";") and not s.startswith("; %bb"):
            continue
        if s.startswith(".loc"):
            c = s.split(";", 1)
            loc = c[1].strip() if len(c) > 1 else ""
            continue
        if s.startswith("; %bb.") or re.match(r"\.LBB\d+_\d+:", s):
            if insts:
                entry = False
            depth, head = 0, True
            if "Depth=" in s:
                depth = int(re.search(r"Depth=(\d+)", s).group(1))
            continue
        if s.startswith(".") or s.endswith(":"):
            continue
        text = s.split(";", 1)[0].strip()
        head = False
        insts.append((text.split()[0], text, ("loop depth %d  " % depth if depth else "") + loc, entry))
    n_load = n_late = n_wait = n_after = 0
    barrier, after = False, []
    for i, (op, text, loc, entry) in enumerate(insts):
        if op == "s_barrier":
            barrier = True
        if op == "s_waitcnt" and "lgkmcnt(0)" in text:
            n_wait += 1
        if op.startswith("s_load_") or op.startswith("s_buffer_load_"):
            n_load += 1
            late = not entry and any(o == "s_waitcnt" and "lgkmcnt(0)" in t for o, t, _, _ in insts[i + 1:i + 6])
            n_late += late
            n_after += barrier
            if not entry:
                after.append(("%s%s %s" % ("*" if late else " ", ">" if barrier else " ", text), loc))
    return {"insts": len(insts), "s_load": n_load, "late": n_late, "waits": n_wait, "after_barrier": n_after, "after": after}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true", help="every kernel of the library, not only the batched path's")
    ap.add_argument("--lines", action="append", default=[], help="list the s_load outside the entry block of this kernel by source line")
    ap.add_argument("--asm")
    ap.add_argument("--remarks")
    ap.add_argument("--flags", default="", help="extra compiler flags (an experiment build's ALT_FLAGS)")
    a = ap.parse_args()
    if a.asm:
        asm, rem = open(a.asm).read(), open(a.remarks).read() if a.remarks else ""
    else:
        asm, rem = compile_asm(a.flags.split())
    remarks = parse_remarks(rem)
    lines = asm.split("\n")
    kernels = {}  # mangled -> body
    amdhsa = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
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
    names = demangle(list(kernels))
    print("%-34s %7s %7s %6s %9s %9s | %5s %5s %11s %8s %5s" % ("kernel", "insts", "s_load", "late", "lgkm(0)", "s_load", "VGPRs", "SGPRs", "spills s/v", "scratch", "occ"))
    print("%-34s %7s %7s %6s %9s %9s |" % ("", "", "", "", "waits", "> barrier"))
    for mangled, body in kernels.items():
        dn = names[mangled]
        if dn.startswith("void "):
            dn = dn[5:]
        if not a.all and not any(dn.startswith(b) for b in BATCHED):
            continue
        k = parse_kernel(body)
        r = remarks.get(mangled, {})
        short = dn.split("(")[0]
        print("%-34s %7d %7d %6d %9d %9d | %5s %5s %11s %8s %5s" % (short, k["insts"], k["s_load"], k["late"], k["waits"], k["after_barrier"], r.get("VGPRs", "?"),
                                                                  r.get("TotalSGPRs", "?"), "%s/%s" % (r.get("SGPRs Spill", "?"), r.get("VGPRs Spill", "?")),
                                                                  r.get("ScratchSize [bytes/lane]", "?"), r.get("Occupancy [waves/SIMD]", "?")))
        if any(w in dn for w in a.lines):
            for text, loc in k["after"]:
                print("      %-48s %s" % (text, loc))


if __name__ == "__main__":
    main()
