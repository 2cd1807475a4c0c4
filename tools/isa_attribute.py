#!/usr/bin/env python3
"""Static instruction counts of one kernel per source line.

    python tools/isa_attribute.py vgsim_amd/csrc/vgx_quad.hip vgx_quad_kernel [--lines 544-739,1101-1221] [--top 40]
                                  [--match v_div_scale_f64] [--ops] [--depth 1] [--flags "..."]

Compiles the .hip for the device with the Makefile's flags plus -gline-tables-only, reads the `.loc` comments of the assembly
(they carry the inline chain: `a.h:12:3 @[ k.hip:583:36 @[ k.hip:1324:111 ] ]`) and attributes every instruction of the named
kernel to a line of the kernel's own file: the frame `--depth` levels inside the outermost one (default 1: the line of the function
the kernel's body was inlined from — an instruction of a helper called from that line counts for that line), the innermost frame
when the chain is shorter.  Per line: VALU (every v_*), of them chain steps (v_fmac_f64 with a DPP source), lane reads
(v_readlane / v_readfirstlane), s_nop, SALU (s_* that compute: no s_nop, s_waitcnt, branches), LDS (ds_*), VMEM.  --match REGEX adds a
column that counts the mnemonics it matches.  The counts are static: a line inside a loop or behind a branch is counted once.
Also prints the kernel's register and spill counts and its code size.  Needs hipcc; no GPU."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

FLAGS = "-O3 -ffp-contract=off -fPIC -std=c++17 -Wno-unused-function"      # vgsim_amd/csrc/Makefile
FRAME = re.compile(r"([^\s@\[\]]+):(\d+):(\d+)")
BRANCH = ("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call", "s_endpgm", "s_barrier", "s_sleep", "s_waitcnt", "s_nop",
          "s_code_end", "s_sethalt", "s_trap", "s_setprio")


def compile_asm(hipcc, src, arch, flags, out):
    cmd = [hipcc, "--offload-arch=" + arch] + flags.split() + ["-gline-tables-only", "-S", "--cuda-device-only", "-o", out, os.path.basename(src)]
    subprocess.check_call(cmd, cwd=os.path.dirname(os.path.abspath(src)), stderr=subprocess.DEVNULL)


def kernel_lines(asm, kernel):
    """the instruction stream of `kernel` and its metadata block"""
    body, meta, inside = [], {}, False
    lines = open(asm).read().splitlines()
    for ln in lines:
        if ln.startswith(kernel + ":"):
            inside = True
            continue
        if inside and ln.startswith(".Lfunc_end"):
            inside = False
        if inside:
            body.append(ln)
    for i, ln in enumerate(lines):       # the msgpack-as-yaml notes: the .name entry closes a kernel's block, the counts precede it
        if re.match(r"\s+\.name:\s+%s\s*$" % re.escape(kernel), ln):
            for back in lines[max(i - 40, 0):i + 12]:
                m = re.match(r"\s+\.(sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count|agpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", back)
                if m:
                    meta[m.group(1)] = int(m.group(2))
    # "; codeLenInByte = N" follows the kernel's body
    m = re.search(r"^%s:.*?; codeLenInByte = (\d+)" % re.escape(kernel), "\n".join(lines), re.S | re.M)
    if m:
        meta["code_bytes"] = int(m.group(1))
    return body, meta


def attribute(body, main, depth):
    rows = collections.defaultdict(collections.Counter)
    mnem = collections.defaultdict(collections.Counter)
    cur = 0
    for ln in body:
        s = ln.strip()
        if s.startswith(".loc"):
            frames = [(os.path.basename(f), int(l)) for f, l, _ in FRAME.findall(s.split(";", 1)[1] if ";" in s else "")]
            own = [l for f, l in frames if f == main]            # innermost first
            if own:
                cur = own[-1 - depth] if len(own) > depth else own[0]
            continue
        if not s or s[0] in ".;" or s.endswith(":"):
            continue
        op = s.split()[0]
        c = rows[cur]
        mnem[cur][op] += 1
        if op.startswith("v_"):
            c["valu"] += 1
            if op.startswith("v_fmac_f64_dpp"):
                c["chain"] += 1
            if op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
                c["readlane"] += 1
        elif op == "s_nop":
            c["nop"] += 1
        elif op.startswith("s_"):
            if not op.startswith(BRANCH):
                c["salu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
    return rows, mnem


def parse_ranges(text):
    out = []
    for part in text.split(","):
        if part:
            a, _, b = part.partition("-")
            out.append((int(a), int(b or a)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source")
    ap.add_argument("kernel")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--flags", default=FLAGS, help="compiler flags (default: the Makefile's)")
    ap.add_argument("--asm", default="", help="read this assembly file instead of compiling (made with -S -gline-tables-only)")
    ap.add_argument("--lines", default="", help="only these lines of the kernel's file, e.g. 544-739,1101-1221")
    ap.add_argument("--depth", type=int, default=1, help="inline frames below the outermost one to attribute to (default 1)")
    ap.add_argument("--top", type=int, default=0, help="print only the N lines with the most VALU")
    ap.add_argument("--ops", action="store_true", help="after the table: the mnemonics of every line printed, with their counts")
    ap.add_argument("--match", default="", help="regular expression: count the mnemonics it matches in a column of its own")
    a = ap.parse_args()
    main_file = os.path.basename(a.source)
    with tempfile.TemporaryDirectory() as tmp:
        asm = a.asm
        if not asm:
            asm = os.path.join(tmp, "k.s")
            compile_asm(a.hipcc, a.source, a.arch, a.flags, asm)
        body, meta = kernel_lines(asm, a.kernel)
    if not body:
        sys.exit("isa_attribute: no kernel %s in %s" % (a.kernel, a.source))
    rows, mnem = attribute(body, main_file, a.depth)
    ranges = parse_ranges(a.lines)
    keep = [l for l in sorted(rows) if not ranges or any(lo <= l <= hi for lo, hi in ranges)]
    rx = re.compile(a.match) if a.match else None
    cols = ["valu", "chain", "readlane", "nop", "salu", "lds", "vmem"]
    total = collections.Counter()
    table = []
    for l in keep:
        c = rows[l]
        extra = sum(n for op, n in mnem[l].items() if rx.search(op)) if rx else 0
        total.update(c)
        total["match"] += extra
        table.append((l, c, extra))
    if a.top:
        table = sorted(table, key=lambda t: -t[1]["valu"])[:a.top]
    print("%s  %s" % (a.kernel, "  ".join("%s=%d" % kv for kv in sorted(meta.items()))))
    print("%6s " % "line" + " ".join("%8s" % c for c in cols) + ("  %8s" % "match" if rx else ""))
    for l, c, extra in table:
        print("%6d " % l + " ".join("%8d" % c[k] for k in cols) + ("  %8d" % extra if rx else ""))
    if a.ops:
        for l, c, extra in table:
            print("%6d: %s" % (l, "  ".join("%s x%d" % (op, n) for op, n in sorted(mnem[l].items(), key=lambda t: (-t[1], t[0])))))
    print("%6s " % "sum" + " ".join("%8d" % total[k] for k in cols) + ("  %8d" % total["match"] if rx else ""))


if __name__ == "__main__":
    main()
