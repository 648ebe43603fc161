#!/usr/bin/env python3
"""Static wait distance of ONE kernel instantiation: for every LDS read (ds_read*) and every global load (global_load*) of a
barrier-delimited section, how many VALU instructions lie between the load and the first s_waitcnt that covers it.  The compile
and the kernel cut are scripts/kernel_census.py's (same flags as pyphysim_amd/csrc/Makefile); runs without a GPU.

A wait covers a load when its counter field is no larger than the number of operations of that counter issued behind the load:
  lgkmcnt   ds_* (reads and writes) and s_load* / s_buffer_load*; LDS operations return in order, so lgkmcnt(N) retires every
            LDS operation but the last N issued.  (Scalar loads return out of order: the compiler then waits for 0.)
  vmcnt     global_* / buffer_* / flat_* / scratch_* loads and stores (gfx950 has one vector-memory counter for both).
The distance counts VALU instructions only (v_*, the matrix-core products included): scalar instructions issue beside them.  A
load whose covering wait lies behind the section's closing barrier is listed with the distance to the barrier and a '+'.

The count is static and in layout order, as the census is: a branch inside a section is read straight through.

usage: python scripts/wait_distance.py [--source pipeline_mimo_pw.hip] [--kernel 'k_run_mimo_ofdm_pw<4, 2, 3, false, 0, true, true>']
                                       [--list SECTION]    (every load of that section, not only the summary)"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_census as kc  # noqa: E402


def counter_of(op):
    if op.startswith("ds_") or op.startswith(("s_load", "s_buffer_load")):
        return "lgkmcnt"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmcnt"
    return None


def watched(op):
    return op.startswith("ds_read") or op.startswith("global_load")


def sections_of(body):
    """[(opcode, operand text)] per barrier-delimited section, in layout order"""
    secs = [[]]
    for line in body:
        line = line.split(";")[0].strip()
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        op, _, rest = line.partition(" ")
        if kc.classify(op) is None:
            continue
        secs[-1].append((op, rest.strip()))
        if op.startswith("s_barrier"):
            secs.append([])
    return secs


def distances(sec):
    """[(index, opcode, operands, VALU instructions up to the covering wait, the wait's text or None, whether that wait is the very
    next instruction)] for the section's loads"""
    out = []
    for i, (op, rest) in enumerate(sec):
        if not watched(op):
            continue
        ctr = counter_of(op)
        behind = valu = 0
        hit, at_once = None, False
        for k, (op2, rest2) in enumerate(sec[i + 1:]):
            if op2.startswith("v_"):
                valu += 1
            elif op2 == "s_waitcnt":
                m = re.search(ctr + r"\((\d+)\)", rest2)
                if m and int(m.group(1)) <= behind:
                    hit, at_once = rest2, k == 0
                    break
            elif counter_of(op2) == ctr:
                behind += 1
        out.append((i, op, rest, valu, hit, at_once))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default="pipeline_mimo_pw.hip")
    ap.add_argument("--kernel", default="k_run_mimo_ofdm_pw<4, 2, 3, false, 0, true, true>")
    ap.add_argument("--define", action="append", default=[])
    ap.add_argument("--list", type=int, action="append", default=[], help="list every load of this section")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([kc.HIPCC] + kc.FLAGS + ["-D" + d for d in args.define] +
                       ["--cuda-device-only", "-S", os.path.join(kc.CSRC, args.source), "-o", out], check=True)
        asm = open(out).read()
    name, body, res = kc.kernel_body(asm, args.kernel)
    secs = sections_of(body)
    print("# %s  (%s, gfx950: VALU instructions between a load and the first s_waitcnt that covers it)" % (name, args.source))
    print("# vgpr_count %s  barriers %d" % (res.get("vgpr_count"), len(secs) - 1))
    print("%-8s%-18s%7s%7s%8s%7s%10s" % ("section", "opcode", "loads", "min", "median", "max", "next-op"))
    for s, sec in enumerate(secs):
        d = distances(sec)
        for op in sorted(set(x[1] for x in d)):
            v = [x[3] for x in d if x[1] == op]
            at_once = sum(1 for x in d if x[1] == op and x[5])
            print("%-8d%-18s%7d%7d%8d%7d%10d" % (s, op, len(v), min(v), int(statistics.median(v)), max(v), at_once))
    print("# next-op: loads whose covering wait is the instruction right behind them")
    for s in args.list:
        print("# section %d, every load:" % s)
        for i, op, rest, valu, hit, _ in distances(secs[s]):
            print("  %5d  %-16s %-34s %5d%s  %s" % (i, op, rest, valu, "" if hit else "+", "s_waitcnt " + hit if hit else "(behind the barrier)"))


if __name__ == "__main__":
    main()
