#!/usr/bin/env python3
"""Static instruction census of ONE kernel instantiation: the translation unit is compiled to gfx950 assembly with the flags of
pyphysim_amd/csrc/Makefile, the named kernel's body is cut at its workgroup barriers, and the instructions of every section are
counted by class.  The class follows from the opcode's PREFIX alone (no list of instruction names):

  mfma    v_mfma*                      cvt     v_cvt*                      f64    any other v_* whose name carries _f64
  move    v_mov* v_accvgpr* v_swap*    lane    v_readlane* v_writelane* v_readfirstlane*  (the SGPR spill traffic)
  select  v_cndmask*                   int     every other v_*             lds    ds_*
  vmem    global_* flat_* buffer_* scratch_*                               scalar s_* (the barrier and s_waitcnt / s_nop included)

The count is static: a section is the TEXT between two barriers in layout order, whichever branches inside it are hot -- the
dynamic figures are rocprofv3's SQ_INSTS_* (profiles/<round>/c4_f64_pmc_summary.json).  Runs without a GPU.

usage: python scripts/kernel_census.py [--source pipeline_mimo_pw.hip] [--kernel 'k_run_mimo_ofdm_pw<4, 2, 3, false, 0, true, true>'] [--top N]
       (--top N adds the N most frequent opcodes of every section; --keep FILE keeps the kernel's assembly)"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pyphysim_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wno-unused-function",
         "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=fast"]
CLASSES = ("f64", "mfma", "cvt", "int", "move", "select", "lane", "lds", "vmem", "scalar")


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_cvt"):
        return "cvt"
    if op.startswith(("v_mov", "v_accvgpr", "v_swap")):
        return "move"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if op.startswith("v_cndmask"):
        return "select"
    if op.startswith("v_"):
        return "f64" if "_f64" in op else "int"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("s_"):
        return "scalar"
    return None


def kernel_body(asm, want):
    """the lines between the label of the kernel whose demangled name contains `want` and its .Lfunc_end"""
    labels = re.findall(r"^(_Z\w+):\s*(?:;.*)?$", asm, re.M)
    names = subprocess.run(["c++filt"], input="\n".join(labels), capture_output=True, text=True, check=True).stdout.split("\n")
    hits = [(l, n) for l, n in zip(labels, names) if want in n]
    if len(hits) != 1:
        sys.exit("%d kernels match %r:\n  %s" % (len(hits), want, "\n  ".join(n.split("(")[0] for _, n in hits) or
                                              "\n  ".join(n.split("(")[0] for n in names if "k_" in n)))
    label, name = hits[0]
    start = asm.index("\n" + label + ":")
    end = asm.index(".Lfunc_end", start)
    res = {}
    for block in asm[asm.index("amdhsa.kernels"):].split("  - .agpr_count:")[1:]:      # the code-object metadata (as kernel_resources.py)
        if re.search(r"\.name:\s+%s\s" % re.escape(label), block):
            for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                      "group_segment_fixed_size"):
                m = re.search(r"\.%s:\s+(\d+)" % k, block)
                res[k] = int(m.group(1)) if m else None
    return name.split("(")[0], asm[start:end].split("\n")[2:], res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default="pipeline_mimo_pw.hip")
    ap.add_argument("--kernel", default="k_run_mimo_ofdm_pw<4, 2, 3, false, 0, true, true>")
    ap.add_argument("--top", type=int, default=0)
    ap.add_argument("--define", action="append", default=[])
    ap.add_argument("--keep", help="write the kernel's assembly to this file")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC] + FLAGS + ["-D" + d for d in args.define] + ["--cuda-device-only", "-S", os.path.join(CSRC, args.source), "-o", out],
                       check=True)
        asm = open(out).read()
    name, body, res = kernel_body(asm, args.kernel)
    if args.keep:
        open(args.keep, "w").write("\n".join(body) + "\n")
    sections = [collections.Counter()]
    ops = [collections.Counter()]
    for line in body:
        line = line.split(";")[0].strip()
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        op = line.split()[0]
        cls = classify(op)
        if cls is None:
            continue
        sections[-1][cls] += 1
        ops[-1][op] += 1
        if op.startswith("s_barrier"):
            sections.append(collections.Counter())
            ops.append(collections.Counter())
    print("# %s  (%s, gfx950, static count per barrier-delimited section in layout order)" % (name, args.source))
    print("# " + "  ".join("%s %s" % kv for kv in res.items()))
    print("%-8s" % "section" + "".join("%8s" % c for c in CLASSES) + "%8s" % "valu")
    tot = collections.Counter()
    for i, s in enumerate(sections):
        valu = sum(s[c] for c in ("f64", "mfma", "cvt", "int", "move", "select", "lane"))
        print("%-8d" % i + "".join("%8d" % s[c] for c in CLASSES) + "%8d" % valu)
        tot.update(s)
    valu = sum(tot[c] for c in ("f64", "mfma", "cvt", "int", "move", "select", "lane"))
    print("%-8s" % "total" + "".join("%8d" % tot[c] for c in CLASSES) + "%8d" % valu)
    if args.top:
        for i, o in enumerate(ops):
            print("# section %d: %s" % (i, "  ".join("%s %d" % kv for kv in o.most_common(args.top))))


if __name__ == "__main__":
    main()
