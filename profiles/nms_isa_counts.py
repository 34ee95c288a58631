#!/usr/bin/env python3
"""Static instruction counts of k_canny_nms4 (or another kernel of revo_pyramid.hip) from the compiler's gfx950 assembly.

  python profiles/nms_isa_counts.py [--rev REV ...] [--kernel k_canny_nms4] [--keep DIR]

Compiles revo_amd/csrc/revo_pyramid.hip with `hipcc -S --cuda-device-only` and the flags of csrc/Makefile, cuts the kernel's
body out of the assembly and counts total / VALU / SALU / waits+nops / v_cndmask / v_cmp / v_mov, and reads the VGPR count and
the scratch size from the kernel's resource comments.  The kernel is straight-line code (the script prints its branch count), so
static counts are the dynamic counts of one thread (24 pixels).  The working tree is always counted; every `--rev REV` adds a
column for that commit's csrc/ (taken with `git archive`, nothing is checked out).  No GPU needed.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = "-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden -fvisibility-inlines-hidden -w".split()
WAITS = ("s_waitcnt", "s_nop", "s_sleep")
# scalar opcodes that are program flow or bookkeeping rather than ALU work are still counted as SALU except these
NOT_ALU = WAITS + ("s_endpgm", "s_branch", "s_cbranch", "s_setprio", "s_barrier", "s_code_end")


def assembly(csrc, keep=None):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = os.path.join(keep or tempfile.mkdtemp(prefix="nms_isa_"), "revo_pyramid.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S"] + FLAGS +
                          ["-I", os.path.join(csrc, "..", "..", "include"), os.path.join(csrc, "revo_pyramid.hip"), "-o", out])
    return open(out).read()


def count(asm, kernel):
    m = re.search(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)^\s*\.section\s+\.rodata.*?^\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel" % re.escape(kernel),
                  asm, re.S | re.M)
    if not m:
        raise SystemExit("kernel %s not found in the assembly" % kernel)
    body, desc = m.group(2), m.group(3)
    ops = []
    for ln in body.splitlines():
        ln = ln.split(";")[0].strip()
        if not ln or ln.startswith(".") or ln.endswith(":"):
            continue
        ops.append(ln.split()[0])
    c = {"instructions": len(ops),
         "VALU": sum(o.startswith("v_") for o in ops),
         "v_cndmask": sum(o.startswith("v_cndmask") for o in ops),
         "v_cmp": sum(o.startswith("v_cmp") for o in ops),
         "v_mov": sum(o.startswith("v_mov") for o in ops),
         "SALU": sum(o.startswith("s_") and not o.startswith(NOT_ALU) and not o.startswith(("s_load", "s_buffer_load")) for o in ops),
         "waits / nops": sum(o.startswith(WAITS) for o in ops),
         "memory": sum(o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_", "s_load", "s_buffer_load")) for o in ops),
         "branches": sum(o.startswith(("s_branch", "s_cbranch")) for o in ops)}
    for key, pat in (("VGPRs", r"\.amdhsa_next_free_vgpr (\d+)"), ("scratch bytes", r"\.amdhsa_private_segment_fixed_size (\d+)")):
        c[key] = int(re.search(pat, desc).group(1))
    vg = re.search(r"\.set %s\.num_vgpr, (\d+)" % re.escape(m.group(1)), asm)  # the count in use; next_free_vgpr is the allocation
    if vg:
        c["VGPRs"] = int(vg.group(1))
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", action="append", default=[], help="also count this commit's sources (repeatable)")
    ap.add_argument("--kernel", default="k_canny_nms4")
    ap.add_argument("--keep", help="write the working tree's revo_pyramid.s into this directory")
    a = ap.parse_args()
    cols = []
    for rev in a.rev:
        tmp = tempfile.mkdtemp(prefix="nms_isa_src_")
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "revo_amd/csrc", "include"], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        cols.append((rev, count(assembly(os.path.join(tmp, "revo_amd", "csrc")), a.kernel)))
        shutil.rmtree(tmp)
    if a.keep:
        os.makedirs(a.keep, exist_ok=True)
    cols.append(("working tree", count(assembly(os.path.join(ROOT, "revo_amd", "csrc"), a.keep), a.kernel)))
    print("%s, gfx950, per thread" % a.kernel)
    print("%-16s" % "" + "".join("%14s" % n[:13] for n, _ in cols))
    for key in cols[0][1]:
        print("%-16s" % key + "".join("%14d" % c[key] for _, c in cols))
    return 0


if __name__ == "__main__":
    sys.exit(main())
