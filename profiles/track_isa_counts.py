#!/usr/bin/env python3
"""Static instruction counts of k_track's streaming loops (and k_pair_info's) from the compiler's gfx950 assembly.

  python profiles/track_isa_counts.py [--rev REV ...] [--keep DIR]

Compiles revo_amd/csrc/revo_track.hip and revo_info.hip with `hipcc -S --cuda-device-only` and the flags csrc/Makefile gives
them (FLAGS_revo_track / FLAGS_revo_info are read from that Makefile, the given revision's for a --rev column), cuts every
k_track / k_pair_info instantiation out of the assembly and finds its streaming loops: the innermost loops (the blocks the
compiler's own loop comments assign to an `Inner Loop Header`) whose body holds the point's global_load_dwordx4.  One trip
of such a loop is one point of one thread, so its static counts are the per-point counts, with every exec-masked block (a
retry's gathers, the Huber division) counted as if taken.  A loop is named by what it loads: the full candidate's patch is
four gathers (two rows of four samples, two rows of two), every error-only retry adds two exec-masked dwordx2 gathers (or
four dword gathers), and the cost pass (tracker.cpp:357-393) has the point and two dword lookups only.  Per loop: instructions, VALU, packed VALU
(v_pk_*), v_mov + v_pk_mov, v_cndmask, SALU, memory ops; per kernel: VGPRs in use / allocated and scratch bytes.
The working tree is always counted; every `--rev REV` adds a column for that commit (taken with `git archive`, nothing is
checked out).  No GPU needed.
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
NOT_ALU = WAITS + ("s_endpgm", "s_branch", "s_cbranch", "s_setprio", "s_barrier", "s_code_end")
UNITS = (("revo_track", "k_track"), ("revo_info", "k_pair_info"))
ROWS = ("instructions", "VALU", "packed", "v_mov+pk_mov", "v_cndmask", "SALU", "memory")


def unit_flags(csrc, unit):
    m = re.search(r"^FLAGS_%s\s*=\s*(.*)$" % unit, open(os.path.join(csrc, "Makefile")).read(), re.M)
    return m.group(1).split() if m else []


def assembly(csrc, unit, keep=None):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = os.path.join(keep or tempfile.mkdtemp(prefix="track_isa_"), unit + ".s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S"] + FLAGS + unit_flags(csrc, unit) +
                          ["-I", os.path.join(csrc, "..", "..", "include"), os.path.join(csrc, unit + ".hip"), "-o", out])
    return open(out).read()


def demangled(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", "").replace("void ", "")) for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def tally(ops):
    return {"instructions": len(ops),
            "VALU": sum(o.startswith("v_") for o in ops),
            "packed": sum(o.startswith("v_pk_") and not o.startswith("v_pk_mov") for o in ops),
            "v_mov+pk_mov": sum(o.startswith(("v_mov", "v_pk_mov")) for o in ops),
            "v_cndmask": sum(o.startswith("v_cndmask") for o in ops),
            "SALU": sum(o.startswith("s_") and not o.startswith(NOT_ALU) and not o.startswith(("s_load", "s_buffer_load")) for o in ops),
            "memory": sum(o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_", "s_load", "s_buffer_load")) for o in ops)}


def loop_name(ops):
    x4 = sum(o in ("global_load_dwordx4", "global_load_dwordx3") for o in ops)  # the point may arrive as x3 (w unused)
    x2 = sum(o == "global_load_dwordx2" for o in ops)
    x1 = sum(o == "global_load_dword" for o in ops)
    if x4 < 3:
        return "cost pass" if x1 else "other"
    n = (x1 + 2 * (x2 - 2)) // 4  # a retry's four samples: four dword gathers, or two dwordx2 where the compiler joins a row's pair
    return "full" if n == 0 else "full + %d retr%s" % (n, "y" if n == 1 else "ies")


def kernels(asm, stem):
    """{mangled name: (loops, resources)}; loops = [(name, counts)] in program order"""
    res = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)^\s*\.section\s+\.rodata.*?^\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel" % stem,
                         asm, re.S | re.M):
        name, body, desc = m.group(1), m.group(2), m.group(3)
        # the compiler names every block's loop in a comment: `.LBB2_163: ; ... =>This Inner Loop Header` opens an innermost loop,
        # `; in Loop: Header=BB2_163` marks its other blocks wherever the layout puts them
        lines = body.splitlines()
        inner, cur, hdr = {}, None, None
        for raw in lines:  # the headers first: the layout may put a loop's latch blocks above its header
            blk = re.match(r"\s*\.L(BB\d+_\d+):", raw)
            if blk or re.match(r"\s*;\s*%bb\.\d+:", raw):
                hdr = blk.group(1) if blk else None
            elif raw.split(";")[0].strip():
                hdr = None
            if "This Inner Loop Header" in raw and hdr:
                inner[hdr] = []
        for raw in lines:
            ln = raw.split(";")[0].strip()
            blk = re.match(r"\s*\.L(BB\d+_\d+):", raw)
            if blk or re.match(r"\s*;\s*%bb\.\d+:", raw):
                m2 = re.search(r"in Loop: Header=(BB\d+_\d+)", raw)
                cur = m2.group(1) if m2 else (blk.group(1) if blk else None)
                cur = cur if cur in inner else None
            if ln and not ln.startswith(".") and not ln.endswith(":") and cur:
                inner[cur].append(ln.split()[0])
        loops = [(loop_name(o), tally(o)) for o in inner.values() if "global_load_dwordx4" in o]
        # allocated: next_free_vgpr rounded up to the granule of 8 (gfx950's unified register file)
        rsrc = {"VGPRs allocated": (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) + 7) // 8 * 8,
                "scratch bytes": int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1))}
        vg = re.search(r"\.set %s\.num_vgpr, (\d+)" % re.escape(name), asm)
        rsrc["VGPRs in use"] = int(vg.group(1)) if vg else rsrc["VGPRs allocated"]
        res[name] = (loops, rsrc)
    return res


def column(csrc, keep=None):
    col = {}
    for unit, stem in UNITS:
        if os.path.exists(os.path.join(csrc, unit + ".hip")):
            col.update(kernels(assembly(csrc, unit, keep), stem))
    return col


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", action="append", default=[], help="also count this commit's sources (repeatable)")
    ap.add_argument("--keep", help="write the working tree's assembly into this directory")
    a = ap.parse_args()
    cols = []
    for rev in a.rev:
        tmp = tempfile.mkdtemp(prefix="track_isa_src_")
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "revo_amd/csrc", "include"], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        cols.append((rev, column(os.path.join(tmp, "revo_amd", "csrc"))))
        shutil.rmtree(tmp)
    if a.keep:
        os.makedirs(a.keep, exist_ok=True)
    cols.append(("working tree", column(os.path.join(ROOT, "revo_amd", "csrc"), a.keep)))
    names = sorted(set().union(*(c.keys() for _, c in cols)))
    nice = demangled(names)
    head = "%-34s" % "" + "".join("%14s" % n[:13] for n, _ in cols)
    for k in names:
        if not any(k in c and c[k][0] for _, c in cols):
            continue
        print("\n%s, gfx950" % nice[k])
        print(head)
        for key in ("VGPRs in use", "VGPRs allocated", "scratch bytes"):
            print("  %-32s" % key + "".join("%14s" % (c[k][1][key] if k in c else "-") for _, c in cols))
        loops = []
        for _, c in cols:
            loops += [n for n, _ in c.get(k, ((), 0))[0] if n not in loops]
        for ln in loops:
            print("  loop: %s, per point" % ln)
            for row in ROWS:
                vals = [dict(c[k][0]).get(ln) if k in c else None for _, c in cols]
                line = "    %-30s" % row + "".join("%14s" % (v[row] if v else "-") for v in vals)
                if row == "VALU" and len(vals) > 1 and vals[0] and vals[-1]:
                    line += "   (%+.1f %%)" % (100.0 * (vals[-1][row] - vals[0][row]) / vals[0][row])
                print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
