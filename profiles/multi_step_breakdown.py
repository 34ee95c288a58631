"""Where an S-stream revo_vo_multi step spends its time, from a rocprofv3 --kernel-trace --memory-copy-trace run of
profiles/multi_stream_rates.py (csv output):

    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -o s32 -- \\
        python profiles/multi_stream_rates.py --streams 32 --reps 1 --frames 16 --workers 1 --depth f32
    python profiles/multi_step_breakdown.py DIR/s32

A step is the interval between the starts of two consecutive batched tracker grids (k_track<false>); the last run of the
profile (its second half of grids) is summarised.  Per step: the busy time of the H2D copies, of the build kernels, of the
tracker grid, of the vote / cloud-copy / promotion kernels, and the time no kernel or copy ran at all (host hops)."""
import csv
import sys
from collections import defaultdict


def union(iv):
    t, end = 0, None
    for a, b in sorted(iv):
        if end is None or a > end:
            t += b - a
            end = b
        elif b > end:
            t += b - end
            end = b
    return t


def main(prefix):
    ks = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
          for r in csv.DictReader(open(prefix + "_kernel_trace.csv"))]
    cs = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(prefix + "_memory_copy_trace.csv"))
          if r["Direction"] == "MEMORY_COPY_HOST_TO_DEVICE"]
    grids = sorted(a for a, b, n in ks if "k_track<false>" in n)
    grids = grids[len(grids) // 2:]  # the timed run (the first half is the warm-up run)
    cls = lambda n: ("tracker grid" if "k_track<false>" in n else "vote + cloud copy" if ("vote" in n or "copy_cloud" in n)
                     else "promotion (copy + EDT)" if ("copy_segments" in n or "edt" in n) else
                     "resident gate" if "gate" in n else "build")
    tot = defaultdict(float)
    nstep = len(grids) - 1
    for a, b in zip(grids, grids[1:]):
        kin = [(max(s, a), min(e, b), cls(n)) for s, e, n in ks if e > a and s < b]
        cin = [(max(s, a), min(e, b)) for s, e in cs if e > a and s < b]
        for c in set(k[2] for k in kin):
            tot[c] += union([(s, e) for s, e, k in kin if k == c])
        tot["H2D copies"] += union(cin)
        tot["device busy (any kernel or copy)"] += union([(s, e) for s, e, _ in kin] + cin)
        tot["step"] += b - a
    print("revo_vo_multi step breakdown: %d steps of the timed run, mean per step (busy time; classes overlap in time)" % nstep)
    for k in ["step", "device busy (any kernel or copy)", "H2D copies", "build", "tracker grid", "vote + cloud copy",
              "promotion (copy + EDT)", "resident gate"]:
        print("  %-34s %8.3f ms" % (k, tot[k] / nstep / 1e6))
    print("  %-34s %8.3f ms" % ("device idle (host hops)", (tot["step"] - tot["device busy (any kernel or copy)"]) / nstep / 1e6))


if __name__ == "__main__":
    main(sys.argv[1])
