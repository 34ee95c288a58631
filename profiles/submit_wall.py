#!/usr/bin/env python3
"""Host wall time of one revo_pipeline_submit in the steady state of the pipelined step: is the host what paces the build stream?

  python profiles/submit_wall.py [--pairs 32] [--width 640 --height 480 --levels 4] [--steps 200] [--warmup 20] [--repeats 3]

The shape of bench.py's pipelined phase without its collective and timing events: one pipeline handle of depth 4, four input
batches in rotation, device records.  Every submit is timed with perf_counter around the call alone; the loop is free-running,
so a submit that finds its slot's previous step unfinished includes the wait for it (that IS the host's pace).  Prints, per
repeat, the step time of the whole loop (wall / steps, device drained at the end) beside the mean, median, 90th percentile and
maximum of the submit calls, and the share of the loop's wall time spent inside submit.  REVO_HIP_SO picks the library."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    from revo_amd import api, synth
    from revo_amd.settings import ImgPyramidSettings, TrackerSettings
    s = ImgPyramidSettings.scaled(a.width, a.height, a.levels)
    cam = api.CameraPyr(s)
    api.TrackerNew(TrackerSettings(), s, cam)
    # a few rendered pairs, repeated to fill the batches: the kernels' work depends on the frames, the host's does not
    base = [synth.make_pair(4000 + i, s) for i in range(4)]
    inputs = []
    for b in range(4):
        pairs = [base[(b + i) % len(base)] for i in range(a.pairs)]
        bgr = torch.from_numpy(np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])).cuda()
        dep = torch.from_numpy(np.stack([p[k][1] for p in pairs for k in ("ref", "curr")]).astype(np.float32)).cuda()
        inputs.append((bgr, dep))
    res = [torch.zeros(a.pairs * 96, dtype=torch.uint8, device="cuda") for _ in range(4)]
    pipe = api.Pipeline(cam, a.pairs, depth=4)
    n = [0]

    def submit():
        bgr, dep = inputs[n[0] % 4]
        t0 = time.perf_counter()
        pipe.submit(bgr.data_ptr(), dep.data_ptr(), res[n[0] % 4].data_ptr())
        t1 = time.perf_counter()
        n[0] += 1
        return (t1 - t0) * 1e6

    for _ in range(a.warmup):
        submit()
    pipe.drain()
    print("library %s, %d pairs of %dx%dx%d, %d steps per repeat" % (os.environ.get("REVO_HIP_SO", "(shipped)"), a.pairs, a.width, a.height, a.levels, a.steps))
    print("repeat   us/step   submit: mean   median      p90      max   share of the loop")
    for r in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        us = [submit() for _ in range(a.steps)]
        pipe.drain()
        wall = (time.perf_counter() - t0) * 1e6
        us.sort()
        print("%6d  %8.1f       %9.1f %8.1f %8.1f %8.1f   %5.1f %%" % (r, wall / a.steps, statistics.mean(us), us[len(us) // 2], us[int(len(us) * 0.9)],
                                                                     us[-1], 100.0 * sum(us) / wall))
    pipe.close()


if __name__ == "__main__":
    main()
