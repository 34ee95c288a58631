"""Cost of free-space carving (revo_map_carve_eval, revo_map_carve) on one GPU, over DESIGN 16's five map rows.

A map of K keyframes (of K different synthetic rooms, as in DESIGN 16's rows: the map disagrees with itself, so there is
plenty to carve); the views are the keyframes' own depth images (device tensors) at their poses, shifted 3 cm sideways so that
something is seen through.  Timed with the wall clock around calls that wait for the device, 3 warm-up rounds, median and best of
`runs`:

  eval x1 / x8    revo_map_carve_eval, counting only (records NULL), with 1 view and with 8 views in one call: one k_map_carve launch
                  over the table and the wait for its counters
  carve ~5 %      revo_map_carve (records NULL) with the margin at which about 5 % of the voxels go (found by bisection on
                  carve_eval beforehand): the counting launch, the writing launch, the exact subtraction and its clean-up rehash;
                  the removed records are merged back between runs (not timed)
  render x1 / x8  api.VoxelMap.render_into of the same 1 and 8 poses, for scale
  subtract_raw    revo_map_subtract_raw of the same ~5 % records from a device buffer, for scale (merged back between runs, not timed)

No rate is asserted.

    python profiles/map_carve_rates.py [--runs 10] [--out profiles/map_carve_rates.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from revo_amd import api, synth
    from revo_amd.settings import ImgPyramidSettings
    lines = []

    def say(line):
        print(line)
        sys.stdout.flush()
        lines.append(line)

    def timed(body, undo=None):
        ts = []
        for r in range(a.runs + 3):
            t0 = time.perf_counter()
            body()
            dt = time.perf_counter() - t0
            if undo is not None:
                undo()
            if r >= 3:
                ts.append(dt)
        return 1e3 * float(np.median(ts)), 1e3 * min(ts)

    sizes = {"320x240": ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0)),
             "640x480": ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))}
    shift = synth.se3_exp(np.array([0.03, 0, 0, 0, 0, 0]))
    say("voxel maps of K keyframes carved with their own depth images 3 cm aside; ms, median / best of %d" % a.runs)
    say("%-28s %9s %8s %7s %15s %15s %15s %15s %15s %15s" % ("map", "voxels", "carved", "margin", "eval x1", "eval x8", "carve ~5 %",
                                                             "render x1", "render x8", "subtract_raw"))
    for name, K, dense, voxel in (("320x240", 2, False, 0.02), ("320x240", 2, True, 0.02), ("640x480", 4, False, 0.01),
                                  ("640x480", 4, True, 0.01), ("640x480", 8, True, 0.005)):
        s = sizes[name]
        cam = api.CameraPyr(s)
        frames = [synth.make_pair(902 + i, s)["ref"] for i in range(K)]
        pyrs = [api.ImgPyramidRGBD(s, cam, *f) for f in frames]
        Ts = [synth.se3_exp(np.array([0.05 * i, 0.01 * i, 0, 0, 0.03 * i, 0])) for i in range(K)]
        m = api.VoxelMap(cam, voxel, dense=dense)
        m.integrate_many(pyrs, [M.astype(np.float32) for M in Ts])
        nv = m.info()["voxels"]
        dev = "cuda:%d" % cam.device
        views = [(torch.from_numpy(np.ascontiguousarray(frames[i % K][1])).to(dev), (Ts[i % K] @ shift).astype(np.float32)) for i in range(8)]

        def quiet(fn, vs, margin):
            return fn(vs, margin=margin, records=False)[1]

        lo, hi = 0.0, 6.0  # the margin at which about 5 % of the voxels go: more margin, fewer voxels (none past DEPTH_MAX)
        for _ in range(16):
            mid = 0.5 * (lo + hi)
            if quiet(m.carve_eval, views, mid)["voxels_carved"] > 0.05 * nv:
                lo = mid
            else:
                hi = mid
        margin = hi
        gone = m.carve_eval(views, margin=margin, device=True)[0]
        carved = gone.numel() // 64
        e1 = timed(lambda: quiet(m.carve_eval, views[:1], voxel))
        e8 = timed(lambda: quiet(m.carve_eval, views, voxel))
        cv = timed(lambda: quiet(m.carve, views, margin), lambda: m.merge_raw(gone)) if carved else (float("nan"),) * 2
        d_depth = torch.empty((8, s.height, s.width), dtype=torch.float32, device=dev)
        d_bgr = torch.empty((8, s.height, s.width, 3), dtype=torch.uint8, device=dev)
        P = np.stack([v[1] for v in views])
        r1 = timed(lambda: m.render_into(d_depth[:1], d_bgr[:1], P[:1]))
        r8 = timed(lambda: m.render_into(d_depth, d_bgr, P))
        sb = timed(lambda: m.subtract_raw(gone), lambda: m.merge_raw(gone)) if carved else (float("nan"),) * 2
        assert m.info()["voxels"] == nv
        say("%-28s %9d %8d %7.4f %7.3f %7.3f %7.3f %7.3f %7.3f %7.3f %7.3f %7.3f %7.3f %7.3f %7.3f %7.3f"
            % ("%s %s x%d, %g m" % (name, "dense" if dense else "edges", K, voxel), nv, carved, margin, *e1, *e8, *cv, *r1, *r8, *sb))
        m.close()
        del pyrs
        cam.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
