"""Cost of taking one keyframe out of the voxel map again (revo_map_subtract_raw) on one GPU.

A dense 1 cm map of 8 640x480 keyframes (poses a few centimetres apart, so they share most voxels).  Timed with the wall clock
around calls closed by info() (waits for the map), 3 warm-up rounds, median and best of `runs`:

  subtract free   subtract_raw of one keyframe's records (device memory) from the map of the 8: the voxels only that keyframe
                  touched die, so the call ends with the pass that moves the live voxels into a fresh table
  subtract keep   the same records from a map that holds that keyframe twice (9 integrations): no voxel dies, the call ends
                  with the decision
  rebuild         the alternative without subtraction: clear, then integrate the 7 remaining keyframes again
                  (revo_map_integrate_many, one launch)

Every timed call starts from a fresh copy of the map (built by a merge_raw that is not timed) in a table that grew to its size
on its own.  Each result is compared with the map of the 7 (or 8) keyframes before its time counts.  No rate is asserted.

    python profiles/map_subtract_rates.py [--runs 20] [--voxel 0.01] [--out profiles/map_subtract_rates.txt]
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
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from revo_amd import api, synth
    from revo_amd.settings import ImgPyramidSettings
    s = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
    cam = api.CameraPyr(s)
    K, out_kf = 8, 3
    pyrs = [api.ImgPyramidRGBD(s, cam, *synth.make_pair(1300 + i, s)["ref"]) for i in range(K)]
    Ts = [synth.se3_exp(np.array([0.03 * i, 0.01 * i, 0, 0, 0.01 * i, 0])).astype(np.float32) for i in range(K)]
    rest = [i for i in range(K) if i != out_kf]

    def fresh(idx):
        m = api.VoxelMap(cam, a.voxel, dense=True)
        m.integrate_many([pyrs[i] for i in idx], [Ts[i] for i in idx])
        m.info()
        return m

    whole, one, seven = fresh(range(K)), fresh([out_kf]), fresh(rest)
    rec_whole, rec_one = whole.export_raw(), one.export_raw()
    rec_twice = fresh(list(range(K)) + [out_kf]).export_raw()
    dropped = one.info()["points_dropped"]
    d_one = torch.from_numpy(rec_one.view(np.uint8).copy()).cuda()
    want7, want8 = seven.export_raw().tobytes(), rec_whole.tobytes()
    lines = []

    def say(line):
        print(line)
        sys.stdout.flush()
        lines.append(line)

    def timed(name, start, kfs, body, want):
        ts, cap = [], 0
        for r in range(a.runs + 3):
            m = api.VoxelMap(cam, a.voxel, dense=True)
            m.merge_raw(start, dropped * (kfs - K + 1), kfs)
            cap = m.info()["capacity"]
            t0 = time.perf_counter()
            body(m)
            m.info()
            dt = time.perf_counter() - t0
            if r >= 3:
                ts.append(dt)
            if r == 0 and m.export_raw().tobytes() != want:
                raise SystemExit("%s: the map is not the map of the remaining keyframes" % name)
            m.close()
        say("%-14s %9.3f %9.3f   (table of %d slots)" % (name, 1e3 * np.median(ts), 1e3 * min(ts), cap))

    say("640x480 dense, voxel %g m, 8 keyframes: %d voxels; keyframe %d: %d records, %d voxels die with it; median / best of %d, ms"
        % (a.voxel, len(rec_whole), out_kf, len(rec_one), len(rec_whole) - seven.info()["voxels"], a.runs))
    timed("subtract free", rec_whole, K, lambda m: m.subtract_raw(d_one, dropped, 1), want7)
    timed("subtract keep", rec_twice, K + 1, lambda m: m.subtract_raw(d_one, dropped, 1), want8)

    def rebuild(m):
        m.clear()
        m.integrate_many([pyrs[i] for i in rest], [Ts[i] for i in rest])

    timed("rebuild", rec_whole, K, rebuild, want7)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
