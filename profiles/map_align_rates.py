"""Cost of registering two voxel maps (revo_map_align_eval, revo_map_align, api.align_maps) on one GPU.

Two maps of the same K keyframes, the second integrated at D * T_w_kf for a twist D of about 1.4 voxels and 0.009 rad.  Timed
with the wall clock around calls that wait for the device, 3 warm-up rounds, median and best of `runs`:

  eval       one revo_map_align_eval of one pose (the two cache launches, the search launch, the record's way back), as source
             voxels per second -- for a few map sizes (edge and dense clouds, 320x240 and 640x480)
  eval x8    the same call with 8 poses in its one launch, per pose
  ladder     api.align_maps from the identity (shifts 2, 1, 0: coarsening both maps, a Gauss-Newton loop per level), in ms, with
             its iterations and the distance of its result from D^-1

The ladder's pose is printed so that it can be compared with the specification's (tests/map_align_ref.py).  No rate is asserted.

    python profiles/map_align_rates.py [--runs 20] [--out profiles/map_align_rates.txt]
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from revo_amd import api, synth
    from revo_amd.settings import ImgPyramidSettings
    lines = []

    def say(line):
        print(line)
        sys.stdout.flush()
        lines.append(line)

    def timed(body):
        ts = []
        for r in range(a.runs + 3):
            t0 = time.perf_counter()
            body()
            dt = time.perf_counter() - t0
            if r >= 3:
                ts.append(dt)
        return float(np.median(ts)), min(ts)

    D = synth.se3_exp(np.array([0.02, -0.015, 0.012, 0.006, -0.005, 0.004]))
    near = (synth.se3_exp(np.array([0.003, -0.002, 0.002, 0.001, -0.001, 0.0005])) @ np.linalg.inv(D)).astype(np.float32)  # mm from alignment
    sizes = {"320x240": ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0)),
             "640x480": ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))}
    say("voxel maps of K keyframes against the same keyframes moved by 1.4 voxels / 0.009 rad; median / best of %d" % a.runs)
    say("%-28s %9s %9s %14s %14s %14s" % ("maps", "dst vox", "src vox", "eval ms", "Mvox/s", "eval x8 ms/pose"))
    for name, K, dense, voxel in (("320x240", 2, False, 0.02), ("320x240", 2, True, 0.02), ("640x480", 4, False, 0.01),
                                  ("640x480", 4, True, 0.01), ("640x480", 8, True, 0.005)):
        s = sizes[name]
        cam = api.CameraPyr(s)
        pyrs = [api.ImgPyramidRGBD(s, cam, *synth.make_pair(902 + i, s)["ref"]) for i in range(K)]
        Ts = [synth.se3_exp(np.array([0.05 * i, 0.01 * i, 0, 0, 0.03 * i, 0])) for i in range(K)]
        dst, src = api.VoxelMap(cam, voxel, dense=dense), api.VoxelMap(cam, voxel, dense=dense)
        dst.integrate_many(pyrs, [T.astype(np.float32) for T in Ts])
        src.integrate_many(pyrs, [(D @ T).astype(np.float32) for T in Ts])
        nd, ns = dst.info()["voxels"], src.info()["voxels"]
        one = timed(lambda: dst.align_eval(src, near))
        eight = timed(lambda: dst.align_eval(src, [near] * 8))
        say("%-28s %9d %9d %6.3f %6.3f %14.2f %8.3f %6.3f" % ("%s %s x%d, %g m" % (name, "dense" if dense else "edges", K, voxel), nd, ns,
                                                             1e3 * one[0], 1e3 * one[1], ns / one[0] / 1e6, 1e3 * eight[0] / 8, 1e3 * eight[1] / 8))
        r = {}

        def ladder():
            r.update(api.align_maps(dst, src))

        lad = timed(ladder)
        E = r["T"].astype(np.float64) @ D
        say("    ladder %8.2f %8.2f ms, iterations %s, status %d, matched %d of %d, %.3g m %.3g rad from D^-1"
            % (1e3 * lad[0], 1e3 * lad[1], [lv["iterations"] for lv in r["levels"]], r["status"], r["info"].matched, r["info"].considered,
               float(np.linalg.norm(E[:3, 3])), synth.rot_angle(np.eye(3), E[:3, :3])))
        say("    T = %s" % np.array2string(r["T"].reshape(-1), precision=9, max_line_width=200))
        dst.close()
        src.close()
        del pyrs
        cam.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
