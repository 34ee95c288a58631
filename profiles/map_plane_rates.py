"""Cost of point-to-plane registration of two voxel maps (revo_map_normals, revo_map_align_plane_eval, api.align_maps with
metric="plane") on one GPU, beside the point-to-point figures of the same maps (profiles/map_align_rates.py).

Two maps of the same K keyframes, the second integrated at D * T_w_kf for a twist D of about 1.4 voxels and 0.009 rad.  Timed
with the wall clock around calls that wait for the device, 3 warm-up rounds, median and best of `runs`:

  normals    VoxelMap.normals' device part is the normal cache of every point-to-plane call: timed as the difference between one
             align_plane_eval and one align_eval of the same pose (the means and the search are in both), and as the whole
             normals() call (cache, export, sort on the host)
  eval       one align_plane_eval of one pose, and of 8 poses in its one launch, per pose; align_eval alongside
  ladder     api.align_maps from the identity (shifts 2, 1, 0) for both metrics, in ms, with the iterations and the distance of
             the result from D^-1

No rate is asserted.

    python profiles/map_plane_rates.py [--runs 10] [--out profiles/map_plane_rates.txt]
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
        return 1e3 * float(np.median(ts)), 1e3 * min(ts)

    D = synth.se3_exp(np.array([0.02, -0.015, 0.012, 0.006, -0.005, 0.004]))
    near = (synth.se3_exp(np.array([0.003, -0.002, 0.002, 0.001, -0.001, 0.0005])) @ np.linalg.inv(D)).astype(np.float32)
    sizes = {"320x240": ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0)),
             "640x480": ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))}
    say("voxel maps of K keyframes against the same keyframes moved by 1.4 voxels / 0.009 rad; ms, median / best of %d" % a.runs)
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
        rec = dst.align_plane_eval(src, near)
        say("%s %s x%d, %g m: %d dst / %d src voxels, %d normals, %d matched near alignment"
            % (name, "dense" if dense else "edges", K, voxel, nd, ns, rec.dst_normals, rec.matched))
        p1, q1 = timed(lambda: dst.align_eval(src, near)), timed(lambda: dst.align_plane_eval(src, near))
        p8, q8 = timed(lambda: dst.align_eval(src, [near] * 8)), timed(lambda: dst.align_plane_eval(src, [near] * 8))
        nm = timed(lambda: dst.normals())
        say("    eval, 1 pose        point %7.3f %7.3f   plane %7.3f %7.3f   (normal cache: the difference, %.3f)"
            % (p1 + q1 + (q1[0] - p1[0],)))
        say("    eval x8, per pose   point %7.3f %7.3f   plane %7.3f %7.3f" % (p8[0] / 8, p8[1] / 8, q8[0] / 8, q8[1] / 8))
        say("    normals()           %7.3f %7.3f   (cache, export and the host's sort)" % nm)
        for metric in ("point", "plane"):
            r = {}

            def ladder():
                r.update(api.align_maps(dst, src, metric=metric))

            lad = timed(ladder)
            E = r["T"].astype(np.float64) @ D
            say("    ladder, %-5s %8.2f %8.2f ms, iterations %s, status %d, matched %d of %d, %.3g m %.3g rad from D^-1"
                % (metric, lad[0], lad[1], [lv["iterations"] for lv in r["levels"]], r["status"], r["info"].matched, r["info"].considered,
                   float(np.linalg.norm(E[:3, 3])), synth.rot_angle(np.eye(3), E[:3, :3])))
        dst.close()
        src.close()
        del pyrs
        cam.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
