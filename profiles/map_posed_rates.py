"""Cost of putting a registered voxel map into another map's frame (revo_map_pose_raw, revo_map_merge_posed) on one GPU.

Two maps of the same K keyframes, the second integrated at D * T_w_kf (DESIGN 16's map rows), and D^-1 as the pose.  Timed with
the wall clock around calls that wait for the device, 3 warm-up rounds, median and best of `runs`:

  pose_raw      revo_map_pose_raw(device_out = 1) into a buffer allocated beforehand, then the wait for the map's stream: the
                counting launch, the writing launch and the two waits for the counters -- no allocation, no Python wrapper work
  merge_posed   a copy of the destination takes the source under T (dst.merge_posed), then gives it back (subtract_posed, not timed)
  merge         the same copy takes the source slot by slot (dst.merge, revo_map_merge), then gives it back (subtract, not timed)

The figure of interest is merge_posed against merge on the same commit.  No rate is asserted.

    python profiles/map_posed_rates.py [--runs 10] [--out profiles/map_posed_rates.txt]
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

    D = synth.se3_exp(np.array([0.02, -0.015, 0.012, 0.006, -0.005, 0.004]))
    T = np.linalg.inv(D).astype(np.float32)
    sizes = {"320x240": ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0)),
             "640x480": ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))}
    say("voxel maps of K keyframes, the source moved by D, posed by D^-1; ms, median / best of %d" % a.runs)
    say("%-28s %9s %9s %9s %17s %17s %17s" % ("maps", "dst vox", "src vox", "moved", "pose_raw", "merge_posed", "merge"))
    for name, K, dense, voxel in (("320x240", 2, False, 0.02), ("320x240", 2, True, 0.02), ("640x480", 4, False, 0.01),
                                  ("640x480", 4, True, 0.01), ("640x480", 8, True, 0.005)):
        s = sizes[name]
        cam = api.CameraPyr(s)
        pyrs = [api.ImgPyramidRGBD(s, cam, *synth.make_pair(902 + i, s)["ref"]) for i in range(K)]
        Ts = [synth.se3_exp(np.array([0.05 * i, 0.01 * i, 0, 0, 0.03 * i, 0])) for i in range(K)]
        dst, src = api.VoxelMap(cam, voxel, dense=dense), api.VoxelMap(cam, voxel, dense=dense)
        dst.integrate_many(pyrs, [M.astype(np.float32) for M in Ts])
        src.integrate_many(pyrs, [(D @ M).astype(np.float32) for M in Ts])
        nd, ns = dst.info()["voxels"], src.info()["voxels"]
        moved = src.pose_raw(T, device=True)[1]["voxels_moved"]
        import ctypes as C
        import torch
        from revo_amd import _lib
        L = _lib.lib()
        buf = torch.empty(64 * max(ns, 1), dtype=torch.uint8, device="cuda:%d" % cam.device)
        torch.cuda.synchronize()
        Tc = np.ascontiguousarray(T.T).reshape(16)
        n = C.c_size_t()

        def pose_raw():
            _lib.check(L.revo_map_pose_raw(src._h, Tc.ctypes.data_as(_lib.f32p), C.c_float(voxel), 1, C.c_void_p(buf.data_ptr()), ns,
                                           C.byref(n), 1, None))
            src.sync()

        raw = timed(pose_raw)
        posed = timed(lambda: dst.merge_posed(src, T), lambda: dst.subtract_posed(src, T))
        plain = timed(lambda: (dst.merge(src), dst.sync()), lambda: dst.subtract(src))
        say("%-28s %9d %9d %9d %8.3f %8.3f %8.3f %8.3f %8.3f %8.3f"
            % ("%s %s x%d, %g m" % (name, "dense" if dense else "edges", K, voxel), nd, ns, moved, raw[0], raw[1], posed[0], posed[1],
               plain[0], plain[1]))
        dst.close()
        src.close()
        del pyrs
        cam.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
