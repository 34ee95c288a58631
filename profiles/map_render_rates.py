"""Cost of rendering views of the voxel map (api.VoxelMap.render_into, revo_map_render in include/revo_hip.h) on one GPU.

  1. Time per 640x480 view: device time of one call (HIP events on the tracker stream around its splat and resolve launches,
     VoxelMap.last_render_ms; device output, warmed) over its views.  Edge and dense maps of `--kfs` synth keyframes at their
     ground-truth poses, voxel 1 cm and 5 cm, splat_max 0 and 4, 1 and 32 views per call (the keyframe poses, cycled), with
     and without the load in front of each atomic (REVO_MAP_RENDER_SKIP=0).  Median and best of `--reps` calls.
  2. The same view the only way there was before: VoxelMap.points() (revo_map_extract: every voxel to the host, sorted) and the
     numpy z-buffer of tests/map_render_ref.py.  Wall time, median of 3.
  3. One experiment, no threshold: a keyframe pyramid built from a rendered dense view (through host arrays and
     api.ImgPyramidRGBD) against the real keyframe image, both tracked to the real next frame; pose errors against the ground
     truth.

    python profiles/map_render_rates.py [--reps 20] [--kfs 4]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kfs", type=int, default=4)
    a = ap.parse_args()
    import torch
    from revo_amd import api, synth
    from revo_amd.settings import ImgPyramidSettings, TrackerSettings
    import map_render_ref as mr
    s = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
    cam = api.CameraPyr(s)
    seq = synth.make_sequence(77, s, 2 * a.kfs, max_t=0.02, max_rot_deg=1.0)
    kfs = seq[::2]
    pyrs = [api.ImgPyramidRGBD(s, cam, f[0], f[1]) for f in kfs]
    Ts = [np.asarray(f[3], np.float32) for f in kfs]
    NV = 32
    dd = torch.empty((NV, s.height, s.width), dtype=torch.float32, device="cuda")
    db = torch.empty((NV, s.height, s.width, 3), dtype=torch.uint8, device="cuda")
    dc = torch.empty((NV,), dtype=torch.int32, device="cuda")
    print("640x480 views of maps of %d keyframes, one MI355X; device time per view, median / best of %d calls" % (a.kfs, a.reps))

    print("\n1. VoxelMap.render_into (us per view)")
    print("%6s %6s %9s %10s %6s %6s %5s %10s %10s %10s" % ("cloud", "voxel", "voxels", "slots", "splat", "views", "skip", "median",
                                                          "best", "covered"))
    maps = {}
    for dense in (False, True):
        for v in (0.01, 0.05):
            m = api.VoxelMap(cam, v, dense=dense)
            m.integrate_many(pyrs, Ts)
            info = m.info()
            maps[(dense, v)] = m
            for splat in (0, 4):
                for n in (1, NV):
                    poses = [Ts[k % len(Ts)] for k in range(n)]
                    for skip in (1, 0):
                        os.environ["REVO_MAP_RENDER_SKIP"] = str(skip)
                        ms = []
                        for r in range(3 + a.reps):
                            m.render_into(dd[:n], db[:n], poses, splat_max=splat, d_covered=dc[:n], wait=False)
                            t = m.last_render_ms()
                            if r >= 3:
                                ms.append(t / n)
                        print("%6s %6.2f %9d %10d %6d %6d %5d %10.1f %10.1f %10d"
                              % ("dense" if dense else "edges", v, info["voxels"], info["capacity"], splat, n, skip,
                                 1e3 * np.median(ms), 1e3 * min(ms), int(dc[0].item())))
                        sys.stdout.flush()
    os.environ.pop("REVO_MAP_RENDER_SKIP", None)

    print("\n2. the same view through revo_map_extract + a numpy z-buffer (ms per view, wall, median of 3), splat_max 4")
    for (dense, v), m in maps.items():
        t_ext, t_np = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            xyz, rgb, _ = m.points()
            t1 = time.perf_counter()
            ref_out = mr.render(xyz, rgb, v, mr.view_of(s, Ts[0], 4))
            t2 = time.perf_counter()
            t_ext.append(t1 - t0)
            t_np.append(t2 - t1)
        got = m.render(Ts[0], splat_max=4)
        same = got[0].tobytes() == ref_out[0].tobytes() and got[1].tobytes() == ref_out[1].tobytes() and got[2] == ref_out[2]
        print("%6s %6.2f  extract %8.2f  numpy %8.2f  total %8.2f   (same bytes as the device view: %s)"
              % ("dense" if dense else "edges", v, 1e3 * np.median(t_ext), 1e3 * np.median(t_np),
                 1e3 * (np.median(t_ext) + np.median(t_np)), same))
        sys.stdout.flush()

    print("\n3. experiment: tracking the real next frame against a keyframe built from a rendered dense view (1 cm, splat_max 4)")
    m = maps[(True, 0.01)]
    trk = api.TrackerNew(TrackerSettings(), s, cam)
    for k in range(1, len(kfs)):
        i_kf, i_next = 2 * k, 2 * k + 1
        T_ref_curr = np.linalg.inv(np.asarray(seq[i_kf][3], np.float64)) @ np.asarray(seq[i_next][3], np.float64)
        cur = api.ImgPyramidRGBD(s, cam, seq[i_next][0], seq[i_next][1])
        real = api.ImgPyramidRGBD(s, cam, seq[i_kf][0], seq[i_kf][1])
        real.makeKeyframe()
        d, b, cov = m.render(Ts[k], splat_max=4)
        model = api.ImgPyramidRGBD(s, cam, b, d)
        model.makeKeyframe()
        row = []
        for ref in (real, model):
            status, R, T, err = trk.trackFrames(np.eye(3), np.zeros(3), ref, cur)
            er, et = synth.pose_error(R, T, T_ref_curr)
            row.append((status, er, et, err))
        print("keyframe %d -> frame %d: real keyframe %.2e rad %.2e m (status %d, err %.4f) | rendered keyframe %.2e rad %.2e m "
              "(status %d, err %.4f), view covered %.1f %%"
              % (i_kf, i_next, row[0][1], row[0][2], row[0][0], row[0][3], row[1][1], row[1][2], row[1][0], row[1][3],
                 100.0 * cov / (s.width * s.height)))


if __name__ == "__main__":
    main()
