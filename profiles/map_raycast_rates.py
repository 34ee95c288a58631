"""Cost of casting rays through the voxel map (api.VoxelMap.raycast_into / cast_rays; revo_map_raycast, revo_map_cast_rays in
include/revo_hip.h) on one GPU, written to profiles/map_raycast_rates.txt.

Device time of one call through revo_map_raycast_last_ms (HIP events on the tracker stream from the start of the block-table
launch to the end of the march; device outputs), 3 warm-up calls, then median and best of `--reps` calls:

  1. views: the carving scene's map (tests/map_carve_cases.py: two dense 320x240 keyframes, 2 cm) at 320x240, and a dense 1 cm map
     of `--kfs` 640x480 synth keyframes at 640x480; 1 and 16 views per call (the keyframe poses, cycled); with the block table and
     without it (REVO_MAP_RAYCAST_BLOCKS=0); beside each, revo_map_render at splat_max = 4 from the same poses
     (revo_map_render_last_ms);
  2. cast_rays: 2^16 and 2^20 rays of the 640x480 map's views (their pixels' rays, cycled), device in and out.

    python profiles/map_raycast_rates.py [--reps 20] [--kfs 4] [--out profiles/map_raycast_rates.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kfs", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_raycast_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import _lib, api, mapfile, synth
    from revo_amd.settings import ImgPyramidSettings, MapRayParams
    import map_carve_cases as cc
    lines = []

    def say(text=""):
        print(text)
        sys.stdout.flush()
        lines.append(text)

    # the scene map: built from its records; the 640x480 map: integrated from synth keyframes
    s320 = cc.settings320()
    cam320 = api.CameraPyr(s320)
    scene = api.VoxelMap(cam320, cc.VOXEL, dense=True)
    scene.merge_raw(cc.scene_records().astype(mapfile.RAW_DTYPE))
    scene_poses = [T.astype(np.float32) for T in cc.poses()[:2]]
    s640 = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
    cam640 = api.CameraPyr(s640)
    seq = synth.make_sequence(77, s640, 2 * a.kfs, max_t=0.02, max_rot_deg=1.0)[::2]
    big = api.VoxelMap(cam640, 0.01, dense=True)
    big.integrate_many([api.ImgPyramidRGBD(s640, cam640, f[0], f[1]) for f in seq], [np.asarray(f[3], np.float32) for f in seq])
    big_poses = [np.asarray(f[3], np.float32) for f in seq]

    say("Rays through the voxel map, one MI355X; device time per call over its views, median / best of %d calls after 3 warm-up calls" % a.reps)
    say("\n1. views (us per view): raycast_into with and without the block table, render_into at splat_max 4 from the same poses")
    say("%-22s %9s %10s %6s %7s %10s %10s %10s %12s" % ("map", "voxels", "slots", "views", "blocks", "median", "best", "hit pixels", "cells / ray"))
    NV = 16
    for name, m, s, poses in (("scene 2 cm, 320x240", scene, s320, scene_poses), ("dense 1 cm, 640x480", big, s640, big_poses)):
        info = m.info()
        dd = torch.empty((NV, s.height, s.width), dtype=torch.float32, device="cuda")
        db = torch.empty((NV, s.height, s.width, 3), dtype=torch.uint8, device="cuda")
        dh = torch.empty((NV,), dtype=torch.int32, device="cuda")
        di = torch.empty((8,), dtype=torch.int64, device="cuda")
        for n in (1, NV):
            P = [poses[k % len(poses)] for k in range(n)]
            for blocks in (1, 0):
                os.environ["REVO_MAP_RAYCAST_BLOCKS"] = str(blocks)
                ms = []
                for r in range(3 + a.reps):
                    m.raycast_into(dd[:n], db[:n], P, d_hits=dh[:n], d_info=di, wait=False)
                    t = m.last_raycast_ms()
                    if r >= 3:
                        ms.append(t / n)
                i = di.cpu().numpy()
                say("%-22s %9d %10d %6d %7s %10.1f %10.1f %10d %12.1f" % (name, info["voxels"], info["capacity"], n, "on" if blocks else "off",
                                                                        1e3 * np.median(ms), 1e3 * min(ms), int(dh[0].item()), i[5] / max(1, i[0])))
            os.environ.pop("REVO_MAP_RAYCAST_BLOCKS", None)
            ms = []
            for r in range(3 + a.reps):
                m.render_into(dd[:n], db[:n], P, splat_max=4, d_covered=dh[:n], wait=False)
                t = m.last_render_ms()
                if r >= 3:
                    ms.append(t / n)
            say("%-22s %9d %10d %6d %7s %10.1f %10.1f %10d %12s" % (name, info["voxels"], info["capacity"], n, "splat", 1e3 * np.median(ms),
                                                                  1e3 * min(ms), int(dh[0].item()), "-"))

    say("\n2. cast_rays on the dense 1 cm map (device in and out): the rays of its views' pixels, cycled")
    say("%10s %7s %10s %10s %12s %10s %12s" % ("rays", "blocks", "median ms", "best ms", "Mrays / s", "hits", "cells / ray"))
    k = (s640.fx, s640.fy, s640.cx, s640.cy, s640.depth_min, s640.depth_max)
    per_view = [np.concatenate([o, s0[:, None], d, s1[:, None]], 1) for o, s0, d, s1 in
                (mapfile.ray_view_rays(mapfile.ray_view(T, k, (s640.width, s640.height))) for T in big_poses)]
    pool = np.concatenate(per_view).astype(np.float32)
    L = _lib.lib()
    for n in (1 << 16, 1 << 20):
        rays = pool[np.arange(n) * 7 % len(pool)]  # a stride through the views: neighbours in the buffer are not neighbours in a view
        d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
        d_out = torch.empty(16 * n, dtype=torch.uint8, device="cuda")
        di = torch.empty((8,), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        prm = MapRayParams(4096)
        for blocks in (1, 0):
            os.environ["REVO_MAP_RAYCAST_BLOCKS"] = str(blocks)
            ms = []
            for r in range(3 + a.reps):
                _lib.check(L.revo_map_cast_rays(big._h, n, C.c_void_p(d_rays.data_ptr()), 1, 1, C.byref(prm), C.c_void_p(d_out.data_ptr()), 1,
                                                C.c_void_p(di.data_ptr())))
                t = big.last_raycast_ms()
                if r >= 3:
                    ms.append(t)
            i = di.cpu().numpy()
            say("%10d %7s %10.3f %10.3f %12.1f %10d %12.1f" % (n, "on" if blocks else "off", np.median(ms), min(ms), n / np.median(ms) / 1e3,
                                                             i[1], i[5] / max(1, i[0])))
        os.environ.pop("REVO_MAP_RAYCAST_BLOCKS", None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
