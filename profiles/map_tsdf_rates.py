"""Cost of revo_map_tsdf_fuse and revo_map_tsdf_mesh (api.VoxelMap.fuse_into / mesh_into; include/revo_hip.h) on one GPU,
written to profiles/map_tsdf_rates.txt.

The carving scene (tests/map_carve_cases.py: 320x240 depth views, 2 cm voxels) in a box of 256^3 cells around the map's median
voxel; 8 views: the scene's four, twice.  3 warm-up calls, then the median of `--reps` calls, a host clock around one call and
the wait for the stream, everything in device memory:

  1. fuse_into of the box from the 8 views, beside observe_into (radius 0, margin = trunc) on the same box and views -- the
     yardstick: the same class rule per cell and view, one byte per cell instead of eight;
  2. mesh_into of that volume: the counting pass alone, and counting and both emit passes.

    python profiles/map_tsdf_rates.py [--reps 10] [--size 256] [--commit TEXT] [--out profiles/map_tsdf_rates.txt]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_tsdf_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import api, mapfile
    import map_carve_cases as cc
    lines = []

    def say(text=""):
        print(text)
        sys.stdout.flush()
        lines.append(text)

    def clock(fn, reps=a.reps):
        ms = []
        for r in range(3 + reps):
            t0 = time.perf_counter()
            fn()
            if r >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms))

    rec = cc.scene_records().astype(mapfile.RAW_DTYPE)
    cam = api.CameraPyr(cc.settings320())
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    m.merge_raw(rec)
    e = a.size
    lo, n = np.median(mapfile.key_axes(rec["key"]), 0).astype(np.int64) - e // 2, (e, e, e)
    views = [(torch.from_numpy(np.ascontiguousarray(D)).cuda(), T, k) for D, T, k in cc.scene_views(False)] * 2
    trunc = float(mapfile.tsdf_trunc(cc.VOXEL))
    cells = e ** 3
    d_tsdf = torch.zeros(n + (2,), dtype=torch.int32, device="cuda")
    d_seen = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(8, dtype=torch.int64, device="cuda")
    say("TSDF fusion and meshing of the voxel map, one MI355X, source: %s" % a.commit)
    say("scene: %d views of 320x240, voxels of %g m, trunc %g m, a box of %d^3 cells; median of %d calls after 3 warm-up calls,"
        % (len(views), cc.VOXEL, trunc, e, a.reps))
    say("a host clock around the call and its wait, everything in device memory")
    say("\n1. fuse_into beside observe_into (radius 0, margin = trunc) on the same box and views")
    say("%-14s %10s %16s %14s" % ("call", "ms", "Gcell-views / s", "GB/s written"))
    ms_f = clock(lambda: m.fuse_into(d_tsdf, views, lo, d_info=d_info))
    info = dict(zip(mapfile.TSDF_INFO_KEYS, d_info.cpu().numpy().tolist()))
    ms_o = clock(lambda: m.observe_into(d_seen, views, lo, radius=0, margin=trunc))
    say("%-14s %10.3f %16.2f %14.1f" % ("fuse_into", ms_f, cells * len(views) / ms_f / 1e6, 8 * cells / ms_f / 1e6))
    say("%-14s %10.3f %16.2f %14.1f" % ("observe_into", ms_o, cells * len(views) / ms_o / 1e6, cells / ms_o / 1e6))
    say("fuse / observe: %.2f; the volume: %s" % (ms_f / ms_o, info))
    same = bool(((d_tsdf[..., 1] > 0) == (d_seen != 0)).all().item())
    say("weight > 0 exactly where the seen byte is not 0: %s" % same)
    say("\n2. mesh_into of that volume")
    nv, nt, minfo = m.mesh_into(None, None, d_tsdf, lo)
    d_v = torch.zeros((max(nv, 1), 3), dtype=torch.float32, device="cuda")
    d_t = torch.zeros((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    ms_c = clock(lambda: m.mesh_into(None, None, d_tsdf, lo))
    ms_m = clock(lambda: m.mesh_into(d_v, d_t, d_tsdf, lo))
    say("%-22s %10s %14s %16s" % ("call", "ms", "Gcells / s", "Mtriangles / s"))
    say("%-22s %10.3f %14.2f %16s" % ("count only", ms_c, cells / ms_c / 1e6, "-"))
    say("%-22s %10.3f %14.2f %16.1f" % ("count, vertices, tris", ms_m, cells / ms_m / 1e6, nt / ms_m / 1e3))
    say("the mesh: %s" % minfo)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    m.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
