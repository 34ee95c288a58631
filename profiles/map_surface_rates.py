"""Cost of revo_map_tsdf_fuse_color and revo_map_tsdf_mesh_attr (api.VoxelMap.fuse_into(d_color=) / mesh_into(d_normals=, d_colors=);
include/revo_hip.h) on one GPU, written to profiles/map_surface_rates.txt.

DESIGN 26's protocol and scene (profiles/map_tsdf_rates.py): the carving scene's 320x240 depth views, 2 cm voxels, a box of 256^3
cells around the map's median voxel, 8 views (the scene's four, twice), trunc 8 cm; 3 warm-up calls, then the median of `--reps`
calls, a host clock around one call and the wait for the stream, everything in device memory.  The yardsticks run in the same
process on the same inputs: fuse_into without d_color and mesh_into without the attribute outputs -- the kernels DESIGN 26
measured, whose gfx950 code this change leaves as it was.

    python profiles/map_surface_rates.py [--reps 10] [--size 256] [--commit TEXT] [--out profiles/map_surface_rates.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_surface_rates.txt"))
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
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    rec = cc.scene_records().astype(mapfile.RAW_DTYPE)
    cam = api.CameraPyr(cc.settings320())
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    m.merge_raw(rec)
    e = a.size
    lo, n = np.median(mapfile.key_axes(rec["key"]), 0).astype(np.int64) - e // 2, (e, e, e)
    frames = cc.scene_frames()[0]
    plain = [(torch.from_numpy(np.ascontiguousarray(D)).cuda(), T, k) for D, T, k in cc.scene_views(False)] * 2
    coloured = [v + (torch.from_numpy(np.ascontiguousarray(frames[i % 4][0])).cuda(),) for i, v in enumerate(plain)]
    trunc = float(mapfile.tsdf_trunc(cc.VOXEL))
    cells = e ** 3
    d_tsdf = torch.zeros(n + (2,), dtype=torch.int32, device="cuda")
    d_tsdf2 = torch.zeros(n + (2,), dtype=torch.int32, device="cuda")
    d_color = torch.zeros(n + (4,), dtype=torch.int32, device="cuda")
    d_info = torch.zeros(8, dtype=torch.int64, device="cuda")
    d_cinfo = torch.zeros(4, dtype=torch.int64, device="cuda")
    say("Colour and normals on the TSDF surface, one MI355X, source: %s" % a.commit)
    say("scene: %d views of 320x240, voxels of %g m, trunc %g m, a box of %d^3 cells; median (min .. max) of %d calls after 3 warm-up"
        % (len(plain), cc.VOXEL, trunc, e, a.reps))
    say("calls, a host clock around the call and its wait, everything in device memory")
    say("\n1. fuse_into without and with d_color")
    say("%-20s %10s %20s %16s %14s" % ("call", "ms", "min .. max", "Gcell-views / s", "GB/s written"))
    f0 = clock(lambda: m.fuse_into(d_tsdf, plain, lo, d_info=d_info))
    f1 = clock(lambda: m.fuse_into(d_tsdf2, coloured, lo, d_info=d_info, d_color=d_color, d_color_info=d_cinfo))
    for name, t, bytes_ in (("fuse_into", f0, 8), ("fuse_into, d_color", f1, 24)):
        say("%-20s %10.3f %9.3f .. %7.3f %16.2f %14.1f" % (name, t[0], t[1], t[2], cells * len(plain) / t[0] / 1e6, bytes_ * cells / t[0] / 1e6))
    info = dict(zip(mapfile.TSDF_INFO_KEYS, d_info.cpu().numpy().tolist()))
    cinfo = dict(zip(mapfile.TSDF_COLOR_INFO_KEYS, d_cinfo.cpu().numpy().tolist()))
    same = bool((d_tsdf == d_tsdf2).all().item())
    say("with / without colour: %.2f; the volumes: %s %s; the tsdf bytes are the same: %s" % (f1[0] / f0[0], info, cinfo, same))
    say("\n2. mesh_into of those volumes without and with the attribute outputs")
    nv, nt, minfo = m.mesh_into(None, None, d_tsdf, lo)
    d_v = torch.zeros((max(nv, 1), 3), dtype=torch.float32, device="cuda")
    d_t = torch.zeros((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    d_n = torch.zeros((max(nv, 1), 3), dtype=torch.float32, device="cuda")
    d_c = torch.zeros((max(nv, 1), 4), dtype=torch.uint8, device="cuda")
    m0 = clock(lambda: m.mesh_into(d_v, d_t, d_tsdf, lo))
    m1 = clock(lambda: m.mesh_into(d_v, d_t, d_tsdf, lo, d_normals=d_n))
    m2 = clock(lambda: m.mesh_into(d_v, d_t, d_tsdf, lo, d_normals=d_n, d_colors=d_c, d_color=d_color))
    say("%-28s %10s %20s %14s %16s" % ("call", "ms", "min .. max", "Gcells / s", "Mvertices / s"))
    for name, t in (("mesh_into", m0), ("mesh_into, normals", m1), ("mesh_into, normals, colours", m2)):
        say("%-28s %10.3f %9.3f .. %7.3f %14.2f %16.1f" % (name, t[0], t[1], t[2], cells / t[0] / 1e6, nv / t[0] / 1e3))
    k = np.bincount(d_c[:nv, 3].cpu().numpy(), minlength=3).tolist()
    say("with normals / without: %.2f; with normals and colours / without: %.2f; the mesh: %s; vertices by k: %s" % (m1[0] / m0[0], m2[0] / m0[0], minfo, k))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    m.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
