"""Cost of revo_map_tsdf_raycast (api.VoxelMap.surface_raycast_into; include/revo_hip.h) on one GPU, written to
profiles/map_tsdf_ray_rates.txt.

DESIGN 26's protocol and scene (profiles/map_tsdf_rates.py): the carving scene's 320x240 depth views, 2 cm voxels, a box of 256^3
cells around the map's median voxel, 8 views (the scene's four, twice) fused with their colour images, trunc 8 cm; 3 warm-up
calls, then the median of `--reps` calls, a host clock around one call and the wait for the stream, everything in device memory.
The call is timed at the default step from the eight views' own poses, once with all outputs and once with depth only, and both
again with REVO_MAP_TSDF_RAY_MASK=0, the plain march that evaluates every sample.  The yardsticks run in the same process on the
same inputs: raycast_into of the voxel map from the same poses, and mesh_into of the same volumes.

The share of samples the block mask lets the kernel skip is derived on the CPU, not counted in the kernel: the march's samples
are the call's own `samples`; a sample is evaluated when its base lies in a marked block, and once more as the predecessor of such
a sample when it was skipped itself.  (The third reason, a sample in an unmarked block behind a valid sample with F < 0, ends an
inside run and happens at most once per such run; it is not counted.)

    python profiles/map_tsdf_ray_rates.py [--reps 10] [--size 256] [--commit TEXT] [--out profiles/map_tsdf_ray_rates.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def evaluated_samples(cells, lo, voxel, view, samples, step, min_weight=1):
    """How many samples of a view's rays the masked march evaluates, by the rule in this file's head.  samples: [h, w], the
    samples each ray counts (mapfile.tsdf_raycast_records)."""
    from revo_amd import mapfile
    f32 = np.float32
    n = np.asarray(cells.shape, np.int64)
    inside = (cells["weight"] >= max(1, min_weight)) & (cells["sum"] < 0)
    near = inside[:-1, :-1, :-1].copy()  # a base one of whose corners is inside
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                near |= inside[dx:n[0] - 1 + dx, dy:n[1] - 1 + dy, dz:n[2] - 1 + dz]
    nb = (n - 1 + 7) // 8
    pad = np.zeros(tuple(nb * 8), bool)
    pad[:n[0] - 1, :n[1] - 1, :n[2] - 1] = near
    marked = pad.reshape(nb[0], 8, nb[1], 8, nb[2], 8).any((1, 3, 5))
    vw = mapfile.ray_view(*view)
    o, _, d, _ = mapfile.ray_view_rays(vw)
    zmin = vw[4][4]
    left = samples.reshape(-1).astype(np.int64)
    centre = np.asarray(lo, np.int64).astype(f32) + f32(0.5)
    top = (n - 2).astype(f32)
    prev = np.zeros(len(o), bool)
    total = 0
    with np.errstate(all="ignore"):
        for k in range(int(left.max())):
            s = f32(zmin + f32(k) * step)
            u = (o + s * d) / f32(voxel) - centre
            b = np.floor(u)
            inbox = np.all(np.isfinite(u) & (b >= 0) & (b <= top), 1)
            bi = np.where(inbox[:, None], b, 0).astype(np.int64) >> 3
            ev = inbox & marked[bi[:, 0], bi[:, 1], bi[:, 2]] & (k < left)
            total += int(ev.sum()) + (int((ev & ~prev).sum()) if k else 0)
            prev = ev
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_tsdf_ray_rates.txt"))
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
    s = cc.settings320()
    cam = api.CameraPyr(s)
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    m.merge_raw(rec)
    e = a.size
    lo, n = np.median(mapfile.key_axes(rec["key"]), 0).astype(np.int64) - e // 2, (e, e, e)
    frames = cc.scene_frames()[0]
    plain = [(torch.from_numpy(np.ascontiguousarray(D)).cuda(), T, k) for D, T, k in cc.scene_views(False)] * 2
    coloured = [v + (torch.from_numpy(np.ascontiguousarray(frames[i % 4][0])).cuda(),) for i, v in enumerate(plain)]
    poses = np.stack([np.asarray(v[1], np.float32) for v in plain])
    trunc = float(mapfile.tsdf_trunc(cc.VOXEL))
    d_tsdf = torch.zeros(n + (2,), dtype=torch.int32, device="cuda")
    d_color = torch.zeros(n + (4,), dtype=torch.int32, device="cuda")
    m.fuse_into(d_tsdf, coloured, lo, d_color=d_color)
    nv_, h, w = len(poses), s.height, s.width
    d_depth = torch.zeros((nv_, h, w), dtype=torch.float32, device="cuda")
    d_nrm = torch.zeros((nv_, h, w, 3), dtype=torch.float32, device="cuda")
    d_bgr = torch.zeros((nv_, h, w, 3), dtype=torch.uint8, device="cuda")
    d_hits = torch.zeros(nv_, dtype=torch.int32, device="cuda")
    d_info = torch.zeros(8, dtype=torch.int64, device="cuda")
    say("Views of the TSDF surface, one MI355X, source: %s" % a.commit)
    say("scene: %d views of %dx%d, voxels of %g m, trunc %g m, a box of %d^3 cells, the default step of one voxel edge; median (min .. max)"
        % (nv_, w, h, cc.VOXEL, trunc, e))
    say("of %d calls after 3 warm-up calls, a host clock around the call and its wait, everything in device memory" % a.reps)

    def full():
        m.surface_raycast_into(d_depth, d_tsdf, lo, poses, d_normals=d_nrm, d_bgr=d_bgr, d_color=d_color, d_hits=d_hits, d_info=d_info)

    def depth_only():
        m.surface_raycast_into(d_depth, d_tsdf, lo, poses)

    say("\n1. surface_raycast_into, through the block mask and (REVO_MAP_TSDF_RAY_MASK=0) without it")
    say("%-40s %10s %20s %12s" % ("call", "ms", "min .. max", "Mrays / s"))
    rows = []
    for tag, env in (("", None), (", plain march", "0")):
        if env is None:
            os.environ.pop("REVO_MAP_TSDF_RAY_MASK", None)
        else:
            os.environ["REVO_MAP_TSDF_RAY_MASK"] = env
        rows.append(("depth, normals, colours" + tag, clock(full)))
        if env is None:
            masked = [x.cpu().numpy().copy() for x in (d_depth, d_nrm, d_bgr, d_hits, d_info)]
        else:
            same = all(np.array_equal(x.cpu().numpy().view(np.uint8), y.view(np.uint8)) for x, y in zip((d_depth, d_nrm, d_bgr, d_hits, d_info), masked))
        rows.append(("depth only" + tag, clock(depth_only)))
    os.environ.pop("REVO_MAP_TSDF_RAY_MASK", None)
    for name, t in rows:
        say("%-40s %10.3f %9.3f .. %7.3f %12.1f" % (name, t[0], t[1], t[2], nv_ * h * w / t[0] / 1e3))
    info = dict(zip(mapfile.TSDF_RAY_INFO_KEYS, masked[4].tolist()))
    say("the call: %s; hits per view: %s" % (info, masked[3].tolist()))
    say("with / without the mask: %.2f (all outputs), %.2f (depth only); the two marches give the same bytes: %s"
        % (rows[0][1][0] / rows[2][1][0], rows[1][1][0] / rows[3][1][0], same))

    say("\n2. the yardsticks, same process, same poses and volumes")
    d_vbgr = torch.zeros((nv_, h, w, 3), dtype=torch.uint8, device="cuda")
    r0 = clock(lambda: m.raycast_into(d_depth, d_vbgr, poses))
    nv, nt, minfo = m.mesh_into(None, None, d_tsdf, lo)
    d_v = torch.zeros((max(nv, 1), 3), dtype=torch.float32, device="cuda")
    d_t = torch.zeros((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    m0 = clock(lambda: m.mesh_into(d_v, d_t, d_tsdf, lo))
    say("%-40s %10s %20s" % ("call", "ms", "min .. max"))
    for name, t in (("raycast_into of the voxel map, 8 views", r0), ("mesh_into of the volume", m0)):
        say("%-40s %10.3f %9.3f .. %7.3f" % (name, t[0], t[1], t[2]))
    say("the voxel map: %d voxels; the mesh: %d vertices, %d triangles" % (len(rec), nv, nt))

    say("\n3. what the mask skips, derived on the CPU from mapfile.tsdf_raycast_records over the four distinct views")
    cells = np.ascontiguousarray(d_tsdf.cpu().numpy()).view(mapfile.TSDF_CELL_DTYPE)[..., 0]
    k = cc.intrinsics320()
    views = [(poses[i], k, (w, h)) for i in range(4)]
    want = mapfile.tsdf_raycast_records(cells, None, lo, cc.VOXEL, views)
    agree = all(want["depth"][i].tobytes() == masked[0][i].tobytes() and want["normals"][i].tobytes() == masked[1][i].tobytes() for i in range(4))
    total = want["info"]["samples"]
    ev = sum(evaluated_samples(cells, lo, cc.VOXEL, views[i], want["samples"][i], np.float32(cc.VOXEL)) for i in range(4))
    say("samples of the march: %d; evaluated by the masked kernel: %d; skipped: %.1f %%; depth and normals are mapfile's bytes: %s"
        % (total, ev, 100.0 * (1.0 - ev / max(total, 1)), agree))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    m.close()
    return 0 if same and agree else 1


if __name__ == "__main__":
    sys.exit(main())
