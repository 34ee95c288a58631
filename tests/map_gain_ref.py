"""Per-pose, per-cell restatement of revo_map_view_gain's contract (include/revo_hip.h), bit for bit.  Written as the
loops the contract describes on top of the other specifications -- map_raycast_ref (the predicted depth image), map_carve_ref (a
point's class in a view) and map_seen_ref (a cell's centre, which cells are unknown) -- without revo_amd.mapfile, whose
vectorised gain_records is checked against it.  It has no cull: every cell of the box is looked at for every pose.

  camera   (fx, fy, cx, cy, zmin, zmax) and (width, height), revo_map_raycast's rules
  pose     finite with an orthogonal rotation (map_carve_ref.is_orthogonal); a pose in device memory that is not gives an
           all-zero record and casts no ray
  image    map_raycast_ref.raycast's depth of the view at the pose: the hit voxel's z, 0 for a miss; with miss_depth != 0 every
           0 becomes miss_depth
  unknown  map_seen_ref.is_unknown: not solid at min_count, (seen & 0x7F) < max(min_views, 1), bit 7 clear
  class    map_carve_ref.classify(centre, View(image, pose, camera), radius, margin, margin_rel)
  record   over the unknown cells: FREE, CONFIRMED, not OUTSIDE; hits = hit pixels (before miss_depth)
Test infrastructure only."""
import numpy as np

import map_carve_ref as mc
import map_raycast_ref as rr
import map_render_ref as mr
import map_seen_ref as sr

F = np.float32
FIELDS = ("unknown_free", "unknown_surface", "unknown_inside", "hits")
INFO_KEYS = ("poses", "cells", "unknown", "unknown_free", "unknown_surface", "unknown_inside", "rays", "ray_hits")
MAX_POSES = 4096
_images = {}


def pose_ok(T):
    T = np.asarray(T, F).reshape(4, 4)
    return bool(np.all(np.isfinite(T))) and bool(mc.is_orthogonal(T[:3, :3]))


def check_params(radius, min_views, margin, margin_rel, miss_depth, max_steps, k):
    mc.check_params(radius, margin, margin_rel)
    miss = F(miss_depth)
    if miss != 0 and not (miss > F(k[4]) and miss < F(k[5])):
        raise ValueError("miss_depth")
    if not 1 <= int(max_steps) <= 1 << 20:
        raise ValueError("max_steps")
    if int(min_views) < 0:
        raise ValueError("min_views")


def predicted(records, voxel, k, size, T, min_count, max_steps):
    """(depth [h, w] float32 with 0 = miss, hits) of the view at the pose; kept per input, the march is a slow loop."""
    key = (records.tobytes(), float(voxel), tuple(float(x) for x in k), tuple(size), np.asarray(T, F).tobytes(), int(min_count), int(max_steps))
    if key not in _images:
        v = mr.View(size[0], size[1], *k, T_w_c=T)
        got = rr.raycast(records, voxel, v, min_count, max_steps)
        _images[key] = (got["depth"].reshape(size[1], size[0]).copy(), int(got["info"]["hits"]))
    return _images[key]


def view_gain(records, voxel, lo, n, seen, view, poses, radius=1, min_views=1, margin=None, margin_rel=0.0, miss_depth=0.0, min_count=1,
              max_steps=4096, device_poses=False):
    """-> (records: one dict of FIELDS per pose, info dict of INFO_KEYS, classes int64 [poses, cells] with -1 at the cells that
    are not unknown and at every cell of a refused device pose)."""
    k, size = view
    margin = F(voxel if margin is None else margin)
    margin_rel = F(margin_rel)
    check_params(radius, min_views, margin, margin_rel, miss_depth, max_steps, k)
    poses = np.asarray(poses, F).reshape(-1, 4, 4)
    if not 1 <= len(poses) <= MAX_POSES:
        raise ValueError("1 .. 4096 poses")
    n = [int(x) for x in n]
    solid = sr.solid_cells(records, lo, n, min_count)
    cells = n[0] * n[1] * n[2]
    cls = np.full((len(poses), cells), -1, np.int64)
    out = []
    info = dict.fromkeys(INFO_KEYS, 0)
    info["poses"], info["cells"] = len(poses), cells
    info["unknown"] = sum(1 for a in np.ndindex(*n) if sr.is_unknown(solid[a], seen[a], min_views))
    for j, T in enumerate(poses):
        r = dict.fromkeys(FIELDS, 0)
        out.append(r)
        if not pose_ok(T):
            if device_poses:
                continue
            raise ValueError("pose %d" % j)
        D, r["hits"] = predicted(records, voxel, k, size, T, min_count, max_steps)
        info["rays"] += size[0] * size[1]
        if F(miss_depth) != 0:
            D = np.where(D == 0, F(miss_depth), D).astype(F)
        v = mc.View(D, T, k)
        c = 0
        for ix in range(n[0]):
            for iy in range(n[1]):
                for iz in range(n[2]):
                    if sr.is_unknown(solid[ix, iy, iz], seen[ix, iy, iz], min_views):
                        cl = mc.classify(sr.centre(lo, (ix, iy, iz), voxel), v, int(radius), margin, margin_rel)
                        cls[j, c] = cl
                        r["unknown_free"] += cl == mc.FREE
                        r["unknown_surface"] += cl == mc.CONFIRMED
                        r["unknown_inside"] += cl != mc.OUTSIDE
                    c += 1
        for f in FIELDS:
            r[f] = int(r[f])
    for f, g in (("unknown_free", "unknown_free"), ("unknown_surface", "unknown_surface"), ("unknown_inside", "unknown_inside"), ("ray_hits", "hits")):
        info[f] = sum(r[g] for r in out)
    return out, info, cls
