"""Per-cell restatement of the known-space contracts (include/revo_hip.h revo_map_observe / revo_map_known_field /
revo_map_frontiers), bit for bit.  Written as the loops the contracts describe, one cell and one view at a time,
without revo_amd.mapfile, whose vectorised observe_records / known_field_records / frontier_records are checked against it.

  point    p_i = (float32(lo_i + a_i) + 0.5) * voxel, every operation float32
  class    map_carve_ref.classify(p, view, radius, margin, margin_rel): DESIGN 19's rule for the point p
  byte     in = accumulate ? seen[c] : 0; f = views with FREE; s = CONFIRMED in any view;
           seen[c] = ((in | s << 7) & 0x80) | min(127, (in & 0x7F) + f)
  solid    a voxel with count >= max(min_count, 1) at the cell
  known    solid, or (seen & 0x7F) >= max(min_views, 1), or seen & 0x80; otherwise unknown
  field    map_field_ref's brute force over the cells that are solid or unknown
  frontier not solid, (seen & 0x7F) >= max(min_views, 1), and a face neighbour inside the box is unknown
Test infrastructure only."""
import numpy as np

import map_carve_ref as mc
import map_field_ref as fr

F = np.float32
INFO_KEYS = ("cells", "cells_free", "cells_surface", "votes", "newly_known")
KNOWN_KEYS = fr.INFO_KEYS + ("unknown", "known_free")


def centre(lo, a, voxel):
    return tuple((F(int(lo[i]) + int(a[i])) + F(0.5)) * F(voxel) for i in range(3))


def byte(b_in, f, s):
    return ((b_in | (s << 7)) & 0x80) | min(127, (b_in & 0x7F) + f)


def observe(voxel, lo, n, views, radius=1, margin=None, margin_rel=0.0, seen=None):
    """-> (seen uint8 [n0, n1, n2], info dict, one class-count dict per view, classes [cells, n_views]).  seen: the volume to
    accumulate into (None: a call that does not accumulate)."""
    margin = F(voxel if margin is None else margin)
    margin_rel = F(margin_rel)
    mc.check_params(radius, margin, margin_rel)
    views = [v if isinstance(v, mc.View) else mc.View(*v) for v in views]
    if not 1 <= len(views) <= 64:
        raise ValueError("1 .. 64 views")
    n = [int(x) for x in n]
    out = np.zeros(n, np.uint8)
    cls = np.zeros((n[0] * n[1] * n[2], len(views)), np.int64)
    info = dict.fromkeys(INFO_KEYS, 0)
    info["cells"] = out.size
    c = 0
    for ix in range(n[0]):
        for iy in range(n[1]):
            for iz in range(n[2]):
                p = centre(lo, (ix, iy, iz), voxel)
                for j, v in enumerate(views):
                    cls[c, j] = mc.classify(p, v, int(radius), margin, margin_rel)
                f = int((cls[c] == mc.FREE).sum())
                s = int((cls[c] == mc.CONFIRMED).any())
                b_in = 0 if seen is None else int(seen[ix, iy, iz])
                b = byte(b_in, f, s)
                out[ix, iy, iz] = b
                info["cells_free"] += (b & 0x7F) != 0
                info["cells_surface"] += (b & 0x80) != 0
                info["votes"] += f
                info["newly_known"] += b_in == 0 and b != 0
                c += 1
    counts = [{name: int((cls[:, j] == k).sum()) for k, name in enumerate(mc.CLASSES)} for j in range(len(views))]
    return out, {k: int(x) for k, x in info.items()}, counts, cls


def solid_cells(records, lo, n, min_count=1):
    lo = np.asarray(lo, np.int64)
    out = np.zeros([int(x) for x in n], bool)
    for key, cnt in zip(fr.key_axes(records["key"]), records["count"]):
        a = key - lo
        if int(cnt) >= max(1, int(min_count)) and all(0 <= a[i] < n[i] for i in range(3)):
            out[tuple(a)] = True
    return out


def is_free(b, min_views):
    return (int(b) & 0x7F) >= max(1, int(min_views))


def is_unknown(solid, b, min_views):
    return not solid and not is_free(b, min_views) and not (int(b) & 0x80)


def unknown_cells(records, lo, n, seen, min_count=1, min_views=1):
    solid = solid_cells(records, lo, n, min_count)
    out = np.zeros(solid.shape, bool)
    for a in np.ndindex(*solid.shape):
        out[a] = is_unknown(solid[a], seen[a], min_views)
    return solid, out


def known_field(records, lo, n, seen, min_count=1, clamp=0, min_views=1):
    """-> (d2 uint32 [n0, n1, n2], info dict): map_field_ref.brute_force over one record per obstacle cell."""
    solid, unknown = unknown_cells(records, lo, n, seen, min_count, min_views)
    cells = np.argwhere(solid | unknown) + np.asarray(lo, np.int64)
    obst = np.zeros(len(cells), records.dtype)
    b = cells + (1 << 20)
    obst["key"] = (b[:, 0].astype(np.uint64) << np.uint64(42)) | (b[:, 1].astype(np.uint64) << np.uint64(21)) | b[:, 2].astype(np.uint64)
    obst["count"] = 1
    d2, _ = fr.brute_force(obst, lo, n, 1, clamp)
    _, info = fr.brute_force(records, lo, n, min_count, clamp)  # cells, solid, outside, below of the map itself
    info["max_d2"] = int(d2[d2 != fr.NONE].max()) if (d2 != fr.NONE).any() else 0
    info["unknown"] = int(unknown.sum())
    info["known_free"] = info["cells"] - info["solid"] - info["unknown"]
    return d2, info


def frontiers(records, lo, n, seen, min_count=1, min_views=1):
    """-> [k, 3] int32 absolute cells in ascending order of the cell's place in the box."""
    solid, unknown = unknown_cells(records, lo, n, seen, min_count, min_views)
    out = []
    for a in np.ndindex(*solid.shape):
        if solid[a] or not is_free(seen[a], min_views):
            continue
        for axis in range(3):
            for d in (-1, 1):
                b = list(a)
                b[axis] += d
                if 0 <= b[axis] < solid.shape[axis] and unknown[tuple(b)]:
                    out.append([int(lo[i]) + a[i] for i in range(3)])
                    break
            else:
                continue
            break
    return np.asarray(out, np.int32).reshape(-1, 3)
