"""Per-view, per-cell and per-vertex restatement of the surface contracts (include/revo_hip.h revo_map_tsdf_fuse_color /
revo_map_tsdf_mesh_attr), bit for bit, as the loops the contracts describe on top of map_tsdf_ref, without
revo_amd.mapfile, whose vectorised tsdf_records(bgr=) / mesh_attr_records are checked against it.

  colour cell  (sum_b, sum_g, sum_r, weight uint32)
  update       where the view's TSDF update of the cell takes place (the TSDF weight was below 2^20) and the class is CONFIRMED:
               sum_c += BGR[iv, iu][c], weight += 1, (iu, iv) the centre pixel of the class rule;  FREE: the TSDF cell only
  f(c)         float32(sum) / float32(weight)
  gradient     per axis: both neighbours valid (f+ - f-) * 0.5; only c + e: f+ - f(c); only c - e: f(c) - f-; neither: 0.
               A cell outside the box is not valid.
  normal       g = g0 + a (g1 - g0); l2 = (gx gx + gy gy) + gz gz; n = g / sqrt(l2); (0, 0, 0) when l2 is 0 or not finite
  colour       k = the edge's end cells with colour weight > 0; m = float32(sum_c) / float32(weight);
               k = 2: m0 + a (m1 - m0); k = 1: the coloured end's m; k = 0: 0;  byte = rint(min(max(v, 0), 255))
Every operation is a float32 operation rounded on its own.  Test infrastructure only."""
import itertools

import numpy as np

import map_carve_ref as mc
import map_seen_ref as sr
import map_tsdf_ref as tr

F = np.float32
COLOR = np.dtype([("sum_b", "<u4"), ("sum_g", "<u4"), ("sum_r", "<u4"), ("weight", "<u4")])
COLOR_KEYS = ("color_updates", "cells_colored")


def centre_pixel(p, v):
    """(iv, iu) of a point whose class is CONFIRMED at radius 0: the class rule's own operations."""
    px, py, pz = F(p[0]), F(p[1]), F(p[2])
    x, y, z = (((v.Rc[i, 0] * px + v.Rc[i, 1] * py) + v.Rc[i, 2] * pz) + v.tc[i] for i in range(3))
    u = (v.fx * x) / z + v.cx
    w = (v.fy * y) / z + v.cy
    return int(np.floor(w + F(0.5))), int(np.floor(u + F(0.5)))


def fuse_color(voxel, lo, n, views, bgr, trunc=None, tsdf=None, color=None):
    """-> (cells, info, per-view counts, colour cells COLOR [n0, n1, n2], colour info dict).  tsdf, color: the volumes to
    accumulate into (both None: a call that does not accumulate)."""
    trunc = F(4) * F(voxel) if trunc is None else F(trunc)
    tr.check_trunc(trunc)
    views = [v if isinstance(v, mc.View) else mc.View(*v) for v in views]
    if not 1 <= len(views) <= 64 or len(bgr) != len(views):
        raise ValueError("1 .. 64 views, a colour image each")
    assert (tsdf is None) == (color is None)
    n = [int(x) for x in n]
    out, cout = np.zeros(n, tr.CELL), np.zeros(n, COLOR)
    cls = np.zeros((n[0] * n[1] * n[2], len(views)), np.int64)
    info = dict.fromkeys(tr.INFO_KEYS, 0)
    info["cells"] = out.size
    cinfo = dict.fromkeys(COLOR_KEYS, 0)
    c = 0
    for ix in range(n[0]):
        for iy in range(n[1]):
            for iz in range(n[2]):
                p = sr.centre(lo, (ix, iy, iz), voxel)
                s, w = (0, 0) if tsdf is None else (int(tsdf[ix, iy, iz]["sum"]), int(tsdf[ix, iy, iz]["weight"]))
                col = [0, 0, 0, 0] if color is None else [int(x) for x in color[ix, iy, iz].tolist()]
                for j, v in enumerate(views):
                    cls[c, j], q = tr.quantum(p, v, trunc)
                    if q is None:
                        continue
                    if w >= tr.W_MAX:
                        info["saturated"] += 1
                        continue
                    s, w = s + q, w + 1
                    info["updates"] += 1
                    if cls[c, j] == mc.CONFIRMED:
                        iv, iu = centre_pixel(p, v)
                        for k in range(3):
                            col[k] += int(bgr[j][iv, iu, k])
                        col[3] += 1
                        cinfo["color_updates"] += 1
                out[ix, iy, iz] = (s, w)
                cout[ix, iy, iz] = tuple(col)
                info["cells_weighted"] += w > 0
                info["cells_inside"] += w > 0 and s < 0
                cinfo["cells_colored"] += col[3] > 0
                assert col[3] <= w and max(col[:3]) <= 255 << 20
                c += 1
    counts = [{name: int((cls[:, j] == k).sum()) for k, name in enumerate(mc.CLASSES)} for j in range(len(views))]
    return out, {k: int(x) for k, x in info.items()}, counts, cout, cinfo


# ------------------------------------------------------------------------------------------------------- the attributes --
def vertex_edges(cells, min_weight=1):
    """The (cell, type) of every vertex of tr.mesh, in its order."""
    n = cells.shape
    mw = max(1, int(min_weight))
    place = lambda c: (c[0] * n[1] + c[1]) * n[2] + c[2]  # noqa: E731
    valid = cells["weight"].astype(np.int64) >= mw
    inside = valid & (cells["sum"] < 0)
    edges = set()
    for c in np.ndindex(*[max(0, x - 1) for x in n]):
        corner = [(c[0] + o[0], c[1] + o[1], c[2] + o[2]) for o in map(tr.offset, range(8))]
        if not all(valid[x] for x in corner):
            continue
        for k in range(6):
            tc = tr.tetra_corners(k)
            for i, j in itertools.combinations(range(4), 2):
                if inside[corner[tc[i]]] != inside[corner[tc[j]]]:
                    edges.add((place(corner[tc[i]]), (tc[i] ^ tc[j]) - 1, corner[tc[i]]))
    return [(e[2], e[1]) for e in sorted(edges)]


def field(cells, c):
    return F(int(cells[c]["sum"])) / F(int(cells[c]["weight"]))


def gradient(cells, c, mw):
    n = cells.shape
    ok = lambda x: all(0 <= x[i] < n[i] for i in range(3)) and int(cells[x]["weight"]) >= mw  # noqa: E731
    g = []
    for axis in range(3):
        lo = tuple(c[i] - (i == axis) for i in range(3))
        hi = tuple(c[i] + (i == axis) for i in range(3))
        if ok(lo) and ok(hi):
            g.append((field(cells, hi) - field(cells, lo)) * F(0.5))
        elif ok(hi):
            g.append(field(cells, hi) - field(cells, c))
        elif ok(lo):
            g.append(field(cells, c) - field(cells, lo))
        else:
            g.append(F(0))
    return g


def alpha(cells, c0, c1):
    n0 = int(cells[c0]["sum"]) * int(cells[c1]["weight"])
    n1 = int(cells[c1]["sum"]) * int(cells[c0]["weight"])
    return F(np.float64(n0) / np.float64(n0 - n1))


def normal(cells, c0, c1, mw):
    a = alpha(cells, c0, c1)
    g0, g1 = gradient(cells, c0, mw), gradient(cells, c1, mw)
    with np.errstate(all="ignore"):
        g = [g0[i] + a * (g1[i] - g0[i]) for i in range(3)]
        l2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        if not np.isfinite(l2) or l2 == 0:
            return [F(0), F(0), F(0)]
        ln = np.sqrt(l2)
        return [g[i] / ln for i in range(3)]


def colour(cells, color, c0, c1):
    a = alpha(cells, c0, c1)
    w0, w1 = int(color[c0]["weight"]), int(color[c1]["weight"])
    out = []
    for name in ("sum_b", "sum_g", "sum_r"):
        m0 = F(int(color[c0][name])) / F(w0) if w0 else None
        m1 = F(int(color[c1][name])) / F(w1) if w1 else None
        v = m0 + a * (m1 - m0) if w0 and w1 else m0 if w0 else m1 if w1 else F(0)
        out.append(int(np.rint(min(max(v, F(0)), F(255)))))
    return out + [(w0 > 0) + (w1 > 0)]


def mesh_attr(cells, color, lo, voxel, min_weight=1):
    """-> (vertices, triangles, info, normals float32 [V, 3], colours uint8 [V, 4] or None)."""
    cells = np.asarray(cells)
    vertices, triangles, info = tr.mesh(cells, lo, voxel, min_weight)
    edges = vertex_edges(cells, min_weight)
    assert len(edges) == len(vertices)
    mw = max(1, int(min_weight))
    normals = np.zeros((len(edges), 3), F)
    colours = None if color is None else np.zeros((len(edges), 4), np.uint8)
    for i, (c0, typ) in enumerate(edges):
        d = tr.offset(typ + 1)
        c1 = (c0[0] + d[0], c0[1] + d[1], c0[2] + d[2])
        normals[i] = normal(cells, c0, c1, mw)
        if color is not None:
            colours[i] = colour(cells, color, c0, c1)
    return vertices, triangles, info, normals, colours
