"""Per-view, per-cell and per-cube restatement of the TSDF contracts (include/revo_hip.h revo_map_tsdf_fuse / revo_map_tsdf_mesh,
DESIGN 26), bit for bit.  Written as the loops the contracts describe, on top of map_carve_ref (the class of a point in a view)
and map_seen_ref (a cell's centre), without revo_amd.mapfile, whose vectorised tsdf_records / mesh_records are checked against it.

  cell     (sum int32, weight uint32); p = map_seen_ref.centre
  class    map_carve_ref.classify(p, view, 0, trunc, 0)
  update   FREE: q = 1024;  CONFIRMED: q = int(rint(((dc - z) / trunc) * 1024)), float32 operation by operation, dc the centre
           pixel's depth and z the camera-space depth of p;  every other class: none
           a cell whose weight is 2^20 takes no update (counted in saturated); else sum += q, weight += 1
  valid    weight >= max(min_weight, 1);  inside: valid and sum < 0
  cube     at cell c, corners c + {0,1}^3 inside the box; active: all eight valid
  tetra    per permutation pi of (x, y, z) in lexicographic order: c, c + e_pi0, c + e_pi0 + e_pi1, c + (1,1,1)
  edge     (cell, type = dx + 2 dy + 4 dz - 1); a vertex where the ends differ in `inside` and a tetrahedron of an active cube has it
  vertex   n0 = s0 w1, n1 = s1 w0 (int64), a = float32(float64(n0) / float64(n0 - n1)),
           pos_i = ((float32(lo_i + c_i) + 0.5) + (d_i ? a : 0)) * voxel
  triangle the table of the contract; its orientation is decided here per triangle, geometrically, in exact rational arithmetic at
           the edge midpoints: the normal points from the inside corners to the outside corners.  The 6 x 16 table plays no part.
Test infrastructure only."""
import itertools
from fractions import Fraction

import numpy as np

import map_carve_ref as mc
import map_seen_ref as sr

F = np.float32
CELL = np.dtype([("sum", "<i4"), ("weight", "<u4")])
INFO_KEYS = ("cells", "updates", "cells_weighted", "cells_inside", "saturated")
MESH_KEYS = ("cells", "valid", "inside", "cubes", "cubes_active", "vertices", "triangles")
W_MAX = 1 << 20
PERMS = tuple(itertools.permutations(range(3)))  # lexicographic
assert PERMS[1] == (0, 2, 1) and len(PERMS) == 6


def check_trunc(trunc):
    if not (np.isfinite(F(trunc)) and F(trunc) > 0):
        raise ValueError("trunc")


def depths(p, v):
    """(z, dc) of a point whose class is FREE or CONFIRMED at radius 0: the camera-space depth and the centre pixel's depth, the
    class rule's own operations."""
    px, py, pz = F(p[0]), F(p[1]), F(p[2])
    x, y, z = (((v.Rc[i, 0] * px + v.Rc[i, 1] * py) + v.Rc[i, 2] * pz) + v.tc[i] for i in range(3))
    u = (v.fx * x) / z + v.cx
    w = (v.fy * y) / z + v.cy
    return z, v.D[int(np.floor(w + F(0.5))), int(np.floor(u + F(0.5)))]


def quantum(p, v, trunc):
    """(class, q or None) of the point p in the view v."""
    trunc = F(trunc)
    cls = mc.classify(p, v, 0, trunc, F(0))
    if cls == mc.FREE:
        return cls, 1024
    if cls == mc.CONFIRMED:
        z, dc = depths(p, v)
        q = int(np.rint(((dc - z) / trunc) * F(1024)))
        assert abs(q) <= 1024
        return cls, q
    return cls, None


def fuse(voxel, lo, n, views, trunc=None, tsdf=None):
    """-> (cells CELL [n0, n1, n2], info dict, one class-count dict per view, classes [cells, n_views]).  tsdf: the volume to
    accumulate into (None: a call that does not accumulate)."""
    trunc = F(4) * F(voxel) if trunc is None else F(trunc)
    check_trunc(trunc)
    views = [v if isinstance(v, mc.View) else mc.View(*v) for v in views]
    if not 1 <= len(views) <= 64:
        raise ValueError("1 .. 64 views")
    n = [int(x) for x in n]
    out = np.zeros(n, CELL)
    cls = np.zeros((n[0] * n[1] * n[2], len(views)), np.int64)
    info = dict.fromkeys(INFO_KEYS, 0)
    info["cells"] = out.size
    c = 0
    for ix in range(n[0]):
        for iy in range(n[1]):
            for iz in range(n[2]):
                p = sr.centre(lo, (ix, iy, iz), voxel)
                s, w = (0, 0) if tsdf is None else (int(tsdf[ix, iy, iz]["sum"]), int(tsdf[ix, iy, iz]["weight"]))
                for j, v in enumerate(views):
                    cls[c, j], q = quantum(p, v, trunc)
                    if q is None:
                        continue
                    if w >= W_MAX:
                        info["saturated"] += 1
                        continue
                    s, w = s + q, w + 1
                    info["updates"] += 1
                out[ix, iy, iz] = (s, w)
                info["cells_weighted"] += w > 0
                info["cells_inside"] += w > 0 and s < 0
                c += 1
    counts = [{name: int((cls[:, j] == k).sum()) for k, name in enumerate(mc.CLASSES)} for j in range(len(views))]
    return out, {k: int(x) for k, x in info.items()}, counts, cls


def sdf(cells, trunc):
    """Metres: sum / weight * trunc / 1024 in float64, NaN where the weight is 0."""
    with np.errstate(all="ignore"):
        return np.where(cells["weight"] > 0, cells["sum"].astype(np.float64) / cells["weight"] * float(F(trunc)) / 1024.0, np.nan)


# ---------------------------------------------------------------------------------------------------------------- the mesh --
def offset(bits):
    return (bits & 1, (bits >> 1) & 1, (bits >> 2) & 1)


def tetra_corners(k):
    """The corner numbers (dx + 2 dy + 4 dz) of v0 .. v3 of the tetrahedron k."""
    p = PERMS[k]
    return (0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7)


def case_triangles(ins):
    """ins: the four `inside` flags of v0 .. v3 -> the triangles of the contract's table, each three edges (i, j), i < j, indices
    into v0 .. v3, before the orientation is decided."""
    edge = lambda a, b: (min(a, b), max(a, b))  # noqa: E731
    inside = [i for i in range(4) if ins[i]]
    outside = [i for i in range(4) if not ins[i]]
    if len(inside) in (0, 4):
        return []
    if len(inside) in (1, 3):
        a = inside[0] if len(inside) == 1 else outside[0]
        b, c, d = [i for i in range(4) if i != a]
        return [(edge(a, b), edge(a, c), edge(a, d))]
    a, b = inside
    c, d = outside
    return [(edge(a, c), edge(a, d), edge(b, d)), (edge(a, c), edge(b, d), edge(b, c))]


def outward(tri, corners, ins):
    """Whether the triangle (three edges of the tetrahedron with the corner numbers `corners`), taken at the edges' midpoints, has
    its normal pointing from the inside corners to the outside corners: exact."""
    pos = [tuple(Fraction(x) for x in offset(c)) for c in corners]
    mid = [tuple((pos[i][k] + pos[j][k]) / 2 for k in range(3)) for i, j in tri]
    u = [mid[1][k] - mid[0][k] for k in range(3)]
    v = [mid[2][k] - mid[0][k] for k in range(3)]
    nrm = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    cin = [sum(pos[i][k] for i in range(4) if ins[i]) / sum(ins) for k in range(3)]
    cout = [sum(pos[i][k] for i in range(4) if not ins[i]) / (4 - sum(ins)) for k in range(3)]
    dot = sum(nrm[k] * (cout[k] - cin[k]) for k in range(3))
    assert dot != 0
    return dot > 0


def vertex(cells, lo, voxel, cell, typ):
    d = offset(typ + 1)
    lo_end = cells[cell]
    hi_end = cells[cell[0] + d[0], cell[1] + d[1], cell[2] + d[2]]
    n0 = int(lo_end["sum"]) * int(hi_end["weight"])
    n1 = int(hi_end["sum"]) * int(lo_end["weight"])
    assert abs(n0) < 1 << 51 and abs(n1) < 1 << 51
    a = F(np.float64(n0) / np.float64(n0 - n1))
    return [((F(int(lo[i]) + cell[i]) + F(0.5)) + (a if d[i] else F(0))) * F(voxel) for i in range(3)]


def mesh(cells, lo, voxel, min_weight=1):
    """-> (vertices float32 [V, 3], triangles uint32 [T, 3], info dict of MESH_KEYS)."""
    cells = np.asarray(cells)
    assert cells.dtype == CELL and cells.ndim == 3
    n = cells.shape
    mw = max(1, int(min_weight))
    place = lambda c: (c[0] * n[1] + c[1]) * n[2] + c[2]  # noqa: E731
    valid = np.zeros(n, bool)
    inside = np.zeros(n, bool)
    for c in np.ndindex(*n):
        valid[c] = int(cells[c]["weight"]) >= mw
        inside[c] = valid[c] and int(cells[c]["sum"]) < 0
    info = dict.fromkeys(MESH_KEYS, 0)
    info.update(cells=cells.size, valid=int(valid.sum()), inside=int(inside.sum()))
    edges = set()
    cubes = []
    for c in np.ndindex(*[max(0, x - 1) for x in n]):
        info["cubes"] += 1
        corner = [(c[0] + o[0], c[1] + o[1], c[2] + o[2]) for o in map(offset, range(8))]
        if not all(valid[x] for x in corner):
            continue
        info["cubes_active"] += 1
        cubes.append((c, corner))
        for k in range(6):
            tc = tetra_corners(k)
            for i, j in itertools.combinations(range(4), 2):
                if inside[corner[tc[i]]] != inside[corner[tc[j]]]:
                    edges.add((place(corner[tc[i]]), (tc[i] ^ tc[j]) - 1, corner[tc[i]]))
    edges = sorted(edges)
    index = {(e[0], e[1]): i for i, e in enumerate(edges)}
    vertices = np.array([vertex(cells, lo, voxel, e[2], e[1]) for e in edges], F).reshape(-1, 3)
    triangles = []
    for c, corner in cubes:  # ascending place: np.ndindex's order
        for k in range(6):
            tc = tetra_corners(k)
            ins = [bool(inside[corner[x]]) for x in tc]
            for tri in case_triangles(ins):
                if not outward(tri, tc, ins):
                    tri = (tri[0], tri[2], tri[1])
                triangles.append([index[(place(corner[tc[i]]), (tc[i] ^ tc[j]) - 1)] for i, j in tri])
    info["vertices"], info["triangles"] = len(vertices), len(triangles)
    return vertices, np.array(triangles, np.uint32).reshape(-1, 3), info


def swap_table():
    """The 6 x 16 table from the geometric rule: bit `case` of entry k is set when the triangles of the tetrahedron k in the case
    (bit i: v_i inside) are listed with their last two vertices swapped."""
    out = []
    for k in range(6):
        word = 0
        for case in range(1, 15):
            ins = [bool((case >> i) & 1) for i in range(4)]
            flips = {not outward(t, tetra_corners(k), ins) for t in case_triangles(ins)}
            assert len(flips) == 1  # both triangles of a quad turn the same way
            word |= int(flips.pop()) << case
        out.append(word)
    return out
