"""The specification of revo_map_tsdf_track_eval (include/revo_hip.h) as a loop: per pose, per visited pixel, one float32
operation per line of arithmetic; the sums are exact (rational arithmetic over the float terms, rounded to float32 once).  The
interpolant and its gradient are map_tsdf_ray_ref's.  It knows nothing of revo_amd.mapfile.  Test infrastructure only."""
from fractions import Fraction

import numpy as np

import map_tsdf_ray_ref as rr

F = np.float32
CELL = rr.CELL
RECORD = np.dtype([("S", "<f4", (28,)), ("matched", "<u8"), ("considered", "<u8"), ("skipped", "<u8"), ("centre", "<f4", (3,)),
                   ("max_dist", "<f4"), ("R", "<f4", (9,)), ("T", "<f4", (3,)), ("flags", "<i4"), ("reserved", "<i4")])
# why a pixel leaves, or that it stays
NO_DEPTH, OUTSIDE, INVALID_CELL, GATED, ACCEPTED = range(5)
CLASSES = ("no_depth", "outside", "invalid_cell", "gated", "accepted")
MAX_POSES = 4096


def params(trunc, max_dist=None, stride=1, min_weight=1, centre=None):
    """(trunc, max_dist, stride, min_weight, centre) as the call runs with them, or ValueError."""
    tr = F(trunc)
    if not np.isfinite(tr) or not tr > 0:
        raise ValueError("trunc")
    md = F(0 if max_dist is None else max_dist)
    if not np.isfinite(md) or md < 0 or md > tr:
        raise ValueError("max_dist")
    if not 0 <= int(stride) <= 8:
        raise ValueError("stride")
    c = np.zeros(3, F) if centre is None else np.asarray(centre, F).reshape(3)
    if not np.all(np.isfinite(c)):
        raise ValueError("centre")
    return tr, (F(tr * F(0.5)) if md == 0 else md), max(1, int(stride)), max(1, int(min_weight)), c


def is_orthogonal(R):
    """revo_map_align_eval's rule on a rotation, as map_align_ref states it."""
    import map_align_ref as mar
    return mar.is_orthogonal(R)


def round_exact(terms):
    """The float32 nearest the exact sum of the float32 terms, ties to even."""
    exact = sum((Fraction(float(t)) for t in terms), Fraction(0))
    if exact == 0:
        return F(0)
    f = F(float(exact))  # a double nearest the sum, then a float: may be one step off; the neighbours decide
    best = None
    for cand in (np.nextafter(f, F(-np.inf)), f, np.nextafter(f, F(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - exact)
        even = (int(F(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, F(cand), even)
    return best[1]


def pixel(cells, lo, voxel, kq, mw, cam, R, t, md, c, x, y, D):
    """One pixel under one pose -> (class, None or the 28 float32 terms)."""
    fx, fy, cx, cy, zmin, zmax = cam
    if not (np.isfinite(D) and D > zmin and D < zmax):
        return NO_DEPTH, None
    dcx = F(F(F(x) - cx) / fx)
    dcy = F(F(F(y) - cy) / fy)
    pc = (F(dcx * D), F(dcy * D), D)
    p = [F(F(F(F(R[i, 0] * pc[0]) + F(R[i, 1] * pc[1])) + F(R[i, 2] * pc[2])) + t[i]) for i in range(3)]
    b, r = [], []
    for i in range(3):
        u = F(F(p[i] / voxel) - F(F(lo[i]) + F(0.5)))
        if not np.isfinite(u):
            return OUTSIDE, None
        bi = np.floor(u)
        if not 0 <= bi <= cells.shape[i] - 2:
            return OUTSIDE, None
        b.append(int(bi))
        r.append(F(u - F(bi)))
    f = {}
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cell = cells[b[0] + dx, b[1] + dy, b[2] + dz]
                if int(cell["weight"]) < mw:
                    return INVALID_CELL, None
                f[dx, dy, dz] = rr.field(cell)
    Fv, G = rr.interpolate(f, *r)
    e = F(Fv * kq)
    g = [F(F(G[i] * kq) / voxel) for i in range(3)]
    if not abs(e) <= md:
        return GATED, None
    u = [F(p[i] - c[i]) for i in range(3)]
    a = [F(F(u[1] * g[2]) - F(u[2] * g[1])), F(F(u[2] * g[0]) - F(u[0] * g[2])), F(F(u[0] * g[1]) - F(u[1] * g[0]))]
    J = g + a
    terms = [F(J[i] * J[j]) for i in range(6) for j in range(i, 6)] + [F(J[i] * e) for i in range(6)] + [F(e * e)]
    return ACCEPTED, terms


def track_eval(cells, lo, voxel, trunc, depth, camera, zrange, poses, max_dist=None, stride=1, min_weight=1, centre=None):
    """-> (RECORD array, one per pose; per pose the class of every visited pixel as an [lh, lw] array, None for a flagged pose)."""
    tr, md, st, mw, c = params(trunc, max_dist, stride, min_weight, centre)
    voxel = F(voxel)
    kq = F(tr / F(1024.0))
    D = np.asarray(depth, F)
    h, w = D.shape
    cam = tuple(F(x) for x in tuple(camera)[:4] + tuple(zrange))
    Ts = np.asarray(poses, F).reshape(-1, 4, 4)
    if not 1 <= len(Ts) <= MAX_POSES:
        raise ValueError("poses")
    out = np.zeros(len(Ts), RECORD)
    classes = []
    with np.errstate(all="ignore"):
        for rec, T in zip(out, Ts):
            rec["centre"], rec["max_dist"] = c, md
            rec["R"], rec["T"] = np.ascontiguousarray(T[:3, :3].T).reshape(9), T[:3, 3]
            if not np.all(np.isfinite(T[:3, :4])) or not is_orthogonal(T[:3, :3]):
                rec["flags"] = 1
                classes.append(None)
                continue
            ys, xs = range(0, h, st), range(0, w, st)
            cls = np.zeros((len(ys), len(xs)), np.int64)
            cols = [[] for _ in range(28)]
            for j, y in enumerate(ys):
                for i, x in enumerate(xs):
                    cls[j, i], terms = pixel(cells, lo, voxel, kq, mw, cam, T[:3, :3], T[:3, 3], md, c, x, y, D[y, x])
                    if terms is not None:
                        for k in range(28):
                            cols[k].append(terms[k])
            rec["S"] = [round_exact(col) for col in cols]
            rec["matched"] = int((cls == ACCEPTED).sum())
            rec["considered"] = cls.size
            rec["skipped"] = int((cls <= INVALID_CELL).sum())
            classes.append(cls)
    return out, classes
