"""Per-voxel restatement of the free-space carving contract (include/revo_hip.h revo_map_carve_eval / revo_map_carve),
bit for bit.  Written as the loop the contract describes, one voxel and one view at a time, without revo_amd.mapfile, whose
vectorised carve_records is checked against it.  All arithmetic is float32 scalars, every operation rounded on its own.

  view     Rc = R^T of T_w_c, tc_i = -(((Rc_i0 tx) + (Rc_i1 ty)) + (Rc_i2 tz))   (map_render_ref.world_to_camera)
  voxel    candidates have count >= max(min_count, 1) and, when max_count != 0, count <= max_count;
           p = float32(float64(sum_q) / float64(count) * 2^-20)
  class    OUTSIDE    pc = ((Rc[:,0] px + Rc[:,1] py) + Rc[:,2] pz) + tc not finite, z <= zmin, z >= zmax,
                      u = (fx x) / z + cx or v = (fy y) / z + cy not finite or |u|, |v| >= 2^20, or the window
                      [iu - r, iu + r] x [iv - r, iv + r] around iu = floor(u + 0.5), iv = floor(v + 0.5) not wholly in the image
           UNKNOWN    a depth of the window is not finite, <= zmin or >= zmax
           FREE       z < dmin - (margin + margin_rel dmin), dmin the window's minimum
           CONFIRMED  |z - dc| <= mc, with dc = D[iv, iu], mc = margin + margin_rel dc
           OCCLUDED   z > dc + mc
           EDGE       the rest
  carved   FREE in at least max(min_views, 1) views; the carved voxels' whole records leave the map."""
import math

import numpy as np

import map_records_ref as mrr
import map_render_ref as mr
import voxel_map_ref as ref

F = np.float32
OUTSIDE, UNKNOWN, FREE, CONFIRMED, OCCLUDED, EDGE = range(6)
CLASSES = ("outside", "unknown", "free", "confirmed", "occluded", "edge")
INFO_KEYS = ("voxels_considered", "voxels_carved", "points_carved", "votes")
U_LIMIT = F(1 << 20)


class View:
    """One checked view: depth [h, w] float32, T_w_c 4x4, intrinsics (fx, fy, cx, cy, zmin, zmax)."""

    def __init__(self, depth, T_w_c, intrinsics):
        self.D = np.ascontiguousarray(np.asarray(depth, F))
        self.T = np.asarray(T_w_c, F).reshape(4, 4)
        self.fx, self.fy, self.cx, self.cy, self.zmin, self.zmax = (F(x) for x in intrinsics)
        check_view(self)
        self.Rc, self.tc = mr.world_to_camera(self.T)
        self.h, self.w = self.D.shape


def is_orthogonal(R):
    """|R R^T - I|_F < 1e-5 and det > 0 in float32 (revo_map_align_eval's rule)."""
    R = np.asarray(R, F)
    n2 = F(0)
    for r in range(3):
        for c in range(3):
            v = (R[r, 0] * R[c, 0] + R[r, 1] * R[c, 1]) + R[r, 2] * R[c, 2]
            v = v - (F(1) if r == c else F(0))
            n2 = n2 + v * v
    det = ((R[0, 0] * (R[1, 1] * R[2, 2] - R[1, 2] * R[2, 1]) - R[0, 1] * (R[1, 0] * R[2, 2] - R[1, 2] * R[2, 0]))
           + R[0, 2] * (R[1, 0] * R[2, 1] - R[1, 1] * R[2, 0]))
    return bool(np.sqrt(n2) < F(1e-5) and det > 0)


def check_view(v):
    if v.D.ndim != 2 or not (1 <= v.D.shape[0] <= 2048 and 1 <= v.D.shape[1] <= 2048):
        raise ValueError("image size")
    k = [v.fx, v.fy, v.cx, v.cy, v.zmin, v.zmax]
    if not all(np.isfinite(x) for x in k) or not (v.fx > 0 and v.fy > 0) or not (v.zmin >= 0 and v.zmin < v.zmax):
        raise ValueError("intrinsics or depth range")
    if not np.all(np.isfinite(v.T)) or not is_orthogonal(v.T[:3, :3]):
        raise ValueError("pose")


def check_params(radius, margin, margin_rel):
    if not 0 <= int(radius) <= 3:
        raise ValueError("radius")
    for x in (F(margin), F(margin_rel)):
        if not (np.isfinite(x) and x >= 0):
            raise ValueError("margin")


def usable(d, v):
    return bool(np.isfinite(d) and d > v.zmin and d < v.zmax)


def classify(p, v, r, margin, margin_rel):
    """The class of the point p (three float32) in the view v."""
    px, py, pz = F(p[0]), F(p[1]), F(p[2])
    with np.errstate(all="ignore"):
        x, y, z = (((v.Rc[i, 0] * px + v.Rc[i, 1] * py) + v.Rc[i, 2] * pz) + v.tc[i] for i in range(3))
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)) or z <= v.zmin or z >= v.zmax:
            return OUTSIDE
        u = (v.fx * x) / z + v.cx
        w = (v.fy * y) / z + v.cy
        if not (abs(u) < U_LIMIT and abs(w) < U_LIMIT):  # NaN / inf fail the comparison
            return OUTSIDE
        iu, iv = int(math.floor(u + F(0.5))), int(math.floor(w + F(0.5)))
        if iu - r < 0 or iu + r > v.w - 1 or iv - r < 0 or iv + r > v.h - 1:
            return OUTSIDE
        win = [v.D[iv + dy, iu + dx] for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
        if not all(usable(d, v) for d in win):
            return UNKNOWN
        dmin = min(win)
        if z < dmin - (margin + margin_rel * dmin):
            return FREE
        dc = v.D[iv, iu]
        mc = margin + margin_rel * dc
        if abs(z - dc) <= mc:
            return CONFIRMED
        return OCCLUDED if z > dc + mc else EDGE


def carve_eval(rec, voxel, views, radius=1, min_views=1, min_count=1, max_count=0, margin=None, margin_rel=0.0):
    """-> (the carved voxels' records in ascending key order, info dict, one class-count dict per view, classes [n_candidates,
    n_views]).  rec: canonical records; views: View objects or (depth, T_w_c, intrinsics) tuples."""
    margin = F(voxel if margin is None else margin)
    margin_rel = F(margin_rel)
    check_params(radius, margin, margin_rel)
    views = [v if isinstance(v, View) else View(*v) for v in views]
    if not 1 <= len(views) <= 64:
        raise ValueError("1 .. 64 views")
    sel = rec["count"] >= max(1, int(min_count))
    if int(max_count):
        sel &= rec["count"] <= int(max_count)
    cand = rec[sel]
    pts = ref.mean_position(cand["sum_q"], cand["count"].astype(np.int64)).reshape(-1, 3)
    cls = np.zeros((len(cand), len(views)), np.int64)
    for i, p in enumerate(pts):
        for j, v in enumerate(views):
            cls[i, j] = classify(p, v, int(radius), margin, margin_rel)
    votes = (cls == FREE).sum(1)
    gone = cand[votes >= max(1, int(min_views))].copy()
    info = dict(voxels_considered=len(cand), voxels_carved=len(gone), points_carved=int(gone["count"].sum()), votes=int(votes.sum()))
    counts = [{name: int((cls[:, j] == c).sum()) for c, name in enumerate(CLASSES)} for j in range(len(views))]
    return gone, info, counts, cls


def remaining(rec, gone):
    """The map without the carved voxels: whole records leave."""
    return rec[~np.isin(rec["key"], gone["key"])]


def carve(rec, voxel, views, **kw):
    """-> (the map afterwards, removed records, info, per-view counts)."""
    gone, info, counts, _ = carve_eval(rec, voxel, views, **kw)
    return remaining(rec, gone), gone, info, counts


def counters_after(counters, info):
    """The map's counters after a carve: points_integrated falls by points_carved, voxels by voxels_carved, the rest stays."""
    return dict(counters, voxels=counters["voxels"] - info["voxels_carved"],
                points_integrated=counters["points_integrated"] - info["points_carved"])


assert mrr.DTYPE.itemsize == 64
