"""numpy specification of the registration of point sets against a voxel map's distance field (include/revo_hip.h
revo_map_df_align_eval / revo_map_df_align_system / revo_map_df_align), bit for bit.

Every float32 operation below is one numpy float32 operation (no fused multiply-add), in the order the header states; the
sums go through exact_sums_ref, the loop is map_plane_ref.gauss_newton (revo_align_host.h's arithmetic written out).
Test infrastructure only: nothing under revo_amd/ imports it."""
import ctypes as C

import numpy as np

import exact_sums_ref as xr
import map_align_ref as mar
import map_plane_ref as mpr

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
CONVERGED, ITER_LIMIT, LOST = mar.CONVERGED, mar.ITER_LIMIT, mar.LOST


class DfAlignInfo(C.Structure):
    """revo_map_df_align_info, field by field (written without revo_amd.settings, which is checked against it)."""
    _fields_ = [("S", C.c_float * 28), ("matched", C.c_uint64), ("considered", C.c_uint64), ("skipped", C.c_uint64),
                ("centre", C.c_float * 3), ("max_dist", C.c_float), ("R", C.c_float * 9), ("T", C.c_float * 3),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(DfAlignInfo) == 208


def lerp(x0, x1, w):
    """x0 + w * (x1 - x0): one subtraction, one product, one addition."""
    d = x1 - x0
    t = w * d
    return x0 + t


def interpolate(d2, lo, voxel, points, T):
    """The per-point part up to the gate, at the pose T (4x4 float32) -> dict of arrays over ALL points: ok (inside the
    interpolation cells and finite), none (a corner holds NONE), pt [N, 3], w [N, 3], c (the interpolant in cells), g [N, 3]
    (its derivative) and e (metres); c, g and e are only meaningful where ok & ~none."""
    d2 = np.asarray(d2, np.uint32)
    n = np.asarray(d2.shape, np.int64)
    lo = np.asarray(lo, np.int64).reshape(3)
    p = np.asarray(points, F).reshape(-1, 3)
    T = np.asarray(T, F)
    v = F(voxel)
    with np.errstate(all="ignore"):
        pt = np.zeros((len(p), 3), F)
        for i in range(3):
            a0 = T[i, 0] * p[:, 0]
            a1 = T[i, 1] * p[:, 1]
            a2 = T[i, 2] * p[:, 2]
            pt[:, i] = ((a0 + a1) + a2) + T[i, 3]
        q = pt / v
        g = q - F(0.5)
        f = np.floor(g)
        w = g - f
        a = f - lo.astype(F)
        assert g.dtype == F and w.dtype == F and a.dtype == F
        ok = np.all(np.isfinite(pt) & np.isfinite(g) & (a >= F(0)) & (a <= (n - 2).astype(F)), axis=1)
    ai = np.where(ok[:, None], a, F(0)).astype(np.int64)
    ai = np.minimum(ai, np.maximum(n - 2, 0))  # points that are not ok read cell 0 of a box that may have one cell on an axis
    top = np.minimum(ai + 1, n - 1)
    corner = {}
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                x, y, z = (top if i else ai)[:, 0], (top if j else ai)[:, 1], (top if k else ai)[:, 2]
                corner[i, j, k] = d2[x, y, z]
    none = np.zeros(len(p), bool)
    for val in corner.values():
        none |= val == NONE
    with np.errstate(all="ignore"):
        s = {key: np.sqrt(val.astype(F)) for key, val in corner.items()}
        wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
        m = {(i, j): lerp(s[i, j, 0], s[i, j, 1], wz) for i in (0, 1) for j in (0, 1)}
        dz = {(i, j): s[i, j, 1] - s[i, j, 0] for i in (0, 1) for j in (0, 1)}
        l_ = [lerp(m[i, 0], m[i, 1], wy) for i in (0, 1)]
        h_ = [m[i, 1] - m[i, 0] for i in (0, 1)]
        k_ = [lerp(dz[i, 0], dz[i, 1], wy) for i in (0, 1)]
        c = lerp(l_[0], l_[1], wx)
        gx = l_[1] - l_[0]
        gy = lerp(h_[0], h_[1], wx)
        gz = lerp(k_[0], k_[1], wx)
        e = c * v
    assert c.dtype == F and gx.dtype == F and gy.dtype == F and gz.dtype == F and e.dtype == F
    return dict(ok=ok, none=none, pt=pt, w=w, c=c, g=np.stack([gx, gy, gz], 1), e=e)


def terms_of(u, g, e):
    """The 28 float term arrays of the accepted points: J_i J_j (i <= j, row by row), J_i e, e e with J = (g, u x g)."""
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    gx, gy, gz = g[:, 0], g[:, 1], g[:, 2]
    J = [gx, gy, gz, uy * gz - uz * gy, uz * gx - ux * gz, ux * gy - uy * gx]
    return [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * e for i in range(6)] + [e * e]


def df_align_eval(d2, lo, voxel, points, T, max_dist, centre=(0, 0, 0)):
    """The record revo_map_df_align_eval writes for one pose (a DfAlignInfo)."""
    T = np.asarray(T, F)
    out = DfAlignInfo()
    c = np.asarray(centre, F).reshape(3)
    out.centre[:] = c.tolist()
    out.max_dist = F(max_dist)
    # a NaN pose keeps its bits: R (column-major, as given) and T bytewise
    C.memmove(C.addressof(out) + DfAlignInfo.R.offset, np.ascontiguousarray(T[:3, :3].T).tobytes(), 36)
    C.memmove(C.addressof(out) + DfAlignInfo.T.offset, np.ascontiguousarray(T[:3, 3]).tobytes(), 12)
    if not np.all(np.isfinite(T[:3, :4])) or not mar.is_orthogonal(T[:3, :3]):
        out.flags = 1
        return out
    r = interpolate(d2, lo, voxel, points, T)
    live = r["ok"] & ~r["none"]
    with np.errstate(all="ignore"):
        acc = live & (r["e"] <= F(max_dist))
    u = r["pt"][acc] - c
    for i, t in enumerate(terms_of(u, r["g"][acc], r["e"][acc])):
        assert t.dtype == F
        out.S[i] = xr.round_exact_f32(t)
    out.matched, out.considered, out.skipped = int(acc.sum()), len(r["ok"]), int((~live).sum())
    return out


def system(info):
    """revo_map_df_align_system: revo_map_align_plane_system's arithmetic."""
    return mpr.system(info)


def default_centre(points, T_init):
    """The mean of the points under T_init, in float64, rounded to float32 (api.align_maps' rule)."""
    p = np.asarray(points, F).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T_init, F).astype(np.float64)
    return (T[:3, :3] @ p.mean(0) + T[:3, 3]).astype(F)


def df_align(d2, lo, voxel, points, T_init, max_dist, centre, max_iters=30, eps_t=1e-6, eps_r=1e-6, min_matched=12, seen=None):
    """revo_map_df_align's loop -> (T_out 4x4 float32, DfAlignInfo at T_out, iterations, status); seen: a list that collects
    every record in the order it was evaluated."""
    def evaluate(T):
        rec = df_align_eval(d2, lo, voxel, points, T, max_dist, centre)
        if seen is not None:
            seen.append(rec)
        return rec

    return mpr.gauss_newton(evaluate, system, T_init, centre, max_iters, eps_t, eps_r, min_matched)
