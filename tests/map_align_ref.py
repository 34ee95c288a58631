"""numpy specification of the voxel maps' registration (include/revo_hip.h revo_map_coarsen / revo_map_align_eval /
revo_map_align_system / revo_map_align), bit for bit where the contract is bit for bit.

Maps are record arrays (map_records_ref.DTYPE, ascending keys) as voxel_map_ref / map_records_ref build them; a voxel's point is
voxel_map_ref.mean_position of its sums, and every sum of a record is exact_sums_ref.round_exact_f32 of its float32 terms.
Test infrastructure only: nothing under revo_amd/ imports it."""
import ctypes as C
import math

import numpy as np

import exact_sums_ref as xr
import map_records_ref as mrr
import voxel_map_ref as ref

F = np.float32
CONVERGED, ITER_LIMIT, LOST = 0, 1, 2


class Info(C.Structure):
    """revo_map_align_info, field by field (written without revo_amd.settings, which is checked against it)."""
    _fields_ = [("S", C.c_float * 16), ("matched", C.c_uint64), ("considered", C.c_uint64), ("skipped", C.c_uint64),
                ("centre", C.c_float * 3), ("max_dist", C.c_float), ("R", C.c_float * 9), ("T", C.c_float * 3),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(Info) == 160


def unpack_keys(key):
    """Packed keys -> N x 3 int64 unbiased indices."""
    key = np.asarray(key, np.uint64)
    m = np.uint64(0x1fffff)
    return np.stack([((key >> np.uint64(s)) & m).astype(np.int64) - ref.KEY_BIAS for s in (42, 21, 0)], 1)


def coarsen(rec, shift):
    """revo_map_coarsen: floor(k / 2^shift) per axis (numpy's >> on int64 is arithmetic), sums added per coarse key."""
    rec = np.asarray(rec, mrr.DTYPE)
    key = ref.pack_keys(unpack_keys(rec["key"]) >> shift) if len(rec) else np.zeros(0, np.uint64)
    uk, inv = np.unique(key, return_inverse=True)
    out = np.zeros(len(uk), mrr.DTYPE)
    out["key"] = uk
    np.add.at(out["count"], inv, rec["count"])
    np.add.at(out["sum_q"], inv, rec["sum_q"])
    np.add.at(out["sum_bgr"], inv, rec["sum_bgr"])
    return out


def points_of(rec, min_count):
    """(keys, xyz float32) of the voxels with count >= max(min_count, 1): what revo_map_extract returns, in key order."""
    rec = np.asarray(rec, mrr.DTYPE)
    rec = rec[rec["count"] >= max(1, int(min_count))]
    return rec["key"], ref.mean_position(rec["sum_q"], rec["count"]).reshape(-1, 3)


def is_orthogonal(R):
    """is_orthogonal of revo_track_dev.h on the row-major 3x3 float32 R: |R R^T - I|_F < 1e-5 and det > 0, float32 throughout."""
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


def matches(dst_rec, dst_voxel, src_rec, T, max_dist, min_count_dst=1, min_count_src=1):
    """Steps 1-7 of the contract at the pose T (4x4 float32, source -> destination).
    -> (p' of the accepted matches [M, 3], their q [M, 3], considered, skipped)."""
    T = np.asarray(T, F)
    _, p = points_of(src_rec, min_count_src)
    dkey, dq = points_of(dst_rec, min_count_dst)
    with np.errstate(all="ignore"):
        pt = np.stack([((T[i, 0] * p[:, 0] + T[i, 1] * p[:, 1]) + T[i, 2] * p[:, 2]) + T[i, 3] for i in range(3)], 1).astype(F).reshape(-1, 3)
        f = np.floor(pt / F(dst_voxel))
        ok = np.all(np.abs(pt) < F(ref.RANGE_M), 1) & np.all((f >= ref.KEY_MIN) & (f <= ref.KEY_MAX), 1)
    considered, skipped = len(p), int((~ok).sum())
    pt, k = pt[ok], f[ok].astype(np.int64)
    n = len(pt)
    best_d2 = np.full(n, np.inf, F)
    best_key = np.full(n, np.uint64(0xffffffffffffffff))
    best_q = np.zeros((n, 3), F)
    if len(dkey) and n:
        for ox in (-1, 0, 1):
            for oy in (-1, 0, 1):
                for oz in (-1, 0, 1):
                    kk = k + np.array([ox, oy, oz], np.int64)
                    inr = np.all((kk >= ref.KEY_MIN) & (kk <= ref.KEY_MAX), 1)
                    key = ref.pack_keys(np.where(inr[:, None], kk, 0))
                    j = np.minimum(np.searchsorted(dkey, key), len(dkey) - 1)
                    hit = inr & (dkey[j] == key)
                    q = dq[j]
                    d = pt - q
                    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                    better = hit & ((d2 < best_d2) | ((d2 == best_d2) & (key < best_key)))
                    best_d2 = np.where(better, d2, best_d2)
                    best_key = np.where(better, key, best_key)
                    best_q = np.where(better[:, None], q, best_q)
    md2 = F(max_dist) * F(max_dist)
    acc = (best_key != np.uint64(0xffffffffffffffff)) & (best_d2 <= md2)
    return pt[acc], best_q[acc], considered, skipped


def align_eval(dst_rec, dst_voxel, src_rec, T, max_dist, min_count_dst=1, min_count_src=1, centre=(0, 0, 0)):
    """The record revo_map_align_eval writes for one pose (an Info)."""
    T = np.asarray(T, F)
    out = Info()
    c = np.asarray(centre, F).reshape(3)
    out.centre[:] = c.tolist()
    out.max_dist = F(max_dist)
    out.R[:] = np.ascontiguousarray(T[:3, :3].T).reshape(9).tolist()  # column-major, as given
    out.T[:] = T[:3, 3].tolist()
    if not np.all(np.isfinite(T[:3, :4])) or not is_orthogonal(T[:3, :3]):
        # a NaN pose keeps its bits: write R and T bytewise
        C.memmove(C.addressof(out) + Info.R.offset, np.ascontiguousarray(T[:3, :3].T).tobytes(), 36)
        C.memmove(C.addressof(out) + Info.T.offset, np.ascontiguousarray(T[:3, 3]).tobytes(), 12)
        out.flags = 1
        return out
    pt, q, considered, skipped = matches(dst_rec, dst_voxel, src_rec, T, max_dist, min_count_dst, min_count_src)
    u = pt - c
    r = pt - q
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
    terms = [ux, uy, uz, ux * ux, ux * uy, ux * uz, uy * uy, uy * uz, uz * uz, rx, ry, rz,
             np.concatenate([uy * rz, -(uz * ry)]), np.concatenate([uz * rx, -(ux * rz)]), np.concatenate([ux * ry, -(uy * rx)]),
             np.concatenate([rx * rx, ry * ry, rz * rz])]
    for i, t in enumerate(terms):
        out.S[i] = xr.round_exact_f32(np.asarray(t, F))
    out.matched, out.considered, out.skipped = len(pt), considered, skipped
    return out


def system(info):
    """revo_map_align_system: (H [6, 6], g [6]) float64 for the increment x = (v, w) applied on the left about the centre."""
    S = np.array(list(info.S), np.float64)
    n = float(info.matched)

    def hat(a):
        return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], np.float64)

    su = S[0:3]
    xx, xy, xz, yy, yz, zz = S[3:9]
    H = np.zeros((6, 6))
    H[:3, :3] = n * np.eye(3)
    H[:3, 3:] = -hat(su)
    H[3:, :3] = hat(su)
    H[3:, 3:] = np.array([[yy + zz, -xy, -xz], [-xy, xx + zz, -yz], [-xz, -yz, xx + yy]])
    return H, S[9:15].copy()


def solve(H, g):
    """x of H x = -g by the Cholesky factorisation and pivot rule of revo_pair_info_covariance; None: rank-deficient."""
    L = np.zeros((6, 6))
    for j in range(6):
        p = H[j, j]
        for k in range(j):
            p -= L[j, k] * L[j, k]
        if not (p > 64.0 * 2.220446049250313e-16 * H[j, j]) or not math.isfinite(p):
            return None
        L[j, j] = math.sqrt(p)
        for i in range(j + 1, 6):
            v = H[i, j]
            for k in range(j):
                v -= L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        v = -g[i]
        for k in range(i):
            v -= L[i, k] * y[k]
        y[i] = v / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k, i] * x[k]
        x[i] = v / L[i, i]
    return x if np.all(np.isfinite(x)) else None


def min_pivot_ratio(H):
    """The smallest Cholesky pivot over its diagonal entry (the rank rule refuses <= 64 * 2^-52); 0 if the factorisation fails."""
    L = np.zeros((6, 6))
    worst = np.inf
    for j in range(6):
        p = H[j, j] - float(np.dot(L[j, :j], L[j, :j]))
        if not p > 0:
            return 0.0
        worst = min(worst, p / H[j, j])
        L[j, j] = math.sqrt(p)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - float(np.dot(L[i, :j], L[j, :j]))) / L[j, j]
    return worst


def se3_exp(x):
    """synth.se3_exp, restated: expm(hat(x)) for x = (v, w)."""
    x = np.asarray(x, np.float64)
    v, w = x[:3], x[3:]
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-10:
        a, b, c, d = 1.0, 0.0, 0.5, 0.0
    else:
        a, b = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th)
        c, d = b, (th - math.sin(th)) / (th * th * th)
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + a * W + b * (W @ W)
    E[:3, 3] = (np.eye(3) + c * W + d * (W @ W)) @ v
    return E


def align(dst_rec, dst_voxel, src_rec, T_init, max_dist, min_count_dst=1, min_count_src=1, centre=(0, 0, 0), max_iters=30,
          eps_t=1e-6, eps_r=1e-6, min_matched=12):
    """revo_map_align's loop -> (T_out 4x4 float32, Info at T_out, iterations, status)."""
    kw = dict(max_dist=max_dist, min_count_dst=min_count_dst, min_count_src=min_count_src, centre=centre)
    c = np.asarray(centre, F).astype(np.float64)
    Cp, Cm = np.eye(4), np.eye(4)
    Cp[:3, 3], Cm[:3, 3] = c, -c
    T = np.asarray(T_init, F).astype(np.float64)
    Tsys = T.copy()
    status, it = ITER_LIMIT, 0
    while it < max_iters:
        rec = align_eval(dst_rec, dst_voxel, src_rec, T.astype(F), **kw)
        x = None
        if not (rec.flags & 1) and rec.matched >= min_matched:
            x = solve(*system(rec))
        if x is None:
            status, T = LOST, Tsys
            break
        it += 1
        Tsys = T.copy()
        T = ((Cp @ se3_exp(x)) @ Cm) @ T
        if np.max(np.abs(x[:3])) < eps_t and np.max(np.abs(x[3:])) < eps_r:
            status = CONVERGED
            break
    Tf = T.astype(F)
    return Tf, align_eval(dst_rec, dst_voxel, src_rec, Tf, **kw), it, status


def default_centre(src_rec, T_init, min_count_src=1):
    """The ladder's centre: the mean of the source's points under T_init, in float64, rounded to float32."""
    _, p = points_of(src_rec, min_count_src)
    T = np.asarray(T_init, F).astype(np.float64)
    return (T[:3, :3] @ p.astype(np.float64).mean(0) + T[:3, 3]).astype(F) if len(p) else np.zeros(3, F)


def align_maps(dst_rec, src_rec, voxel, T_init=None, shifts=(2, 1, 0), centre=None, **kw):
    """api.align_maps: coarsen both maps per level, align with max_dist = that level's edge, hand the pose down.
    -> (T, Info, iterations, status) of the last level and the list of every level's."""
    T = np.eye(4, dtype=F) if T_init is None else np.asarray(T_init, F)
    if centre is None:
        centre = default_centre(src_rec, T, kw.get("min_count_src", 1))
    levels = []
    for sh in shifts:
        v = F(np.ldexp(F(voxel), sh))
        d, s = (dst_rec, src_rec) if sh == 0 else (coarsen(dst_rec, sh), coarsen(src_rec, sh))
        levels.append(align(d, v, s, T, v, centre=centre, **kw))
        T = levels[-1][0]
    return levels[-1], levels
