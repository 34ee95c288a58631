"""numpy specification of the point-to-plane registration of voxel maps (include/revo_hip.h revo_map_normals /
revo_map_align_plane_eval / revo_map_align_plane_system / revo_map_align_plane), bit for bit where the contract is
bit for bit.  It builds on map_align_ref (points, orthogonality, the Cholesky solve, coarsening) and voxel_map_ref.

Every float32 operation below is one numpy float32 operation (no fused multiply-add), in the order the header states; the host
loop's double arithmetic is written out in revo_align_host.h's order, so its poses are the library's bit for bit.
Test infrastructure only: nothing under revo_amd/ imports it."""
import ctypes as C
import math

import numpy as np

import exact_sums_ref as xr
import map_align_ref as mar
import voxel_map_ref as ref

F = np.float32
CONVERGED, ITER_LIMIT, LOST = mar.CONVERGED, mar.ITER_LIMIT, mar.LOST
NORMALS_DEFAULT = dict(min_neighbours=5, planarity=0.1, min_spread=0.1)
OFFSETS = [(ox, oy, oz) for ox in (-1, 0, 1) for oy in (-1, 0, 1) for oz in (-1, 0, 1)]  # x outermost, z innermost
NO_KEY = np.uint64(0xffffffffffffffff)


class PlaneInfo(C.Structure):
    """revo_map_plane_info, field by field (written without revo_amd.settings, which is checked against it)."""
    _fields_ = [("S", C.c_float * 28), ("matched", C.c_uint64), ("considered", C.c_uint64), ("skipped", C.c_uint64),
                ("centre", C.c_float * 3), ("max_dist", C.c_float), ("R", C.c_float * 9), ("T", C.c_float * 3),
                ("flags", C.c_int32), ("dst_normals", C.c_int32)]


assert C.sizeof(PlaneInfo) == 208


def _lookup(keys, k, off):
    """The voxels at index k + off among the ascending `keys`: (hit mask, their positions, their packed keys)."""
    kk = k + np.array(off, np.int64)
    inr = np.all((kk >= ref.KEY_MIN) & (kk <= ref.KEY_MAX), 1)
    key = ref.pack_keys(np.where(inr[:, None], kk, 0))
    j = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
    return inr & (keys[j] == key), j, key


def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """One Jacobi rotation of the pair (p, q), r the third index, where a_pq != 0; vp, vq: the two columns of V (N x 3)."""
    go = apq != 0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (F(2) * apq)
        t = np.copysign(F(1), theta) / (np.abs(theta) + np.sqrt(theta * theta + F(1)))
        c = F(1) / np.sqrt(t * t + F(1))
        s = t * c
        h = t * apq
        new = (app - h, aqq + h, np.zeros_like(apq), c * arp - s * arq, s * arp + c * arq,
               c[:, None] * vp - s[:, None] * vq, s[:, None] * vp + c[:, None] * vq)
    old = (app, aqq, apq, arp, arq, vp, vq)
    return tuple(np.where(go if o.ndim == 1 else go[:, None], n, o).astype(F) for n, o in zip(new, old))


def normals(rec, min_count=1, min_neighbours=5, planarity=0.1, min_spread=0.1):
    """revo_map_normals -> (keys, xyz [N, 3], normal [N, 3], lambda [N, 3], neighbours [N] uint32, valid [N] bool), in
    ascending key order: the voxels of revo_map_extract(min_count)."""
    keys, m = mar.points_of(rec, min_count)
    n = len(keys)
    if n == 0:
        return keys, m, np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, np.uint32), np.zeros(0, bool)
    k = mar.unpack_keys(keys)
    s1 = [np.zeros(n, F) for _ in range(3)]
    s2 = [np.zeros(n, F) for _ in range(6)]  # xx xy xz yy yz zz
    nb = np.zeros(n, np.uint32)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    for off in OFFSETS:
        hit, j, _ = _lookup(keys, k, off)
        d = (m[j] - m).astype(F)
        for i in range(3):
            s1[i] = np.where(hit, s1[i] + d[:, i], s1[i]).astype(F)
        for e, (a, b) in enumerate(pairs):
            s2[e] = np.where(hit, s2[e] + d[:, a] * d[:, b], s2[e]).astype(F)
        nb += hit
    fn = nb.astype(F)
    with np.errstate(all="ignore"):
        a00, a01, a02, a11, a12, a22 = [(s2[e] - (s1[a] * s1[b]) / fn).astype(F) for e, (a, b) in enumerate(pairs)]
    v0, v1, v2 = [np.tile(np.eye(3, dtype=F)[:, i], (n, 1)) for i in range(3)]  # the columns of V
    for _ in range(6):
        a00, a11, a01, a02, a12, v0, v1 = _rotate(a00, a11, a01, a02, a12, v0, v1)  # (0, 1), r = 2
        a00, a22, a02, a01, a12, v0, v2 = _rotate(a00, a22, a02, a01, a12, v0, v2)  # (0, 2), r = 1
        a11, a22, a12, a01, a02, v1, v2 = _rotate(a11, a22, a12, a01, a02, v1, v2)  # (1, 2), r = 0
    # sorted with ties to the lower index, the column of the smallest carried along
    l0, l1, l2, nv = a00, a11, a22, v0
    sw = l1 < l0
    l0, l1, nv = np.where(sw, l1, l0), np.where(sw, l0, l1), np.where(sw[:, None], v1, nv)
    front = l2 < l0
    mid = ~front & (l2 < l1)
    l0, l1, l2, nv = (np.where(front, l2, l0), np.where(front, l0, np.where(mid, l2, l1)), np.where(front | mid, l1, l2),
                      np.where(front[:, None], v2, nv))
    with np.errstate(all="ignore"):
        norm = np.sqrt((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2])
        nv = (nv / norm[:, None]).astype(F)
        ax, ay, az = np.abs(nv[:, 0]), np.abs(nv[:, 1]), np.abs(nv[:, 2])
        big = np.where((ax >= ay) & (ax >= az), nv[:, 0], np.where(ay >= az, nv[:, 1], nv[:, 2]))
        nv = np.where((big < 0)[:, None], -nv, nv).astype(F)
        valid = ((nb >= min_neighbours) & np.all(np.isfinite(nv), 1) & (l1 > 0) & (l0 <= F(planarity) * l1) & (l1 >= F(min_spread) * l2))
    nv = np.where(valid[:, None], nv, F(0)).astype(F)
    return keys, m, nv, np.stack([l0, l1, l2], 1).astype(F), nb, valid


class Target:
    """The destination's caches of one point-to-plane call: the candidates (count and a valid normal) with point and normal."""

    def __init__(self, dst_rec, dst_voxel, min_count_dst=1, **nprm):
        p = dict(NORMALS_DEFAULT, **nprm)
        keys, q, nv, _, _, valid = normals(dst_rec, max(1, int(min_count_dst)), **p)
        self.voxel = F(dst_voxel)
        self.keys, self.q, self.n = keys[valid], q[valid], nv[valid]
        self.dst_normals = int(valid.sum())


def matches(tgt, src_rec, T, max_dist, min_count_src=1):
    """map_align_ref.matches with the candidates of a Target -> (p' [M, 3], q [M, 3], normal [M, 3], considered, skipped)."""
    T = np.asarray(T, F)
    _, p = mar.points_of(src_rec, min_count_src)
    with np.errstate(all="ignore"):
        pt = np.stack([((T[i, 0] * p[:, 0] + T[i, 1] * p[:, 1]) + T[i, 2] * p[:, 2]) + T[i, 3] for i in range(3)], 1).astype(F).reshape(-1, 3)
        f = np.floor(pt / tgt.voxel)
        ok = np.all(np.abs(pt) < F(ref.RANGE_M), 1) & np.all((f >= ref.KEY_MIN) & (f <= ref.KEY_MAX), 1)
    considered, skipped = len(p), int((~ok).sum())
    pt, k = pt[ok], f[ok].astype(np.int64)
    n = len(pt)
    best_d2 = np.full(n, np.inf, F)
    best_key = np.full(n, NO_KEY)
    best_j = np.zeros(n, np.int64)
    if len(tgt.keys) and n:
        for off in OFFSETS:
            hit, j, key = _lookup(tgt.keys, k, off)
            d = pt - tgt.q[j]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            better = hit & ((d2 < best_d2) | ((d2 == best_d2) & (key < best_key)))
            best_d2 = np.where(better, d2, best_d2)
            best_key = np.where(better, key, best_key)
            best_j = np.where(better, j, best_j)
    acc = (best_key != NO_KEY) & (best_d2 <= F(max_dist) * F(max_dist))
    if not len(tgt.keys):
        return pt[:0], pt[:0], pt[:0], considered, skipped
    return pt[acc], tgt.q[best_j[acc]], tgt.n[best_j[acc]], considered, skipped


def plane_terms(u, r, nv):
    """The 28 float term arrays of the accepted matches: J_i J_j (i <= j, row by row), J_i e, e e."""
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    nx, ny, nz = nv[:, 0], nv[:, 1], nv[:, 2]
    e = (nx * r[:, 0] + ny * r[:, 1]) + nz * r[:, 2]
    J = [nx, ny, nz, uy * nz - uz * ny, uz * nx - ux * nz, ux * ny - uy * nx]
    return [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * e for i in range(6)] + [e * e]


def align_plane_eval(tgt, src_rec, T, max_dist, min_count_src=1, centre=(0, 0, 0)):
    """The record revo_map_align_plane_eval writes for one pose (a PlaneInfo)."""
    T = np.asarray(T, F)
    out = PlaneInfo()
    c = np.asarray(centre, F).reshape(3)
    out.centre[:] = c.tolist()
    out.max_dist = F(max_dist)
    # a NaN pose keeps its bits: R (column-major, as given) and T bytewise
    C.memmove(C.addressof(out) + PlaneInfo.R.offset, np.ascontiguousarray(T[:3, :3].T).tobytes(), 36)
    C.memmove(C.addressof(out) + PlaneInfo.T.offset, np.ascontiguousarray(T[:3, 3]).tobytes(), 12)
    if not np.all(np.isfinite(T[:3, :4])) or not mar.is_orthogonal(T[:3, :3]):
        out.flags = 1
        return out
    pt, q, nv, considered, skipped = matches(tgt, src_rec, T, max_dist, min_count_src)
    for i, t in enumerate(plane_terms(pt - c, pt - q, nv)):
        out.S[i] = xr.round_exact_f32(np.asarray(t, F))
    out.matched, out.considered, out.skipped = len(pt), considered, skipped
    out.dst_normals = min(tgt.dst_normals, 0x7fffffff)
    return out


def system(info):
    """revo_map_align_plane_system: (H [6, 6], g [6]) float64, H from its upper triangle S[0..20], g = S[21..26]."""
    S = np.array(list(info.S), np.float64)
    H = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = S[k]
            k += 1
    return H, S[21:27].copy()


def _mul4(A, B):
    """mat4_mul of revo_align_host.h: every entry summed over k in index order from 0.0."""
    out = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            v = 0.0
            for k in range(4):
                v += A[i][k] * B[k][j]
            out[i][j] = v
    return out


def se3_exp(x):
    """se3_exp_d of revo_align_host.h, operation for operation -> 4 x 4 nested lists of Python floats."""
    v, w = [float(a) for a in x[:3]], [float(a) for a in x[3:]]
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    W = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    W2 = [W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j] for i in range(3) for j in range(3)]
    a, b, c, d = 1.0, 0.0, 0.5, 0.0
    if not th < 1e-10:
        a, b = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th)
        c, d = b, (th - math.sin(th)) / (th * th * th)
    E = [[0.0] * 4 for _ in range(4)]
    E[3][3] = 1.0
    for i in range(3):
        t = 0.0
        for j in range(3):
            eye = 1.0 if i == j else 0.0
            E[i][j] = eye + a * W[3 * i + j] + b * W2[3 * i + j]
            t += (eye + c * W[3 * i + j] + d * W2[3 * i + j]) * v[j]
        E[i][3] = t
    return E


def gauss_newton(evaluate, system_of, T_init, centre, max_iters=30, eps_t=1e-6, eps_r=1e-6, min_matched=12):
    """align_loop_over of revo_align_host.h over evaluate(T float32 4x4) -> record: (T_out, record at T_out, iterations, status)."""
    c = [float(a) for a in np.asarray(centre, F)]
    Cp = [[1.0, 0.0, 0.0, c[0]], [0.0, 1.0, 0.0, c[1]], [0.0, 0.0, 1.0, c[2]], [0.0, 0.0, 0.0, 1.0]]
    Cm = [[1.0, 0.0, 0.0, -c[0]], [0.0, 1.0, 0.0, -c[1]], [0.0, 0.0, 1.0, -c[2]], [0.0, 0.0, 0.0, 1.0]]
    T = [[float(a) for a in row] for row in np.asarray(T_init, F)]
    Tsys = T
    status, it = ITER_LIMIT, 0
    while it < max_iters:
        rec = evaluate(np.array(T, np.float64).astype(F))
        x = None
        if not (rec.flags & 1) and rec.matched >= min_matched:
            x = mar.solve(*system_of(rec))
        if x is None:
            status, T = LOST, Tsys
            break
        it += 1
        Tsys = T
        T = _mul4(_mul4(_mul4(Cp, se3_exp(x)), Cm), T)
        if np.max(np.abs(x[:3])) < eps_t and np.max(np.abs(x[3:])) < eps_r:
            status = CONVERGED
            break
    Tf = np.array(T, np.float64).astype(F)
    return Tf, evaluate(Tf), it, status


def align_plane(dst_rec, dst_voxel, src_rec, T_init, max_dist, min_count_dst=1, min_count_src=1, centre=(0, 0, 0), max_iters=30,
                eps_t=1e-6, eps_r=1e-6, min_matched=12, **nprm):
    """revo_map_align_plane's loop -> (T_out 4x4 float32, PlaneInfo at T_out, iterations, status)."""
    tgt = dst_rec if isinstance(dst_rec, Target) else Target(dst_rec, dst_voxel, min_count_dst, **nprm)
    return gauss_newton(lambda T: align_plane_eval(tgt, src_rec, T, max_dist, min_count_src, centre), system, T_init, centre,
                        max_iters, eps_t, eps_r, min_matched)


def align_point(dst_rec, dst_voxel, src_rec, T_init, max_dist, min_count_dst=1, min_count_src=1, centre=(0, 0, 0), max_iters=30,
                eps_t=1e-6, eps_r=1e-6, min_matched=12):
    """map_align_ref.align's loop (point-to-point records) with the host arithmetic written out as above: the baseline."""
    return gauss_newton(lambda T: mar.align_eval(dst_rec, dst_voxel, src_rec, T, max_dist, min_count_dst, min_count_src, centre),
                        mar.system, T_init, centre, max_iters, eps_t, eps_r, min_matched)


def align_maps(dst_rec, src_rec, voxel, T_init=None, shifts=(2, 1, 0), centre=None, metric="plane", **kw):
    """api.align_maps(metric=...): coarsen both maps per level, align with max_dist = that level's edge, hand the pose down.
    -> (T, record, iterations, status) of the last level and the list of every level's."""
    T = np.eye(4, dtype=F) if T_init is None else np.asarray(T_init, F)
    if centre is None:
        centre = mar.default_centre(src_rec, T, kw.get("min_count_src", 1))
    one = align_plane if metric == "plane" else align_point
    levels = []
    for sh in shifts:
        v = F(np.ldexp(F(voxel), sh))
        d, s = (dst_rec, src_rec) if sh == 0 else (mar.coarsen(dst_rec, sh), mar.coarsen(src_rec, sh))
        levels.append(one(d, v, s, T, v, centre=centre, **kw))
        T = levels[-1][0]
    return levels[-1], levels
