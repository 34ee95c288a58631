"""A numpy float32 restatement of the tracker's per-point terms and their EXACT sums -- the specification of the
tracker's exact-sums mode (revo_ctx_set_exact_sums).

calcErrorAndBuffers (optimizer.cpp:74-191, optimizer.h:156-185) and calculateWarpUpdate + LGS6::update / finish
(optimizer.cpp:192-234, LGSX.h:320-326,392-398) point by point, vectorised over the points: every float operation is a
separate IEEE single operation (numpy float32, no fused multiply-add), v[3] and v[4] are evaluated in double (the `1.0`
literal promotes those two expressions) and rounded to float once.  The sums are the float nearest the exact sum of the
float terms: math.fsum gives the double nearest it, and wherever that double is a float midpoint the exact rational sum
decides.  Test infrastructure only: nothing under revo_amd/ imports it."""
import math
from fractions import Fraction

import numpy as np

f32 = np.float32


def round_exact_f32(terms):
    """The float32 nearest the exact sum of `terms` (a float32 array), ties to even."""
    t = np.asarray(terms, np.float32).astype(np.float64)
    d = math.fsum(t.tolist()) + 0.0  # the double nearest the exact sum (+0.0: an empty / all-zero sum is +0)
    f = f32(d)
    if float(f) == d or not math.isfinite(d):
        return f
    g = np.nextafter(f, f32(math.inf) if d > float(f) else f32(-math.inf))
    m = (float(f) + float(g)) / 2.0  # exact in double: two adjacent floats
    if d != m:
        return f  # rounding to double cannot cross the midpoint m: f is also the float nearest the exact sum
    exact = sum((Fraction(x) for x in t.tolist()), Fraction(0))
    lo, hi = (f, g) if float(f) < float(g) else (g, f)
    mid = Fraction(m)
    if exact < mid:
        return lo
    if exact > mid:
        return hi
    return lo if (int(lo.view(np.uint32)) & 1) == 0 else hi


def point_terms(ref_table, pts, cam, R, T, edge_distance, use_edge_filter, huber):
    """Per good point: the 21 upper-triangle terms (v[a]*v[c])*w, the 6 terms v[a]*(r*w) (b is minus their sum), w*r^2 and
    r^2.  ref_table: the keyframe's [h, w, 4] gradient / DT table, pts: the current frame's [n, 4] 3-D edge list, cam: fx, fy,
    cx, cy, w, h of the level, R (3x3) / T: the pose.  Returns (terms [27, n_good], sw [n_good], su [n_good], n_good, n_bad)."""
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    w, h = int(cam[4]), int(cam[5])
    R = np.asarray(R, np.float32).reshape(3, 3)
    T = np.asarray(T, np.float32).reshape(3)
    p = np.asarray(pts, np.float32)
    p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
    W = [((R[r, 0] * p0 + R[r, 1] * p1) + R[r, 2] * p2) + T[r] for r in range(3)]
    with np.errstate(all="ignore"):
        u = W[0] / W[2] * fx + cx
        v = W[1] / W[2] * fy + cy
        valid = (u > 1) & (v > 1) & (u < f32(w - 2)) & (v < f32(h - 2))
        X, Y, Z, u, v = W[0][valid], W[1][valid], W[2][valid], u[valid], v[valid]
        ix, iy = u.astype(np.int64), v.astype(np.int64)
        dx, dy = u - ix.astype(np.float32), v - iy.astype(np.float32)
        dxdy = dx * dy
        w11, w01, w10, w00 = dxdy, dy - dxdy, dx - dxdy, ((f32(1) - dx) - dy) + dxdy
        tab = np.asarray(ref_table, np.float32)
        b00, b10, b01, b11 = tab[iy, ix], tab[iy, ix + 1], tab[iy + 1, ix], tab[iy + 1, ix + 1]
        res = [((w11 * b11[:, k] + w01 * b01[:, k]) + w10 * b10[:, k]) + w00 * b00[:, k] for k in range(3)]
        r = res[2]
        good = ~((r > f32(edge_distance)) & bool(use_edge_filter))
        X, Y, Z, r = X[good], Y[good], Z[good], r[good]
        gx, gy = fx * res[0][good], fy * res[1][good]
        huber = f32(huber)
        wr = np.where(r <= huber, f32(1), huber / r).astype(np.float32)
        z = f32(1) / Z
        zs = f32(1) / (Z * Z)
        vv = [z * gx,
              z * gy,
              (-X * zs) * gx + (-Y * zs) * gy,
              (((-X * Y) * zs) * gx).astype(np.float64) + (-(1.0 + ((Y * Y) * zs).astype(np.float64))) * gy.astype(np.float64),
              (1.0 + ((X * X) * zs).astype(np.float64)) * gx.astype(np.float64) + (((X * Y) * zs) * gy).astype(np.float64),
              (-Y * z) * gx + (X * z) * gy]
        vv = [x.astype(np.float32) for x in vv]
        terms = []
        for a in range(6):
            for c in range(a, 6):
                terms.append((vv[a] * vv[c]) * wr)
        rw = r * wr
        for a in range(6):
            terms.append(vv[a] * rw)
        r2 = r * r
        sw = r2 * wr
    n_good = int(good.sum())
    return np.array(terms, np.float32).reshape(27, n_good), sw, r2, n_good, len(p) - n_good


def cost_terms(ref_dt, pts, cam, R, T, edge_distance, use_edge_filter):
    """TrackerNew::evalCostFunction's per-point terms (tracker.cpp:371-389) at a pose, one per point of pts: the keyframe's
    distance transform [h, w] read at the FLOOR of the projection (fx*X)/Z + cx, (fy*Y)/Z + cy where that lies in 0 <= u < w,
    0 <= v < h and the edge filter keeps it, else 0."""
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    w, h = int(cam[4]), int(cam[5])
    R = np.asarray(R, np.float32).reshape(3, 3)
    T = np.asarray(T, np.float32).reshape(3)
    p = np.asarray(pts, np.float32)
    W = [((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + T[r] for r in range(3)]
    out = np.zeros(len(p), np.float32)
    with np.errstate(all="ignore"):
        u = (fx * W[0]) / W[2] + cx
        v = (fy * W[1]) / W[2] + cy
        inside = (u >= 0) & (u < f32(w)) & (v >= 0) & (v < f32(h))
        r = np.asarray(ref_dt, np.float32)[np.floor(v[inside]).astype(np.int64), np.floor(u[inside]).astype(np.int64)]
    out[inside] = np.where((r > f32(edge_distance)) & bool(use_edge_filter), f32(0), r)
    return out


def eval_cost(ref_dt, pts, cam, R, T, edge_distance, use_edge_filter):
    """TrackerNew::evalCostFunction (tracker.cpp:357-393) at a pose: cost_terms summed in float64 (exact for these terms
    whatever the order) and rounded to float once."""
    return f32(cost_terms(ref_dt, pts, cam, R, T, edge_distance, use_edge_filter).astype(np.float64).sum())


def exact_eval(ref_table, pts, cam, R, T, edge_distance, use_edge_filter, huber):
    """What revo_optimizer_eval returns in exact-sums mode: (mean error, sum_w, sum_u, good, bad, A [6x6], b [6])."""
    terms, sw, su, good, bad = point_terms(ref_table, pts, cam, R, T, edge_distance, use_edge_filter, huber)
    n = f32(good)
    sums = [round_exact_f32(terms[k]) for k in range(27)]
    A = np.zeros((6, 6), np.float32)
    k = 0
    s_w, s_u = round_exact_f32(sw), round_exact_f32(su)
    with np.errstate(all="ignore"):  # good = 0: 0/0 like the reference (optimizer.cpp:190, LGSX.h:323-325)
        for a in range(6):
            for c in range(a, 6):
                A[a, c] = A[c, a] = sums[k] / n
                k += 1
        b = np.array([-(sums[21 + a]) / n for a in range(6)], np.float32)
        err = f32(s_w / n)
    return err, s_w, s_u, good, bad, A, b
