"""The specification of revo_map_tsdf_raycast (include/revo_hip.h) as a loop: per view, per pixel, per sample, the plain
march with one float32 operation per line of arithmetic.  It knows nothing of blocks or masks and nothing of revo_amd.mapfile.
Test infrastructure only."""
import numpy as np

F = np.float32
CELL = np.dtype([("sum", "<i4"), ("weight", "<u4")])
COLOR = np.dtype([("sum_b", "<u4"), ("sum_g", "<u4"), ("sum_r", "<u4"), ("weight", "<u4")])
STATUS = ("hit", "range", "backface", "exhausted")
HIT, RANGE, BACKFACE, EXHAUSTED = range(4)
INFO_KEYS = ("rays", "hits", "range", "backface", "exhausted", "samples", "uncolored")
MAX_STEPS = 1 << 20


def params(voxel, step=None, min_weight=1, max_steps=4096):
    """(step, min_weight, max_steps) as the call runs with them, or ValueError."""
    st = F(0 if step is None else step)
    if not np.isfinite(st) or st < 0:
        raise ValueError("step")
    if not 0 <= int(max_steps) <= MAX_STEPS:
        raise ValueError("max_steps")
    return (F(voxel) if st == 0 else st), max(1, int(min_weight)), (int(max_steps) or 4096)


def lerp(x0, x1, a):
    return F(x0 + F(a * F(x1 - x0)))


def bilerp(v00, v01, v10, v11, r0, r1):
    return lerp(lerp(v00, v01, r0), lerp(v10, v11, r0), r1)


def field(cell):
    return F(F(cell["sum"]) / F(cell["weight"]))


def interpolate(f, rx, ry, rz):
    """The interpolant and its own gradient in one cube -> (F, (Gx, Gy, Gz)).  f[dx, dy, dz]: the eight fields.  Along z first, then
    y, then x; a gradient component interpolates the four differences along its axis over the other two axes in the same order."""
    Fv = lerp(bilerp(f[0, 0, 0], f[0, 0, 1], f[0, 1, 0], f[0, 1, 1], rz, ry), bilerp(f[1, 0, 0], f[1, 0, 1], f[1, 1, 0], f[1, 1, 1], rz, ry), rx)
    gx = bilerp(F(f[1, 0, 0] - f[0, 0, 0]), F(f[1, 0, 1] - f[0, 0, 1]), F(f[1, 1, 0] - f[0, 1, 0]), F(f[1, 1, 1] - f[0, 1, 1]), rz, ry)
    gy = bilerp(F(f[0, 1, 0] - f[0, 0, 0]), F(f[0, 1, 1] - f[0, 0, 1]), F(f[1, 1, 0] - f[1, 0, 0]), F(f[1, 1, 1] - f[1, 0, 1]), rz, rx)
    gz = bilerp(F(f[0, 0, 1] - f[0, 0, 0]), F(f[0, 1, 1] - f[0, 1, 0]), F(f[1, 0, 1] - f[1, 0, 0]), F(f[1, 1, 1] - f[1, 1, 0]), ry, rx)
    return Fv, (gx, gy, gz)


def sample(cells, lo, voxel, mw, o, d, s):
    """The sample at depth s of the ray o + s d -> None when it is not valid, else (F, (Gx, Gy, Gz), colour cell)."""
    b, r = [], []
    for i in range(3):
        g = F(o[i] + F(s * d[i]))
        u = F(F(g / voxel) - F(F(lo[i]) + F(0.5)))
        if not np.isfinite(u):
            return None
        bi = np.floor(u)
        if not 0 <= bi <= cells.shape[i] - 2:
            return None
        b.append(int(bi))
        r.append(F(u - F(bi)))
    f = {}
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                c = cells[b[0] + dx, b[1] + dy, b[2] + dz]
                if int(c["weight"]) < mw:
                    return None
                f[dx, dy, dz] = field(c)
    Fv, (gx, gy, gz) = interpolate(f, *r)
    return Fv, (gx, gy, gz), tuple(b[i] + (1 if r[i] >= F(0.5) else 0) for i in range(3))


def channel_byte(s0, w0, s1, w1, a):
    if w0 > 0 and w1 > 0:
        v = lerp(F(F(s0) / F(w0)), F(F(s1) / F(w1)), a)
    elif w0 > 0:
        v = F(F(s0) / F(w0))
    elif w1 > 0:
        v = F(F(s1) / F(w1))
    else:
        v = F(0)
    return int(np.rint(min(max(v, F(0)), F(255))))


def march(cells, color, lo, voxel, mw, step, max_steps, o, d, zmin, zmax):
    """One ray -> (status, samples, depth, normal, bgr, k)."""
    miss = (F(0), (F(0), F(0), F(0)), (0, 0, 0), 0)
    prev = None  # no previous sample
    k = 0
    while True:
        if k == max_steps:
            return (EXHAUSTED, k) + miss
        s = F(zmin + F(F(k) * step))
        if not s < zmax:
            return (RANGE, k) + miss
        cur = sample(cells, lo, voxel, mw, o, d, s)
        if cur is not None and prev is not None:
            (Fp, Gp, Cp, sp), (Fc, Gc, Cc) = prev, cur
            if Fp < 0 and Fc >= 0:
                return (BACKFACE, k + 1) + miss
            if Fp >= 0 and Fc < 0:
                a = F(Fp / F(Fp - Fc))
                depth = F(sp + F(a * step))
                g = [lerp(Gp[i], Gc[i], a) for i in range(3)]
                l2 = F(F(F(g[0] * g[0]) + F(g[1] * g[1])) + F(g[2] * g[2]))
                nrm = tuple(F(x / np.sqrt(l2)) for x in g) if np.isfinite(l2) and l2 > 0 else (F(0), F(0), F(0))
                bgr, kc = (0, 0, 0), 0
                if color is not None:
                    c0, c1 = color[Cp], color[Cc]
                    w0, w1 = int(c0["weight"]), int(c1["weight"])
                    bgr = tuple(channel_byte(int(c0[n]), w0, int(c1[n]), w1, a) for n in ("sum_b", "sum_g", "sum_r"))
                    kc = (w0 > 0) + (w1 > 0)
                return HIT, k + 1, depth, nrm, bgr, kc
        prev = None if cur is None else cur + (s,)
        k += 1


def raycast(cells, color, lo, voxel, views, step=None, min_weight=1, max_steps=4096):
    """views: (T_w_c 4x4, (fx, fy, cx, cy, zmin, zmax), (w, h)).  -> dict of per-view lists depth, normals, bgr (None without a
    colour volume), hits, status, samples, colored, and info."""
    step, mw, ms = params(voxel, step, min_weight, max_steps)
    voxel = F(voxel)
    out = {k: [] for k in ("depth", "normals", "bgr", "hits", "status", "samples", "colored")}
    info = dict.fromkeys(INFO_KEYS, 0)
    with np.errstate(all="ignore"):
        for T, k, (w, h) in views:
            T = np.asarray(T, F)
            fx, fy, cx, cy, zmin, zmax = (F(x) for x in k)
            R, o = T[:3, :3], T[:3, 3]
            depth, nrm, bgr = np.zeros((h, w), F), np.zeros((h, w, 3), F), np.zeros((h, w, 3), np.uint8)
            status, samples, colored = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
            for y in range(h):
                for x in range(w):
                    dcx = F(F(F(x) - cx) / fx)
                    dcy = F(F(F(y) - cy) / fy)
                    d = [F(F(F(R[i, 0] * dcx) + F(R[i, 1] * dcy)) + R[i, 2]) for i in range(3)]
                    status[y, x], samples[y, x], depth[y, x], nrm[y, x], bgr[y, x], colored[y, x] = \
                        march(cells, color, lo, voxel, mw, step, ms, o, d, zmin, zmax)
            out["depth"].append(depth)
            out["normals"].append(nrm)
            out["bgr"].append(bgr if color is not None else None)
            out["hits"].append(int((status == HIT).sum()))
            out["status"].append(status)
            out["samples"].append(samples)
            out["colored"].append(colored)
            info["rays"] += w * h
            for i, name in enumerate(("hits", "range", "backface", "exhausted")):
                info[name] += int((status == i).sum())
            info["samples"] += int(samples.sum())
            info["uncolored"] += int(((status == HIT) & (colored == 0)).sum()) if color is not None else 0
    out["info"] = info
    return out
