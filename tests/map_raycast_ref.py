"""The ray march of revo_map_raycast / revo_map_cast_rays (include/revo_hip.h) restated operation for operation as a
per-ray Python loop.  All arithmetic is float32 (numpy float32 scalars), every operation rounded on its own.

A ray is o[3], s0, d[3], s1: the points o + s d for s0 <= s < s1.
  1. g_i = o_i + s0 d_i, f_i = floor(g_i / voxel); OUTSIDE with 0 cells unless s0 < s1, s1 finite, every g_i finite and
     -2^20 <= f_i <= 2^20 - 1; k_i = int(f_i)
  2. inv_i = 1 / d_i; d_i > 0: step +1, pos 1; d_i < 0: step -1, pos 0; d_i zero or NaN, or inv_i not finite: step 0, t_i = +inf;
     else t_i = (float(k_i + pos_i) voxel - o_i) inv_i
  3. s = s0, cells = 0; loop: cells == max_steps -> EXHAUSTED; cells += 1; cell k solid -> HIT at entry parameter s;
     a = 0, if t_1 < t_a: a = 1, if t_2 < t_a: a = 2; sn = t_a; not sn < s1 -> RANGE; k_a += step_a, out of the index range ->
     OUTSIDE; s = sn; t_a = (float(k_a + pos_a) voxel - o_a) inv_a
Solid: a voxel with count >= max(min_count, 1) -- and, for the rays of a view, whose point (as revo_map_extract forms it),
taken to the camera as revo_map_render does, is finite with zmin < z < zmax.  Test infrastructure only."""
import numpy as np

import map_render_ref as mr
import voxel_map_ref as ref

F = np.float32
HIT, RANGE, OUTSIDE, EXHAUSTED = range(4)
STATUS = ("hit", "range", "outside", "exhausted")
INFO_KEYS = ("rays", "hits", "range", "outside", "exhausted", "cells")
EMPTY = 0xFFFFFFFFFFFFFFFF
LO, HI = -(1 << 20), (1 << 20) - 1
INF = F(np.inf)


def pack_key(k):
    return ((k[0] + (1 << 20)) << 42) | ((k[1] + (1 << 20)) << 21) | (k[2] + (1 << 20))


def march(o, s0, d, s1, voxel, solid, max_steps):
    """One ray.  solid: a container of packed keys (ints).  -> (status, key, s, cells)."""
    o, d, s0, s1, voxel = [F(x) for x in o], [F(x) for x in d], F(s0), F(s1), F(voxel)
    with np.errstate(all="ignore"):
        g = [o[i] + s0 * d[i] for i in range(3)]
        f = [np.floor(g[i] / voxel) for i in range(3)]
        if not (s0 < s1) or not np.isfinite(s1) or not all(np.isfinite(x) for x in g) or not all(F(LO) <= x <= F(HI) for x in f):
            return OUTSIDE, EMPTY, F(0), 0
        k = [int(x) for x in f]
        step, pos, inv, t = [0, 0, 0], [0, 0, 0], [F(0)] * 3, [INF] * 3
        for i in range(3):
            inv[i] = F(1) / d[i]
            if d[i] > 0:
                step[i], pos[i] = 1, 1
            elif d[i] < 0:
                step[i], pos[i] = -1, 0
            if step[i] == 0 or not np.isfinite(inv[i]):
                step[i], t[i] = 0, INF
            else:
                t[i] = (F(k[i] + pos[i]) * voxel - o[i]) * inv[i]
        s, s_seen, cells = s0, F(0), 0  # s_seen: the entry parameter of the last cell examined
        while True:
            if cells == max_steps:
                return EXHAUSTED, EMPTY, s_seen, cells
            cells += 1
            s_seen = s
            key = pack_key(k)
            if key in solid:
                return HIT, key, s, cells
            a = 0
            if t[1] < t[a]:
                a = 1
            if t[2] < t[a]:
                a = 2
            sn = t[a]
            if not (sn < s1):
                return RANGE, EMPTY, s, cells
            k[a] += step[a]
            if k[a] < LO or k[a] > HI:
                return OUTSIDE, EMPTY, s, cells
            s = sn
            t[a] = (F(k[a] + pos[a]) * voxel - o[a]) * inv[a]


def info_of(status, cells):
    status = np.asarray(status)
    return {"rays": int(status.size), "hits": int((status == HIT).sum()), "range": int((status == RANGE).sum()),
            "outside": int((status == OUTSIDE).sum()), "exhausted": int((status == EXHAUSTED).sum()), "cells": int(np.sum(cells))}


def cast_rays(records, voxel, rays, min_count=1, max_steps=4096):
    """-> (key uint64 [N], s float32 [N], cells uint32 [N], status uint8 [N], info) of [N, 8] rays o, s0, d, s1."""
    rec = records[records["count"] >= max(1, int(min_count))]
    solid = set(int(x) for x in rec["key"])
    rays = np.asarray(rays, F).reshape(-1, 8)
    out = [march(r[0:3], r[3], r[4:7], r[7], voxel, solid, max_steps) for r in rays]
    status = np.array([x[0] for x in out], np.uint8)
    cells = np.array([x[3] for x in out], np.uint32)
    return (np.array([x[1] for x in out], np.uint64), np.array([x[2] for x in out], F), cells, status, info_of(status, cells))


def solid_of(records, view, min_count=1):
    """{key: (z, (b, g, r))} of the voxels solid to the view (a map_render_ref.View): the loop form of the view's predicate."""
    rec = records[records["count"] >= max(1, int(min_count))]
    Rc, tc = mr.world_to_camera(view.T)
    p = ref.mean_position(rec["sum_q"], rec["count"].astype(np.int64)).reshape(-1, 3).astype(F)
    out = {}
    with np.errstate(all="ignore"):
        for r, q in zip(rec, p):
            pc = [((Rc[i, 0] * q[0] + Rc[i, 1] * q[1]) + Rc[i, 2] * q[2]) + tc[i] for i in range(3)]
            if all(np.isfinite(x) for x in pc) and pc[2] > view.zmin and pc[2] < view.zmax:
                n = int(r["count"])
                out[int(r["key"])] = (pc[2], tuple((int(c) + n // 2) // n for c in r["sum_bgr"]))
    return out


def pixel_ray(view, x, y):
    """(o, s0, d, s1) of pixel (x, y) of a map_render_ref.View."""
    T = view.T
    with np.errstate(all="ignore"):
        dcx = (F(x) - view.cx) / view.fx
        dcy = (F(y) - view.cy) / view.fy
        d = [((T[i, 0] * dcx) + (T[i, 1] * dcy)) + T[i, 2] for i in range(3)]
    return [T[i, 3] for i in range(3)], view.zmin, d, view.zmax


def raycast(records, voxel, view, min_count=1, max_steps=4096, pixels=None):
    """The view's pixels (all of them in row order, or the given (x, y) list) -> dict of depth float32, bgr uint8 [n, 3],
    key uint64, s float32, cells int64, status int64, [n] each, and info over those pixels."""
    solid = solid_of(records, view, min_count)
    if pixels is None:
        pixels = [(x, y) for y in range(view.height) for x in range(view.width)]
    n = len(pixels)
    out = {"depth": np.zeros(n, F), "bgr": np.zeros((n, 3), np.uint8), "key": np.full(n, EMPTY, np.uint64), "s": np.zeros(n, F),
           "cells": np.zeros(n, np.int64), "status": np.zeros(n, np.int64)}
    for i, (x, y) in enumerate(pixels):
        st, key, s, cells = march(*pixel_ray(view, x, y), voxel, solid, max_steps)
        out["status"][i], out["key"][i], out["s"][i], out["cells"][i] = st, key, s, cells
        if st == HIT:
            out["depth"][i], out["bgr"][i] = solid[key]
    out["info"] = info_of(out["status"], out["cells"])
    return out
