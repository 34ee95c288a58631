"""Hand-made maps and rays shared by the ray-cast tests (test_map_raycast_cpu.py, test_gpu_map_raycast.py): one case
per rule of the march, on a map of edge V = 2^-6 m -- exact in float32, so what a case says about cells and entry parameters is
what the march computes.  A voxel sits at the centre of its cell unless a case says otherwise.  Test infrastructure only."""
import numpy as np

import map_carve_cases as cc

F = np.float32
V = 2.0 ** -6
EMPTY = 0xFFFFFFFFFFFFFFFF
HIT, RANGE, OUTSIDE, EXHAUSTED = range(4)
H = 0.5 * V  # a cell's centre offset


def cell(i, j, k, n=1):
    """A row of map_carve_cases.pack: n points at the centre of cell (i, j, k)."""
    return cc._row(((i + 0.5) * V, (j + 0.5) * V, (k + 0.5) * V), n)


def key_of(i, j, k):
    b = 1 << 20
    return ((i + b) << 42) | ((j + b) << 21) | (k + b)


def records(rows):
    return cc.pack(rows, voxel=V)[0] if rows else np.zeros(0, cc.mrr.DTYPE)


def ray(o, s0, d, s1):
    return [o[0], o[1], o[2], s0, d[0], d[1], d[2], s1]


C0 = (H, H, H)  # the centre of cell (0, 0, 0)
ALONG_X = [cell(3, 0, 0)]
NAN, INF = float("nan"), float("inf")


def ray_cases():
    """-> a list of (name, rows, ray, min_count, max_steps, (status, hit cell or None, s, cells)); s None: not stated."""
    c = []
    # a hit in the start cell: s == s0, one cell
    c.append(("start cell", [cell(2, 3, 4)], ray((2.5 * V - 0.25, 3.5 * V, 4.5 * V), 0.25, (1, 0, 0), 1.0), 1, 4096, (HIT, (2, 3, 4), 0.25, 1)))
    # the tie order: from the corner along the diagonal all three crossings tie, and the lowest axis steps first
    diag = ray((0, 0, 0), 0.0, (1, 1, 1), 4 * V)
    c.append(("tie: x first", [cell(1, 0, 0)], diag, 1, 4096, (HIT, (1, 0, 0), V, 2)))
    c.append(("tie: y never", [cell(0, 1, 0)], diag, 1, 4096, (RANGE, None, None, None)))
    c.append(("tie: then y", [cell(1, 1, 0)], diag, 1, 4096, (HIT, (1, 1, 0), V, 3)))
    c.append(("tie: then z", [cell(1, 1, 1)], diag, 1, 4096, (HIT, (1, 1, 1), V, 4)))
    # a zero component on one axis and on two
    c.append(("d_z == 0", [cell(3, 1, 0)], ray(C0, 0.0, (1, 0.5, 0), 1.0), 1, 4096, (HIT, (3, 1, 0), 2.5 * V, 5)))
    c.append(("d_y == d_z == 0", ALONG_X, ray(C0, 0.0, (1, 0, 0), 1.0), 1, 4096, (HIT, (3, 0, 0), 2.5 * V, 4)))
    c.append(("d_z == -0", [cell(3, 1, 0)], ray(C0, 0.0, (1, 0.5, -0.0), 1.0), 1, 4096, (HIT, (3, 1, 0), 2.5 * V, 5)))
    c.append(("d == 0", ALONG_X, ray(C0, 0.0, (0, 0, 0), 1.0), 1, 4096, (RANGE, None, 0.0, 1)))
    c.append(("d == 0 in a voxel", [cell(0, 0, 0)], ray(C0, 0.0, (0, 0, 0), 1.0), 1, 4096, (HIT, (0, 0, 0), 0.0, 1)))
    # 1 / d overflows: the axis does not step (d is subnormal)
    c.append(("1 / d_y not finite", ALONG_X, ray(C0, 0.0, (1, 1e-40, 0), 1.0), 1, 4096, (HIT, (3, 0, 0), 2.5 * V, 4)))
    # a negative direction on each axis
    c.append(("-x", [cell(-3, 0, 0)], ray(C0, 0.0, (-1, 0, 0), 1.0), 1, 4096, (HIT, (-3, 0, 0), 2.5 * V, 4)))
    c.append(("-y", [cell(0, -3, 0)], ray(C0, 0.0, (0, -1, 0), 1.0), 1, 4096, (HIT, (0, -3, 0), 2.5 * V, 4)))
    c.append(("-z", [cell(0, 0, -3)], ray(C0, 0.0, (0, 0, -1), 1.0), 1, 4096, (HIT, (0, 0, -3), 2.5 * V, 4)))
    c.append(("-x -y -z, not normalised", [cell(-2, -2, -2)], ray(C0, 0.0, (-2, -2, -2), 1.0), 1, 4096, (HIT, (-2, -2, -2), 0.75 * V, 7)))
    # the end of the range: sn == s1 is a miss, one float32 step later the cell is examined; a hit one cell before it
    c.append(("sn == s1", ALONG_X, ray(C0, 0.0, (1, 0, 0), 2.5 * V), 1, 4096, (RANGE, None, 1.5 * V, 3)))
    c.append(("sn just below s1", ALONG_X, ray(C0, 0.0, (1, 0, 0), float(np.nextafter(F(2.5 * V), F(1)))), 1, 4096, (HIT, (3, 0, 0), 2.5 * V, 4)))
    c.append(("hit one cell before s1", [cell(2, 0, 0)], ray(C0, 0.0, (1, 0, 0), 2.5 * V), 1, 4096, (HIT, (2, 0, 0), 1.5 * V, 3)))
    # min_count makes the nearer voxel transparent
    two = [cell(1, 0, 0, 1), cell(3, 0, 0, 3)]
    c.append(("min_count 0", two, ray(C0, 0.0, (1, 0, 0), 1.0), 0, 4096, (HIT, (1, 0, 0), 0.5 * V, 2)))
    c.append(("min_count 1", two, ray(C0, 0.0, (1, 0, 0), 1.0), 1, 4096, (HIT, (1, 0, 0), 0.5 * V, 2)))
    c.append(("min_count 2", two, ray(C0, 0.0, (1, 0, 0), 1.0), 2, 4096, (HIT, (3, 0, 0), 2.5 * V, 4)))
    c.append(("min_count 4", two, ray(C0, 0.0, (1, 0, 0), 1.0), 4, 4096, (RANGE, None, None, None)))
    # max_steps
    c.append(("max_steps 1", ALONG_X, ray(C0, 0.0, (1, 0, 0), 1.0), 1, 1, (EXHAUSTED, None, 0.0, 1)))
    c.append(("max_steps 2", ALONG_X, ray(C0, 0.0, (1, 0, 0), 1.0), 1, 2, (EXHAUSTED, None, 0.5 * V, 2)))
    c.append(("max_steps 3", ALONG_X, ray(C0, 0.0, (1, 0, 0), 1.0), 1, 3, (EXHAUSTED, None, 1.5 * V, 3)))
    c.append(("max_steps 4", ALONG_X, ray(C0, 0.0, (1, 0, 0), 1.0), 1, 4, (HIT, (3, 0, 0), 2.5 * V, 4)))
    c.append(("max_steps 1, start cell", [cell(0, 0, 0)], ray(C0, 0.0, (1, 0, 0), 1.0), 1, 1, (HIT, (0, 0, 0), 0.0, 1)))
    # the index range: the last cell is examined, the step out of it is outside; a start beyond it is outside with no cell
    edge = 16384.0  # 2^20 V
    c.append(("leaves the index range", ALONG_X, ray((edge - H, H, H), 0.0, (1, 0, 0), 1.0), 1, 4096, (OUTSIDE, None, 0.0, 1)))
    c.append(("leaves it downwards", ALONG_X, ray((-edge + H, H, H), 0.0, (-1, 0, 0), 1.0), 1, 4096, (OUTSIDE, None, 0.0, 1)))
    c.append(("last cell hit", [cc._row((edge - H, H, H))], ray((edge - 3 * H, H, H), 0.0, (1, 0, 0), 1.0), 1, 4096,
              (HIT, ((1 << 20) - 1, 0, 0), 0.5 * V, 2)))
    c.append(("starts beyond the range", ALONG_X, ray((edge, H, H), 0.0, (1, 0, 0), 1.0), 1, 4096, (OUTSIDE, None, 0.0, 0)))
    c.append(("starts below the range", ALONG_X, ray((-edge - V, H, H), 0.0, (1, 0, 0), 1.0), 1, 4096, (OUTSIDE, None, 0.0, 0)))
    # rays that are not finite, or empty: outside with no cell
    for name, r in (("o NaN", ray((NAN, H, H), 0.0, (1, 0, 0), 1.0)), ("o inf", ray((H, -INF, H), 0.0, (1, 0, 0), 1.0)),
                    ("d NaN", ray(C0, 0.5, (1, NAN, 0), 1.0)), ("d NaN at s0 0", ray(C0, 0.0, (1, NAN, 0), 1.0)),
                    ("d inf", ray(C0, 0.5, (INF, 0, 0), 1.0)), ("d inf at s0 0", ray(C0, 0.0, (INF, 0, 0), 1.0)),
                    ("s0 NaN", ray(C0, NAN, (1, 0, 0), 1.0)), ("s0 -inf", ray(C0, -INF, (1, 0, 0), 1.0)),
                    ("s1 NaN", ray(C0, 0.0, (1, 0, 0), NAN)), ("s1 inf", ray(C0, 0.0, (1, 0, 0), INF)), ("s1 -inf", ray(C0, 0.0, (1, 0, 0), -INF)),
                    ("s0 == s1", ray(C0, 0.5, (1, 0, 0), 0.5)), ("s0 > s1", ray(C0, 0.75, (1, 0, 0), 0.5)),
                    ("s0 d overflows", ray(C0, 3e38, (10, 0, 0), 3.2e38))):
        c.append((name, ALONG_X + [cell(0, 0, 0)], r, 1, 4096, (OUTSIDE, None, 0.0, 0)))
    return c


# The view of the depth-range cases: the 8 x 8 camera at the identity over [4 V, 15.5 V); pixel (4, 4) looks along +z from the
# origin, through the cells (0, 0, k).
VIEW_K = (4.0, 4.0, 4.0, 4.0, 4 * V, 15.5 * V)
VIEW_SIZE = (8, 8)


def view_cases():
    """-> a list of (name, rows, min_count, what pixel (4, 4) shows: the z of the hit voxel's mean, or None for a miss)."""
    on_zmin = cc._row((H, H, 4 * V))        # in cell (0, 0, 4), the first one the ray examines; its mean has z == zmin
    past_zmax = cc._row((H, H, 15.75 * V))  # in cell (0, 0, 15), which the ray enters at 15 V < zmax; z >= zmax
    in_last = cc._row((H, H, 15.25 * V))
    return [("z == zmin is transparent", [on_zmin, cell(0, 0, 6)], 1, 6.5 * V),
            ("z == zmin alone", [on_zmin], 1, None),
            ("just inside zmin", [cc._row((H, H, 4 * V + 2.0 ** -20)), cell(0, 0, 6)], 1, 4 * V + 2.0 ** -20),
            ("z >= zmax is transparent", [past_zmax], 1, None),
            ("z < zmax in the last cell", [in_last], 1, 15.25 * V),
            ("min_count and the range together", [on_zmin, cell(0, 0, 6, 1), cell(0, 0, 9, 2)], 2, 9.5 * V)]


# The one-voxel-thick wall of the cells kx + kz == WALL_C: 26-connected only, so a march that stepped two axes at once would
# pass through it.  Seen by the 64 x 64 camera at the identity over [2 V, 12 V).
WALL_C = 8
WALL_K = (16.0, 16.0, 32.0, 32.0, 2 * V, 12 * V)
WALL_SIZE = (64, 64)


def wall_records():
    return records([cell(kx, ky, WALL_C - kx) for kx in range(-4, 10) for ky in range(-26, 26)])


def wall_reaching_pixels():
    """The pixels whose ray is past the wall before its range ends: x + z = s (1 + dcx) starts below WALL_C V (at s = 2 V it is
    at most 6 V) and exceeds (WALL_C + 2) V, the far side of every wall cell, at some s < 12 V -- 12 (1 + dcx) > 10."""
    xs = [x for x in range(64) if 12.0 * (1.0 + (x - 32.0) / 16.0) > 10.0 + 1e-6]
    return [(x, y) for y in range(64) for x in xs]
