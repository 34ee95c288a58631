"""Hand-made maps and boxes shared by the distance-field tests (test_map_field_cpu.py, test_gpu_map_field.py), on a map
of edge V = 2^-6 m so that cells are exact: one case per rule of the contract and per path of the kernels.  Test infrastructure
only."""
import numpy as np

import map_raycast_cases as rc

V = rc.V
LO_RIM, HI_RIM = -(1 << 20), (1 << 20) - 1


def records(cells):
    """Records of (i, j, k) or (i, j, k, count) voxel indices."""
    return rc.records([rc.cell(*c) for c in cells])


def case(name, cells, lo, n, min_count=1, clamp=0):
    return {"name": name, "cells": [tuple(c) for c in cells], "lo": tuple(lo), "n": tuple(n), "min_count": min_count, "clamp": clamp}


def _abs(lo, rel):
    return tuple(int(a) + int(b) for a, b in zip(lo, rel))


# the long-line boxes: voxels at cells 5 and 1000 of the long axis, on different cells of the first short axis, none in its
# last plane.  For 1024 x 3 x 2 the farthest cell is (502, 2, 1): 497^2 + 2^2 + 1^2 from the voxel at (5, 0, 0).
LONG_MAX_FIRST = 497 * 497 + 4 + 1
assert LONG_MAX_FIRST == 247014


def long_cases():
    out = []
    for axis, n in ((0, (1024, 3, 2)), (1, (3, 1024, 2)), (2, (3, 2, 1024))):
        short = [a for a in range(3) if a != axis]
        lo = (-500, 7, -37)
        cells = []
        for along, s0 in ((5, 0), (1000, 1)):
            rel = [0, 0, 0]
            rel[axis], rel[short[0]] = along, s0
            cells.append(_abs(lo, rel))
        out.append(case("long axis %d: %d x %d x %d" % ((axis,) + n), cells, lo, n))
    return out


def random_case(seed=5, n=(70, 45, 37), voxels=200, lo=(-31, 5, -37), counts=False):
    rng = np.random.default_rng(seed)
    flat = rng.choice(n[0] * n[1] * n[2], voxels, replace=False)
    rel = np.stack(np.unravel_index(flat, n), -1)
    cells = [_abs(lo, r) + ((int(rng.integers(1, 4)),) if counts else ()) for r in rel]
    return case("random %d x %d x %d, %d voxels" % (n + (voxels,)), cells, lo, n)


def cases():
    c = []
    lo, n = (-2, 3, -1), (5, 4, 3)
    for ix in (0, 4):
        for iy in (0, 3):
            for iz in (0, 2):
                c.append(case("corner %d %d %d of 5 x 4 x 3" % (ix, iy, iz), [_abs(lo, (ix, iy, iz))], lo, n))
    c.append(case("the centre of 5 x 4 x 3", [_abs(lo, (2, 2, 1))], lo, n))
    c.append(case("1 x 1 x 1, solid", [(7, -3, 2)], (7, -3, 2), (1, 1, 1)))
    c.append(case("1 x 1 x 1, empty", [(8, -3, 2)], (7, -3, 2), (1, 1, 1)))
    some = [(0, 0, 0), (3, 4, 4), (1, 2, 3), (3, 0, 2)]
    for axis in range(3):
        n1 = [4, 5, 6]
        n1[axis] = 1
        cells = [tuple(0 if a == axis else v for a, v in enumerate(p)) for p in some]
        c.append(case("size 1 on axis %d" % axis, sorted(set(cells)), (0, 0, 0), n1))
    c.append(case("an empty map", [], (-3, -3, -3), (6, 5, 4)))
    c.append(case("every voxel outside the box", [(-4, 0, 0), (3, 0, 0), (0, 2, 0), (0, -1, -4), (0, 0, 1), (100, 100, 100)], (-3, 0, -3), (6, 2, 4)))
    for nz in (31, 32, 33, 65):
        bits = sorted(set(b for b in (0, 31, 32, 63, 64, nz - 1) if b < nz))
        cells = [(i % 2, (i // 2) % 3, -37 + b) for i, b in enumerate(bits)]
        c.append(case("nz %d from z = -37, first and last bits of the words" % nz, cells, (0, 0, -37), (2, 3, nz)))
    c.append(case("nz 65, one voxel in the last word", [(1, 1, 27)], (0, 0, -37), (2, 3, 65)))
    c.append(case("equidistant voxels", [(0, 2, 2), (4, 2, 2), (2, 0, 2), (2, 4, 2), (2, 2, 0), (2, 2, 4)], (0, 0, 0), (5, 5, 5)))
    for axis in range(3):
        for gap in (1, 2):
            b = [3, 3, 3]
            b2 = list(b)
            b2[axis] += gap
            c.append(case("two voxels %d apart on axis %d" % (gap, axis), [tuple(b), tuple(b2)], (0, 0, 0), (8, 7, 9)))
    counted = [(1, 1, 1, 1), (6, 2, 3, 2), (3, 5, 7, 3), (20, 0, 0, 3), (21, 0, 0, 1)]  # the last two lie outside the box
    for mc in (0, 1, 2, 3, 4):
        c.append(case("min_count %d on counts 1, 2, 3" % mc, counted, (0, 0, 0), (8, 7, 9), min_count=mc))
    for clamp in (0, 1, 2, 50, 1000):
        c.append(case("clamp %d" % clamp, [(1, 1, 1), (6, 5, 7)], (0, 0, 0), (8, 7, 9), clamp=clamp))
    c.append(case("the box touches -2^20", [(LO_RIM, LO_RIM, LO_RIM), (LO_RIM + 2, LO_RIM + 1, LO_RIM + 4)], (LO_RIM,) * 3, (4, 3, 5)))
    c.append(case("the box touches 2^20 - 1", [(HI_RIM, HI_RIM, HI_RIM), (HI_RIM - 3, HI_RIM - 1, HI_RIM - 2)], (HI_RIM - 3, HI_RIM - 2, HI_RIM - 4), (4, 3, 5)))
    c += long_cases()
    c.append(random_case())
    return c
