"""Hand-made fields, seeds and starts shared by the planning tests (test_map_plan_cpu.py, test_gpu_map_plan.py): one
case per rule of the contract and per path of the kernels -- tile rims and partial tiles (the tile edge is 8 cells), the moves
across tile faces, edges and corners, and runs of many rounds.  A case is a field d2 (0: solid, NONE: nothing near), the box's
lo, r2 and seeds (x, y, z, cost0 as absolute voxel indices).  Test infrastructure only."""
import functools

import numpy as np

NONE = np.uint32(0xFFFFFFFF)
LO = (-5, 3, -11)  # every box but the named ones starts below zero on two axes


def case(name, d2, seeds, r2=1, lo=LO):
    d2 = np.ascontiguousarray(d2, np.uint32)
    return {"name": name, "d2": d2, "lo": tuple(lo), "n": d2.shape, "r2": int(r2),
            "seeds": [tuple(int(a) + int(b) for a, b in zip(s[:3], lo)) + (int(s[3]) if len(s) > 3 else 0,) for s in seeds]}


def open_box(n):
    return np.full(n, NONE, np.uint32)


def corners(n):
    """A seed at every corner of the box, each with its own cost0."""
    out = []
    for i, c in enumerate(np.ndindex(2, 2, 2)):
        out.append(tuple((n[k] - 1) * c[k] for k in range(3)) + (5 * i,))
    return out


def random_field(n, blocked, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < blocked, np.uint32(0), NONE).astype(np.uint32)


def free_cells(d2, r2, k, seed):
    """k free cells of the field (relative), chosen at random."""
    rng = np.random.default_rng(seed)
    c = np.argwhere(d2 >= np.uint32(r2))
    return [tuple(int(v) for v in c[i]) for i in rng.choice(len(c), min(k, len(c)), replace=False)]


def random_case(seed=1, n=(33, 20, 11), blocked=0.35):
    d2 = random_field(n, blocked, seed)
    return case("random %d x %d x %d, %d %% blocked, seed %d" % (n + (round(100 * blocked), seed)), d2, free_cells(d2, 1, 1, seed))


def serpentine():
    """40 x 40 x 8: walls across y and z at x = 4, 8, .., 36, each with a gap of two cells at alternating ends of y; the seed
    in the first corridor's far corner.  The corridors are 3 cells wide -- narrower than a tile -- so the way re-enters the
    same tiles again and again, and no scheme that runs a tile at most once per round settles it in one round.  By the
    specification the cost at the far end (39, 39, 7) is 1162, and the CPU model of the tile schedule takes 46 rounds."""
    d2 = open_box((40, 40, 8))
    for k, x in enumerate(range(4, 40, 4)):
        d2[x] = 0
        if k % 2:
            d2[x, 38:] = NONE
        else:
            d2[x, :2] = NONE
    return case("the 40 x 40 x 8 serpentine", d2, [(0, 39, 0)], lo=(0, 0, 0))


SERPENTINE_FAR = (39, 39, 7)


def seed_rules_case():
    """Every seed rule at once on the random box: a seed outside the box, one on a blocked cell, a duplicate with two cost0
    values (the smaller one second), a seed dominated by its neighbour's wave, and seeds in several tiles."""
    n = (33, 20, 11)
    d2 = random_field(n, 0.35, 4)
    f = free_cells(d2, 1, 6, 9)
    solid = tuple(int(v) for v in np.argwhere(d2 == 0)[7])
    near = None
    for c in np.argwhere(d2 != 0):  # a free cell with a free neighbour along x
        if c[0] + 1 < n[0] and d2[c[0] + 1, c[1], c[2]] != 0:
            near = tuple(int(v) for v in c)
            break
    seeds = [(-1, 0, 0, 0), (33, 19, 10, 7), (0, 0, 11, 1), solid + (3,), f[0] + (40,), f[0] + (12,), f[1] + (0,), f[2] + (100,), f[3] + (1 << 24,),
             near + (50,), (near[0] + 1, near[1], near[2], 500)]  # 500 > 50 + 3: dominated
    return case("the seed rules", d2, seeds)


def cases():
    c = []
    c.append(case("1 x 1 x 1, free", open_box((1, 1, 1)), [(0, 0, 0, 9)]))
    c.append(case("1 x 1 x 1, blocked", np.zeros((1, 1, 1)), [(0, 0, 0, 9)]))
    for axis in range(3):
        n = [9, 10, 17]
        n[axis] = 1
        d2 = random_field(tuple(n), 0.25, 20 + axis)
        c.append(case("size 1 on axis %d" % axis, d2, free_cells(d2, 1, 2, axis)))
    for n in ((7, 8, 9), (8, 9, 17), (9, 17, 7), (17, 7, 8), (8, 8, 8)):
        c.append(case("open %d x %d x %d, a seed at every corner" % n, open_box(n), corners(n)))
    d2 = random_field((17, 17, 17), 0.2, 6)
    for k in corners((17, 17, 17)):
        d2[k[:3]] = NONE
    c.append(case("17 x 17 x 17, 20 % blocked, a seed at every corner", d2, corners((17, 17, 17))))
    # a wall two cells thick across the boundary between the tiles at x = 7 | 8, with a one-cell door
    d2 = open_box((16, 12, 10))
    d2[7:9] = 0
    d2[7:9, 5, 4] = NONE
    c.append(case("a wall across a tile boundary with a one-cell door", d2, [(1, 1, 1)]))
    # two free cubes that touch only at the corner (7, 7, 7) | (8, 8, 8): the weight-5 move across a tile corner
    d2 = np.zeros((16, 16, 16), np.uint32)
    d2[:8, :8, :8] = NONE
    d2[8:, 8:, 8:] = NONE
    c.append(case("two free regions that touch at a tile corner", d2, [(2, 3, 4)]))
    # ... and at a tile edge only (the weight-4 move): the cubes share the edge x = 7 | 8, y = 7 | 8
    d2 = np.zeros((16, 16, 8), np.uint32)
    d2[:8, :8] = NONE
    d2[8:, 8:] = NONE
    d2[7, 7, 1:] = 0
    c.append(case("two free regions that touch at one cell of a tile edge", d2, [(2, 3, 4)]))
    d2 = open_box((12, 12, 12))
    d2[3:10, 3:10, 3:10] = 0
    d2[4:9, 4:9, 4:9] = NONE
    c.append(case("an enclosed pocket", d2, [(0, 0, 0)]))
    c.append(case("an all-NONE field", open_box((10, 9, 8)), [(9, 0, 7, 2)]))
    # d2 exactly r2 and r2 - 1 side by side: stripes of 9 (free) and 8 (not), joined along one row
    d2 = np.full((11, 9, 10), 9, np.uint32)
    d2[1::2] = 8
    d2[:, 4, 5] = 9
    c.append(case("d2 = r2 and r2 - 1 side by side", d2, [(0, 0, 0)], r2=9))
    c.append(random_case())
    c.append(seed_rules_case())
    c.append(case("no seed is used", open_box((9, 9, 9)), [(-1, 0, 0), (0, 9, 0)]))
    c.append(case("a line of 128 tiles", open_box((1024, 1, 1)), [(0, 0, 0)], lo=(-512, 0, 0)))
    c.append(serpentine())
    return c


@functools.lru_cache(maxsize=None)
def cached_cases():
    return cases()


def starts_for(c, k=256, seed=3):
    """k starts for a case, all four statuses among them where the case allows: free cells, cells that are not, cells outside
    the box (absolute voxel indices)."""
    rng = np.random.default_rng(seed)
    n, lo = np.asarray(c["n"]), np.asarray(c["lo"])
    inside = rng.integers(0, n, (k, 3))
    inside[::16] = rng.integers(-2, n + 2, (len(inside[::16]), 3))
    inside[1] = (-1, 0, 0)
    inside[2] = n - 1 + (0, 1, 0)
    return [tuple(int(v) for v in r + lo) for r in inside]
