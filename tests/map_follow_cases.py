"""The cases shared by the tests of a box that follows the camera (test_map_follow_cpu.py, test_gpu_map_follow.py), on
map_tsdf_cases' 1/8 m cells and 16 x 12 camera: boxes whose z-lines take every length against the move kernel's runs of four cells,
shifts at every alignment of the source run and at the box's rims, volumes fused and hand-set within FITS, and the poses a following
surface is driven through.  Test infrastructure only."""
import functools
import zlib

import numpy as np

import map_follow_ref as fr
import map_seen_cases as sc
import map_surface_cases as su
import map_tsdf_cases as tc

F = np.float32
V, KC, I4 = tc.V, tc.KC, tc.I4
CELL, COLOR, RECORD = fr.CELL, fr.COLOR, fr.RECORD

BOX_357 = ((-1, -2, 5), (3, 5, 7))          # lo < 0
BOX_300 = ((0, 0, -40), (2, 2, 75))         # 300 cells: the 75 runs of four and the 300 leaving cells span two blocks of 256
BOX_BIG = ((-32, -32, 0), (64, 64, 65))     # 266 240 cells: more than one pass of the 1024-block x 256-cell scan


def z_deltas(nz):
    """delta_z at every alignment of the source run, at the box's size and one past it."""
    return sorted({0, 1, -1, 3, -3, 4, -4, 5, -5, nz, -nz, nz + 1, -(nz + 1)})


def random_volume(seed, n, color=True):
    """Hand-set bytes within FITS: the limits themselves, about a quarter of the cells EMPTY, and the cell (0, 0, 0) with weight 0 and a
    sum that is not 0 -- not EMPTY, though no fuse leaves it."""
    rng = np.random.default_rng(seed)
    n = tuple(int(x) for x in n)
    cells, col = np.zeros(n, CELL), np.zeros(n, COLOR)
    keep = rng.uniform(size=n) >= 0.25
    cells["weight"] = rng.choice(np.array([0, 1, 2, 1 << 20, int(rng.integers(1, 1 << 20))], np.int64), n) * keep
    cells["sum"] = rng.choice(np.array([-(1 << 30), 1 << 30, -1, 0, 1, int(rng.integers(-(1 << 30), 1 << 30))], np.int64), n) * keep
    col["weight"] = rng.choice(np.array([0, 1, 1 << 20], np.int64), n) * keep
    for k in ("sum_b", "sum_g", "sum_r"):
        col[k] = rng.choice(np.array([0, 255, 255 << 20, int(rng.integers(0, 255 << 20))], np.int64), n) * keep
    cells[0, 0, 0] = (-7, 0)
    col[0, 0, 0] = (0, 0, 0, 0)
    return cells, (col if color else None)


def full_volume(seed, n):
    """Every cell with a weight, so that every leaving cell gives a record; vectorised, for the large box."""
    rng = np.random.default_rng(seed)
    n = tuple(int(x) for x in n)
    cells, col = np.zeros(n, CELL), np.zeros(n, COLOR)
    cells["weight"] = rng.integers(1, 1 << 20, n)
    cells["sum"] = rng.integers(-(1 << 30), 1 << 30, n)
    col["weight"] = rng.integers(0, 1 << 20, n)
    col["sum_b"] = rng.integers(0, 255 << 20, n)
    return cells, col


@functools.lru_cache(maxsize=None)
def fused(name, color):
    """(cells, colour or None, lo) of one of map_tsdf_cases' fuse cases, from the per-cell specification."""
    c = tc.fuse_cases()[name]
    if color:
        s = su.fuse_spec(name)
        return s[0], s[3], c["lo"]
    return tc.fuse_spec(name)[0], None, c["lo"]


@functools.lru_cache(maxsize=None)
def shift_cases():
    """name -> dict(cells, color, lo, delta): every small shift case of the CPU and the GPU tests."""
    c = {}

    def add(name, vol, lo, delta):
        c[name] = dict(cells=vol[0], color=vol[1], lo=tuple(int(x) for x in lo), delta=tuple(int(x) for x in delta))

    one = random_volume(1, (1, 1, 1))
    one[0][0, 0, 0], one[1][0, 0, 0] = (5, 2), (1, 2, 3, 1)
    for d in ((0, 0, 0), (1, 0, 0), (0, 0, -1), (-2, 3, 0)):
        add("1x1x1 by %s" % (d,), one, (-4, -3, 8), d)
    for j, d in enumerate(((0, 0, 0), (1, -2, 3), (-1, 2, -3), (2, 4, -6), (-2, -4, 6), (3, 0, 0), (0, -5, 0), (-1, 1, 0), (1, 1, 1))):
        add("3x5x7 by %s" % (d,), random_volume(10 + j, BOX_357[1], color=j % 2 == 0), BOX_357[0], d)
    for nz in (1, 3, 4, 5, 33):  # runs of four cells against z-lines of every length: n[0] * n[1] = 9
        for j, dz in enumerate(z_deltas(nz)):
            add("3x3x%d by dz %d" % (nz, dz), random_volume(100 * nz + j, (3, 3, nz), color=j % 3 != 2), (-1, -1, 6), (0, 0, dz))
        add("3x3x%d by (1, -1, 1)" % nz, random_volume(7 * nz, (3, 3, nz)), (-1, -1, 6), (1, -1, 1))
    for d in ((0, 0, 0), (1, -1, 4), (0, 0, 37), (-1, 1, -5), (0, 1, 3), (0, 0, -76)):
        add("2x2x75 by %s" % (d,), random_volume(zlib.crc32(repr(d).encode()), BOX_300[1]), BOX_300[0], d)
    for color in (True, False):  # fused volumes, with and without colour
        tag = "colour" if color else "no colour"
        add("fused 3x5x7, %s, by (1, -2, 3)" % tag, fused("3x5x7 trunc M", color)[:2], fused("3x5x7 trunc M", color)[2], (1, -2, 3))
        add("fused 3x5x7, %s, by (0, 0, 4)" % tag, fused("3x5x7 trunc M", color)[:2], fused("3x5x7 trunc M", color)[2], (0, 0, 4))
        add("fused 3x3x5, %s, by (0, 0, -4)" % tag, fused("3x3x5", color)[:2], fused("3x3x5", color)[2], (0, 0, -4))
        add("fused 3x3x33, %s, by (-1, 0, 8)" % tag, fused("3x3x33", color)[:2], fused("3x3x33", color)[2], (-1, 0, 8))
    add("all EMPTY, with colour", (np.zeros((3, 3, 4), CELL), np.zeros((3, 3, 4), COLOR)), (0, 0, 0), (1, 1, 1))
    add("all EMPTY, no colour", (np.zeros((3, 3, 5), CELL), None), (0, 0, 0), (0, 0, -5))
    return c


@functools.lru_cache(maxsize=None)
def shift_spec(name):
    """(cells2, color2, records, info) of a case from the per-cell loop, computed once."""
    c = shift_cases()[name]
    return fr.shift(c["cells"], c["color"], c["lo"], c["delta"])


@functools.lru_cache(maxsize=None)
def big_case():
    """The 64 x 64 x 65 box leaving entirely: 266 240 records."""
    cells, col = full_volume(30, BOX_BIG[1])
    return dict(cells=cells, color=col, lo=BOX_BIG[0], delta=(64, 0, 0))


def composition_cases():
    """(volume seed, box, d1, d2) with no opposite signs on any axis, for property (b)."""
    return [(1, BOX_357, (1, 0, 2), (1, -1, 1)), (2, BOX_357, (0, -2, -3), (-1, -1, 0)), (3, BOX_357, (2, 2, 2), (2, 3, 6)),
            (4, ((-1, -1, 6), (3, 3, 33)), (0, 0, 3), (1, 0, 4)), (5, BOX_300, (0, 1, 30), (0, 0, 50)), (6, BOX_357, (0, 0, 0), (1, 1, -1))]


# ------------------------------------------------------------------------------------------------------ a following surface --
FOLLOW_N, FOLLOW_STEP = (12, 10, 8), 2


def follow_views():
    """Six poses of the case camera that move a 12 x 10 x 8 box (step 2, ahead 1/2 m) on every axis and bring it back to where it
    started, each with a depth image around the box's depth and a colour image -> [(depth, T_w_c, intrinsics, bgr)]."""
    from revo_amd import synth
    rng = np.random.default_rng(30)
    turn = synth.se3_exp(np.array([0, 0, 0, 0.02, -0.03, 0.01])).astype(F)
    steps = [(0, 0, 0), (0.5, 0, 0), (0.5, 0.375, 0), (0.5, 0.375, 0.25), (0, 0, 0.25), (0, 0, 0)]
    out = []
    for j, t in enumerate(steps):
        T = np.eye(4, dtype=F) if j != 2 else turn.copy()
        T[:3, 3] = F(t)
        D = rng.choice(np.array([0.4, 0.5625, 0.6875, 0.8125, 1.0, 2.0], F), (12, 16))
        D[rng.uniform(size=D.shape) < 0.06] = np.nan
        out.append((D, T, KC, rng.integers(0, 256, (12, 16, 3), dtype=np.uint8)))
    return out
