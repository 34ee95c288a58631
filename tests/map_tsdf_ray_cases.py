"""The cases shared by the surface ray-cast tests (test_map_tsdf_ray_cpu.py, test_gpu_map_tsdf_ray.py), on map_tsdf_cases'
geometry: voxel edge 1/8 m and the 16 x 12 camera at the origin looking down +z.  With zmin = 0.1 and the default step of one
voxel edge a ray's samples sit at u_z = k + 0.8 - (lo_z + 0.5) cells; with zmin = 1/16 they sit exactly on the cell centres, so
that F is a cell's own field.  Each case is one call: the smallest shape at which its rule can go wrong.  Test infrastructure
only."""
import functools
import zlib

import numpy as np

import map_seen_cases as sc
import map_surface_cases as su
import map_surface_ref as sf
import map_tsdf_cases as tc
import map_tsdf_ray_ref as rr

F = np.float32
V, I4, KC = tc.V, sc.I4, sc.KC
SIZE = (16, 12)
ZMIN, ZMAX = sc.ZMIN, sc.ZMAX
K0 = (8.5, 8.5, 8.0, 6.0, ZMIN, ZMAX)           # the principal point on a pixel: pixel (8, 6) casts (0, 0, 1)
KCENTRES = KC[:4] + (F(1.0 / 16.0), ZMAX)       # samples on the cell centres along z
ALONG_X = np.array([[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], F)   # the camera's z axis is the world's x axis
ALONG_Y = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], F)   # ... the world's y axis


def at(T, x, y, z):
    T = np.array(T, F)
    T[:3, 3] = (x, y, z)
    return T


def behind(z):
    """Looks down -z from (0, 0, z)."""
    return at(sc.BEHIND, 0, 0, z)


def layers(n, axis, values, weight=1):
    """A volume whose field depends on the cell's index along `axis` alone: values[i] is the sum of layer i (None: weight 0)."""
    s, w = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i, v in enumerate(values):
        sl = [slice(None)] * 3
        sl[axis] = i
        s[tuple(sl)], w[tuple(sl)] = (0 if v is None else v), (0 if v is None else weight)
    return tc.volume(s, w)


def colour(cells, name):
    return su.colour_volume(cells.shape, zlib.crc32(name.encode()))


def big_numbers():
    """Weights up to 2^20 and sums up to +-2^30, positive in the three layers nearest the camera and negative behind them."""
    rng = np.random.default_rng(28)
    n = (4, 4, 6)
    w = rng.choice(np.array([1, 2, 3, 1 << 20, 77777], np.int64), n)
    big = rng.choice(np.array([1, 1 << 30, (1 << 30) - 1, 123456789], np.int64), n)
    s = np.where(np.arange(6)[None, None, :] < 3, big, -big)
    return tc.volume(s, w)


@functools.lru_cache(maxsize=None)
def wall():
    """map_tsdf_cases' wall fused from one view with a constant colour image -> (cells, colour cells, lo)."""
    w = tc.wall()
    cells, _, _, col, _ = sf.fuse_color(V, w["lo"], w["n"], w["views"], [su.wall_image()], w["trunc"])
    return cells, col, w["lo"]


def _case(cells, lo, views, kind, color="auto", name="", **prm):
    views = [(np.asarray(T, F), tuple(k), tuple(size)) for T, k, size in views]
    return dict(cells=cells, color=colour(cells, name) if isinstance(color, str) else color, lo=tuple(int(x) for x in lo), views=views, kind=kind,
                step=prm.get("step"), min_weight=prm.get("min_weight", 1), max_steps=prm.get("max_steps", 4096))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(cells, color, lo, views, step, min_weight, max_steps, kind).  kind: "hit" -- built to hit, "miss" -- built so that
    no ray hits, "mixed" -- whatever the rule gives."""
    front = (I4, KC, SIZE)
    c = {}

    def add(name, cells, lo, views, kind, **kw):
        c[name] = _case(cells, lo, views, kind, name=name, **kw)

    # one interpolation cube around the optical axis, four samples inside it
    add("2x2x2", layers((2, 2, 2), 2, [100, -100]), (-1, -1, 7), [front], "hit", step=1.0 / 32.0)
    for n in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        add("axis of 1: %dx%dx%d" % n, layers(n, 2, [100, 50, -50, -100, -100][:n[2]]), (-2 if n[0] > 1 else 0, -2 if n[1] > 1 else 0, 6), [front], "miss")
    add("3x5x7 lo < 0", layers((3, 5, 7), 2, [300, 200, 100, 30, -70, -170, -270], weight=3), (-1, -2, 5), [front], "hit")
    # the sign change between the cells 7 and 8, the zero at 7.9: the samples at 7.3 and 8.3 straddle the border of the mask's blocks
    ramp = [90 + 100 * (7 - i) for i in range(8)] + [-10 - 100 * (i - 8) for i in range(8, 17)]
    add("9x9x17 block border z", layers((9, 9, 17), 2, ramp), (-4, -4, 2), [front], "hit")
    add("17x9x9 block border x", layers((17, 9, 9), 0, ramp), (2, -4, -4), [(ALONG_X, KC, SIZE)], "hit")
    add("9x17x9 block border y", layers((9, 17, 9), 1, ramp), (-4, 2, -4), [(ALONG_Y, KC, SIZE)], "hit")
    add("big numbers", big_numbers(), (-2, -2, 6), [front], "hit")
    # samples on the cell centres: F == 0 as the previous sample of a hit (from the front) and as the end of a backface (from behind)
    zero = layers((5, 5, 5), 2, [100, 100, 0, -100, -100])
    add("zero sums", zero, (-2, -2, 6), [(I4, KCENTRES, SIZE), (behind(3.0), KCENTRES, SIZE)], "mixed")
    add("unknown layer between", layers((5, 5, 6), 2, [100, 100, None, -100, -100, -100]), (-2, -2, 6), [front], "miss")
    hole = layers((5, 5, 6), 2, [100, 100, 100, -100, -100, -100])
    hole["weight"][2, 2, 2] = 0
    add("unknown cell between", hole, (-2, -2, 6), [front], "mixed")
    # a layer one cell thick, samples three cells apart at 0.3, 3.3 and 6.3 cells: the march steps over it
    add("thin layer stepped over", layers((5, 5, 9), 2, [100, 100, 100, 100, -100, 100, 100, 100, 100]), (-2, -2, 6), [front], "miss", step=0.375)
    add("thin layer met", layers((5, 5, 9), 2, [100, 100, 100, 100, -100, 100, 100, 100, 100]), (-2, -2, 6), [front], "hit")
    add("behind the wall", layers((5, 5, 7), 2, [300, 200, 100, 30, -70, -170, -270]), (-2, -2, 6), [(behind(2.5), KC, SIZE)], "miss")
    add("inside and outside the box", layers((9, 9, 17), 2, ramp), (-4, -4, 2), [(at(I4, 0.05, -0.02, 0.6), KC, SIZE), (at(I4, 0, 0, -0.5), KC, SIZE),
                                                                                    (at(I4, 3.0, 0, 0), KC, SIZE)], "mixed")
    add("max_steps 1", layers((9, 9, 17), 2, ramp), (-4, -4, 2), [front], "miss", max_steps=1)
    add("max_steps reaches the hit", layers((9, 9, 17), 2, ramp), (-4, -4, 2), [front], "hit", max_steps=11)   # the hit is sample 10
    add("max_steps one short", layers((9, 9, 17), 2, ramp), (-4, -4, 2), [front], "miss", max_steps=10)
    add("zmax inside the box", layers((9, 9, 17), 2, ramp), (-4, -4, 2), [(I4, KC[:4] + (ZMIN, F(1.2)), SIZE)], "miss")
    add("zero direction components", layers((9, 9, 17), 2, ramp), (-4, -4, 2), [(I4, K0, SIZE)], "hit")
    rnd = tc.random_volume(28, (6, 5, 7), 4)
    rnd["sum"] = np.where(np.arange(7)[None, None, :] < 3, np.abs(rnd["sum"]) + 1, -np.abs(rnd["sum"]) - 1)
    for mw in (0, 1, 3):
        add("min_weight %d" % mw, rnd, (-3, -2, 6), [front], "mixed", min_weight=mw)
    add("1x1 and 16x12", layers((3, 5, 7), 2, [300, 200, 100, 30, -70, -170, -270]), (-1, -2, 5), [(I4, (8.5, 8.5, 0.0, 0.0, ZMIN, ZMAX), (1, 1)), front], "hit")
    rng = np.random.default_rng(64)
    many = [(at(I4, *(rng.uniform(-0.1, 0.1, 3))), (8.5, 8.5, 0.5, 0.5, ZMIN, ZMAX), (2, 2)) for _ in range(64)]
    add("64 views", layers((5, 5, 7), 2, [300, 200, 100, 30, -70, -170, -270]), (-2, -2, 6), many, "hit")
    # long boxes with the surface in the last of four blocks of the mask, and a tilted plane through 3 x 3 x 3 blocks: most of a
    # ray's samples lie in unmarked blocks, which the kernel steps over in runs
    far = [100 * (28 - i) + 50 for i in range(33)]
    tele = (34.0, 34.0, 7.5, 5.5, ZMIN, ZMAX)  # four times the focal length: the whole image looks down the long box
    add("far wall 5x5x33", layers((5, 5, 33), 2, far), (-2, -2, 2), [(I4, tele, SIZE)], "hit")
    add("far wall 33x5x5", layers((33, 5, 5), 0, far), (2, -2, -2), [(ALONG_X, tele, SIZE)], "hit")
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(20), indexing="ij"), -1)
    tilted = tc.volume(np.rint(((np.array([15.0, 12.0, 14.0]) - g) * np.array([0.3, -0.2, 0.9])).sum(-1) * 100).astype(np.int64), np.ones((20, 20, 20), np.int64))
    add("tilted plane 20x20x20", tilted, (-10, -10, 4), [front, (at(I4, 0.4, -0.3, 0.3), KC, SIZE)], "hit")
    cells, col, lo = wall()
    add("wall", cells, lo, [front], "hit", color=col)
    add("sphere", tc.sphere(), (-6, -6, 4), [front], "hit")
    add("sphere without colour", tc.sphere(), (-6, -6, 4), [front], "hit", color=None)
    return c


@functools.lru_cache(maxsize=None)
def spec(name):
    """The loop's result of a case, computed once."""
    c = cases()[name]
    return rr.raycast(c["cells"], c["color"], c["lo"], V, c["views"], c["step"], c["min_weight"], c["max_steps"])


def args(c):
    """A case as mapfile.tsdf_raycast_records takes it."""
    return (c["cells"], c["color"], c["lo"], V, c["views"]), dict(step=c["step"], min_weight=c["min_weight"], max_steps=c["max_steps"])
