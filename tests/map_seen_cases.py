"""The cases shared by the known-space tests (test_map_seen_cpu.py, test_gpu_map_seen.py).

The hand-made geometry: voxel edge 1/8 m, the camera at the origin looking down +z with fx = fy = 8.5 and the plane of cells
with index 8 along z (centres at z = 17/16 m).  There u = 8.5 * x / (17/16) + cx = 8 * x + cx, and a cell of index i along x has
x = (i + 1/2) / 8, so u = i + 1/2 + cx: with cx = 7.5 the cell lands exactly on pixel i + 8, each cell of the plane on a pixel of
its own (and likewise along y with cy = 5.5: pixel j + 6).  Every product and quotient on the way is exact in float32, so what a
case says about z, the pixel and the depths is what the rule sees; with radius 0 a cell's class is decided by its own pixel.
Test infrastructure only."""
import functools

import numpy as np

import map_carve_cases as cc
import map_carve_ref as mc
import map_records_ref as mrr
import map_seen_ref as sr
import voxel_map_ref as ref

F = np.float32
I4 = np.eye(4, dtype=F)
V = 0.125
ZMIN, ZMAX = cc.ZMIN, cc.ZMAX
M = cc.M                                      # 2^-6: the margin of the hand-made cases, exact
KC = (8.5, 8.5, 7.5, 5.5, ZMIN, ZMAX)         # the 16 x 12 camera of the plane
K8 = (8.5, 8.5, 3.5, 3.5, ZMIN, ZMAX)         # an 8 x 8 image: pixel i + 4, j + 4
PLANE_Z = F(17.0 / 16.0)
LO, N = (-4, -3, 6), (9, 7, 5)                # the plane is iz = 2; pixels 4 .. 12 x 3 .. 9
BOXES = (((-4, -3, 8), (1, 1, 1)), ((-1, -2, 5), (3, 5, 7)), (LO, N))
BEHIND = np.diag(F([-1, 1, -1, 1]))           # looks down -z: every cell of the boxes is behind the camera


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


# the cell (i, j) of the plane (voxel indices along x, y) -> what its pixel holds, and its class at radius 0 with margin M
PIXELS = {
    "free": ((-4, 3), F(2.0), "free"),                              # no marked pixel within three of it
    "confirmed": ((1, 0), PLANE_Z, "confirmed"),
    "occluded": ((2, 0), F(0.5), "occluded"),
    "free_boundary": ((-1, 1), PLANE_Z + F(M), "confirmed"),        # z == dmin - m is not free; |z - dc| == mc is confirmed
    "free_one_below": ((-2, 1), up(PLANE_Z + F(M)), "free"),        # the depth one float32 step farther: z < dmin - m
    "confirmed_boundary": ((1, 1), PLANE_Z - F(M), "confirmed"),    # |z - dc| == mc
    "occluded_one_above": ((2, 1), down(PLANE_Z - F(M)), "occluded"),  # one step nearer: z - dc > mc
    "unknown_nan": ((-3, -2), F(np.nan), "unknown"),
    "unknown_zero": ((-1, -2), F(0.0), "unknown"),
    "unknown_zmax": ((1, -2), ZMAX, "unknown"),
    "edge_centre": ((3, 2), F(3.0), "free"),                        # at radius >= 1 the neighbour below makes it an edge
    "edge_neighbour": ((3, 3), F(0.9), "occluded"),
}


def depth_plane():
    """The 16 x 12 image: 2 m everywhere but for PIXELS."""
    D = np.full((12, 16), 2.0, F)
    for (i, j), d, _ in PIXELS.values():
        D[j + 6, i + 8] = d
    return D


def plane_cell(name):
    """The index in the box (LO, N) of a named cell of the plane."""
    (i, j), _, _ = PIXELS[name]
    return (i - LO[0], j - LO[1], 8 - LO[2])


def border_views():
    """Four flat views whose principal point puts the plane's cells on and next to each image border."""
    flat = np.full((12, 16), 2.0, F)
    return [(flat, I4, (8.5, 8.5, 3.5, 5.5, ZMIN, ZMAX)),    # pixels 0 .. 8 along u: the left border
            (flat, I4, (8.5, 8.5, 11.5, 5.5, ZMIN, ZMAX)),   # 8 .. 16: the right border and one beyond it
            (flat, I4, (8.5, 8.5, 7.5, 2.5, ZMIN, ZMAX)),    # 0 .. 6 along v: the top
            (flat, I4, (8.5, 8.5, 7.5, 8.5, ZMIN, ZMAX))]    # 6 .. 12: the bottom and one beyond it


def small_view():
    D = np.full((8, 8), 1.5, F)
    D[2, 5], D[6, 1] = np.inf, F(0.8)
    return (D, I4, K8)


def tilted_view(seed=3):
    """A 16 x 12 view with random depths and holes from a small random pose: nothing about it is exact."""
    from revo_amd import synth
    rng = np.random.default_rng(seed)
    D = rng.choice(np.array([0.9, 1.0625, 1.25, 2.0, 2.0, 3.0], F), (12, 16))
    D[rng.uniform(size=D.shape) < 0.08] = rng.choice(np.array([0.0, np.nan, np.inf, 6.0], F))
    T = synth.se3_exp(np.concatenate([rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.04, 0.04, 3)])).astype(F)
    return (D, T, KC)


def views_all():
    return [(depth_plane(), I4, KC)] + border_views() + [small_view(), tilted_view(), (depth_plane(), BEHIND, KC)]


def views64():
    """64 views: the eight of views_all over and over, each round with another flat depth in the plane view's free pixels."""
    out = []
    for k in range(8):
        vs = views_all()
        D = vs[0][0].copy()
        D[D == F(2.0)] = F(1.5 + 0.25 * k)
        out += [(D, I4, KC)] + vs[1:]
    return out


def cases():
    """name -> dict(lo, n, views, radius, margin, margin_rel): every hand-made observe case of the CPU and the GPU tests."""
    c = {}
    for lo, n in BOXES:
        tag = "x".join(str(x) for x in n)
        for r in range(4):
            c["%s radius %d" % (tag, r)] = dict(lo=lo, n=n, views=views_all(), radius=r, margin=M, margin_rel=0.0)
    c["plane alone, radius 0"] = dict(lo=LO, n=N, views=[(depth_plane(), I4, KC)], radius=0, margin=M, margin_rel=0.0)
    c["relative margin"] = dict(lo=LO, n=N, views=views_all()[:2] + [tilted_view(5)], radius=1, margin=0.0, margin_rel=0.03125)
    c["default margin"] = dict(lo=LO, n=N, views=[tilted_view(7), small_view()], radius=1, margin=None, margin_rel=0.0)
    c["behind"] = dict(lo=LO, n=N, views=[(depth_plane(), BEHIND, KC)], radius=1, margin=M, margin_rel=0.0)
    c["64 views"] = dict(lo=LO, n=N, views=views64(), radius=1, margin=M, margin_rel=0.0)
    return c


@functools.lru_cache(maxsize=None)
def spec(name):
    """The per-cell specification of a case, computed once: (seen, info, per-view counts, classes)."""
    c = cases()[name]
    return sr.observe(V, c["lo"], c["n"], c["views"], c["radius"], c["margin"], c["margin_rel"])


def z_boxes():
    """Boxes whose z-lines start at every alignment of the volume's words, the cell counts around a block, and 1035 cells: a full
    block of 1024, then a second block with a tail word of three cells."""
    out = [((-1, -1, 6), (3, 3, nz)) for nz in (1, 3, 4, 5, 31, 32, 33, 65, 115)]
    return out + [((-1, -2, 4), (3, 5, 17)), ((-2, -4, 5), (4, 8, 8)), ((-128, 0, 8), (257, 1, 1))]


def z_views():
    return [tilted_view(11), small_view()]


# ----------------------------------------------------------------------------------------- volumes for field and frontiers --
def records_at(cells, counts=None):
    """Map records with one voxel per cell (absolute voxel indices), in ascending key order."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    rec = np.zeros(len(cells), mrr.DTYPE)
    rec["key"] = ref.pack_keys(cells)
    rec["count"] = 1 if counts is None else counts
    rec["sum_q"] = np.rint((cells + 0.5) * V * 2.0 ** 20).astype(np.int64) * rec["count"].astype(np.int64)[:, None]
    return rec[np.argsort(rec["key"])]


def random_volume(seed, lo=(-7, 3, -2), n=(33, 20, 11), voxels=25):
    """A random box: a few voxels (some with count 1, below a min_count of 2) and a seen volume with every kind of byte."""
    rng = np.random.default_rng(seed)
    lo, n = np.asarray(lo, np.int64), np.asarray(n, np.int64)
    cells = np.unique(rng.integers(lo - 1, lo + n + 1, (voxels, 3)), axis=0)
    rec = records_at(cells, rng.integers(1, 4, len(cells)))
    seen = rng.choice(np.array([0, 0, 0, 1, 2, 3, 0x7F, 0x80, 0x81, 0xFF], np.uint8), tuple(n))
    seen[rng.integers(0, n[0]):, :, :rng.integers(1, n[2])] = 0   # a block of unseen space
    return dict(lo=lo, n=n, rec=rec, seen=seen)


def wall_scene():
    """The route's world: a 24 x 16 x 16 box of 1/8 m cells from the origin; a wall of voxels in the plane x = 12 that leaves
    the cells y >= 12 open; a flat depth image looking down +x from 1 m in front of the box onto the wall's plane, whose top
    rows (the rays towards high z) hold no depth -> dict(lo, n, rec, views, start, goal).  In front of the wall the cells are
    free up to x = 10, the planes x = 11 .. 13 carry the surface bit, everything behind them and under the hole is unseen."""
    lo, n = (0, 0, 0), (24, 16, 16)
    wall = [(12, y, z) for y in range(12) for z in range(16)]
    # the camera at (-1, 1, 1) m: camera x = -world y, camera y = -world z, camera z = world x
    T = np.array([[0, 0, 1, -1.0], [-1, 0, 0, 1.0], [0, -1, 0, 1.0], [0, 0, 0, 1]], F)
    D = np.full((96, 96), 1.0 + 12.5 * V, F)    # the wall's cell centres lie at world x = 12.5 / 8 m
    D[:40] = np.nan
    k = (40.0, 40.0, 47.5, 47.5, F(0.1), F(8.0))
    return dict(lo=lo, n=n, rec=records_at(wall), views=[(D, T, k)], start=(2, 8, 8), goal=(20, 8, 8))


# ------------------------------------------------------------------------------------------------------------ the scene --
def scene_box(size=64):
    """A size^3 box around the middle of DESIGN 19's scene map."""
    rec = cc.scene_records()
    lo, hi = sr.fr.key_axes(rec["key"]).min(0), sr.fr.key_axes(rec["key"]).max(0)
    return (lo + hi) // 2 - size // 2, np.full(3, size, np.int64)


assert mc.FREE == 2 and mc.CONFIRMED == 3
