"""The cases shared by the TSDF tests (test_map_tsdf_cpu.py, test_gpu_map_tsdf.py), on map_seen_cases' geometry: voxel edge
1/8 m, the 16 x 12 camera at the origin looking down +z, the plane of cells with index 8 along z, each cell of it on a pixel of
its own.  With trunc = M (2^-6) the plane's marked pixels sit exactly on the rule's boundaries: |z - dc| == trunc, and one float32
step either side.  Test infrastructure only."""
import functools

import numpy as np

import map_carve_cases as cc
import map_seen_cases as sc
import map_tsdf_ref as tr

F = np.float32
V, M, I4, KC = sc.V, sc.M, sc.I4, sc.KC
LO, N = sc.LO, sc.N
CELL = tr.CELL

# further cells (i, j) of the plane -> what their pixel holds, their class with trunc = M and their quantum
EXTRA = {
    "inside_front_boundary": ((0, 2), sc.down(sc.PLANE_Z + F(M)), "confirmed", None),   # one step inside |z - dc| == trunc
    "inside_back_boundary": ((-3, 2), sc.up(sc.PLANE_Z - F(M)), "confirmed", None),
    "third": ((0, -1), sc.PLANE_Z + F(M) * F(0.3125), "confirmed", 320),                # (dc - z) / trunc = 5/16, exact
    "behind_quarter": ((2, -1), sc.PLANE_Z - F(M) * F(0.25), "confirmed", -256),
}
# the named cells of map_seen_cases.PIXELS, with trunc = M: their quantum (None: no update)
QUANTA = {"free": 1024, "confirmed": 0, "occluded": None, "free_boundary": 1024, "free_one_below": 1024, "confirmed_boundary": -1024,
          "occluded_one_above": None, "unknown_nan": None, "unknown_zero": None, "unknown_zmax": None, "edge_centre": 1024, "edge_neighbour": None}


def depth_plane():
    """map_seen_cases' 16 x 12 image with the pixels of EXTRA."""
    D = sc.depth_plane()
    for (i, j), d, _, _ in EXTRA.values():
        D[j + 6, i + 8] = d
    return D


def plane_cell(name):
    if name in EXTRA:
        (i, j) = EXTRA[name][0]
        return (i - LO[0], j - LO[1], 8 - LO[2])
    return sc.plane_cell(name)


def views_all():
    return [(depth_plane(), I4, KC)] + sc.views_all()[1:]


def fuse_cases():
    """name -> dict(lo, n, views, trunc): every hand-made fuse case of the CPU and the GPU tests."""
    c = {}
    for lo, n in sc.BOXES:  # 1x1x1, 3x5x7, 9x7x5 with lo < 0
        tag = "x".join(str(x) for x in n)
        c["%s trunc M" % tag] = dict(lo=lo, n=n, views=views_all(), trunc=M)
        c["%s default trunc" % tag] = dict(lo=lo, n=n, views=views_all(), trunc=None)
    c["plane alone"] = dict(lo=LO, n=N, views=[(depth_plane(), I4, KC)], trunc=M)
    c["two views"] = dict(lo=LO, n=N, views=[sc.tilted_view(7), sc.small_view()], trunc=0.25)
    c["behind"] = dict(lo=LO, n=N, views=[(depth_plane(), sc.BEHIND, KC)], trunc=M)
    c["borders"] = dict(lo=LO, n=N, views=sc.border_views(), trunc=None)
    c["64 views"] = dict(lo=LO, n=N, views=sc.views64(), trunc=None)
    for nz in (1, 3, 4, 5, 33):  # runs of four cells against z-lines of every length: n[0] * n[1] = 9
        c["3x3x%d" % nz] = dict(lo=(-1, -1, 6), n=(3, 3, nz), views=sc.z_views(), trunc=None)
    # 1035 cells: a full block of 1024, then a second block of two whole runs and a tail run of three cells -- the smallest box at
    # which a wrong block offset, or a wrong tail in a block that is not the first, shows
    c["3x3x115"] = dict(lo=(-1, -1, 6), n=(3, 3, 115), views=sc.z_views(), trunc=None)
    return c


@functools.lru_cache(maxsize=None)
def fuse_spec(name):
    """The per-cell specification of a case, computed once: (cells, info, per-view counts, classes)."""
    c = fuse_cases()[name]
    return tr.fuse(V, c["lo"], c["n"], c["views"], c["trunc"])


def nearly_full(n=N):
    """A hand-set volume one update under a full weight: two views that both reach a cell saturate it."""
    vol = np.zeros(tuple(n), CELL)
    vol["weight"] = tr.W_MAX - 1
    vol["sum"] = -7
    return vol


# -------------------------------------------------------------------------------------------------------------- the mesh --
def volume(s, w):
    out = np.zeros(np.shape(s), CELL)
    out["sum"], out["weight"] = s, w
    return out


def patterns(rng=None, zero_outside=False):
    """All 256 sign patterns of one cube in a single 47 x 47 x 2 box: the cube of the pattern 16 i + j at the cell (3 i, 3 j, 0), a
    plane of weight-0 cells between neighbours.  rng: weights 1 .. 2^20 and sums up to 2^30 in size; else weight 1, sum -1 / +1
    (zero_outside: 0 for the outside corners)."""
    s, w = np.zeros((47, 47, 2), np.int64), np.zeros((47, 47, 2), np.int64)
    for p in range(256):
        i, j = divmod(p, 16)
        for v in range(8):
            at = (3 * i + (v & 1), 3 * j + ((v >> 1) & 1), (v >> 2) & 1)
            inside = (p >> v) & 1
            if rng is None:
                w[at], s[at] = 1, (-1 if inside else (0 if zero_outside else 1))
            else:
                w[at] = int(rng.choice([1, 2, 3, 1 << 20, int(rng.integers(1, (1 << 20) + 1))]))
                big = int(rng.choice([1, 1 << 30, int(rng.integers(1, (1 << 30) + 1))]))
                s[at] = -big if inside else int(rng.choice([0, big, big]))
    return volume(s, w)


def sphere(n=12, r=4.2):
    """A ball of radius r cells in the middle of an n^3 box: every cell valid, the surface well inside the box."""
    g = np.arange(n) - (n - 1) / 2.0
    d = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    return volume(np.rint((d - r) * 1000.0).astype(np.int64), np.ones((n, n, n), np.int64))


def random_volume(seed, n, max_weight=4):
    rng = np.random.default_rng(seed)
    return volume(rng.integers(-50, 50, n), rng.integers(0, max_weight + 1, n))


def mesh_cases():
    """name -> dict(cells, lo, min_weight): every hand-made mesh case of the CPU and the GPU tests."""
    c = {"256 patterns": dict(cells=patterns(), lo=(-20, 3, -1), min_weight=1),
         "256 patterns, random weights": dict(cells=patterns(np.random.default_rng(26)), lo=(0, 0, 0), min_weight=1),
         "256 patterns, zero sums": dict(cells=patterns(zero_outside=True), lo=(5, -50, 7), min_weight=1),
         "sphere": dict(cells=sphere(), lo=(-6, -6, 4), min_weight=1)}
    for mw in (0, 1, 3):
        c["min_weight %d" % mw] = dict(cells=random_volume(3, (5, 4, 6)), lo=(-2, 0, 9), min_weight=mw)
    for n in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (1, 1, 1)):
        c["no cube %dx%dx%d" % n] = dict(cells=random_volume(4, n, 1), lo=(0, -3, 2), min_weight=1)
    for seed in (1, 2, 3):
        v = random_volume(10 + seed, (2, 2, 3), 1)
        v["weight"] = 1
        c["shared face %d" % seed] = dict(cells=v, lo=(-1, -1, -1), min_weight=1)
    c["300 cells in a line of blocks"] = dict(cells=random_volume(5, (2, 2, 75), 6), lo=(0, 0, -40), min_weight=2)
    return c


@functools.lru_cache(maxsize=None)
def mesh_spec(name):
    """(vertices, triangles, info) of a case from the per-cube loop, computed once."""
    c = mesh_cases()[name]
    return tr.mesh(c["cells"], c["lo"], V, c["min_weight"])


WALL_DEPTH = F(1.09)


def wall():
    """A fronto-parallel wall at WALL_DEPTH seen by the plane's camera, over the box (LO, N) with the default trunc (1/2 m): every
    cell is CONFIRMED, the zero crossing lies between the planes iz = 2 and iz = 3 -> dict(lo, n, views, trunc)."""
    return dict(lo=LO, n=N, views=[(np.full((12, 16), WALL_DEPTH, F), I4, KC)], trunc=None)


def scene64():
    """The 64^3 box of DESIGN 19's scene with its four views."""
    lo, n = sc.scene_box(64)
    return lo, n, cc.scene_views(False)


# ------------------------------------------------------------------------------------------------------ mesh properties --
def closed_mesh_numbers(vertices, triangles):
    """(V, E, F, every undirected edge in exactly two triangles once in each direction, six times the signed volume)."""
    t = np.asarray(triangles, np.int64)
    directed = {}
    for a, b, c in t.tolist():
        for e in ((a, b), (b, c), (c, a)):
            directed[e] = directed.get(e, 0) + 1
    ok = all(n == 1 and directed.get((b, a), 0) == 1 for (a, b), n in directed.items())
    p = np.asarray(vertices, np.float64)
    vol6 = float(np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]])).sum()) if len(t) else 0.0
    return len(np.unique(t)), len(directed) // 2, len(t), ok, vol6
