"""The cases shared by the surface tests (test_map_surface_cpu.py, test_gpu_map_surface.py): map_tsdf_cases' fuse cases
with a random seeded BGR image per view, and its mesh cases with a hand-set colour volume whose weights are 0 in about half of the
cells, so that the vertices' k takes 0, 1 and 2.  Test infrastructure only."""
import functools
import zlib

import numpy as np

import map_surface_ref as sf
import map_tsdf_cases as tc
import map_tsdf_ref as tr

F = np.float32
V = tc.V
COLOR = sf.COLOR

# boxes 1x1x1 and 3x5x7 with lo < 0; 1, 2 and 64 views; z-lines of 1, 3, 4, 5 and 33 cells against the kernel's runs of four
FUSE_NAMES = ("1x1x1 trunc M", "3x5x7 trunc M", "3x5x7 default trunc", "plane alone", "two views", "borders", "64 views",
              "3x3x1", "3x3x3", "3x3x4", "3x3x5", "3x3x33")


def images(views, seed):
    """One random [h, w, 3] uint8 image per view."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, np.shape(v[0]) + (3,), dtype=np.uint8) for v in views]


def fuse_cases():
    """name -> dict(lo, n, views, trunc, bgr)."""
    base = tc.fuse_cases()
    return {name: dict(base[name], bgr=images(base[name]["views"], zlib.crc32(name.encode()))) for name in FUSE_NAMES}


@functools.lru_cache(maxsize=None)
def fuse_spec(name):
    """The per-cell specification of a case, computed once: (cells, info, per-view counts, colour cells, colour info)."""
    c = fuse_cases()[name]
    return sf.fuse_color(V, c["lo"], c["n"], c["views"], c["bgr"], c["trunc"])


def nearly_full(n):
    """A hand-set pair of volumes one update under a full TSDF weight: of two CONFIRMED views the second is dropped from both."""
    vol = tc.nearly_full(n)
    col = np.zeros(tuple(n), COLOR)
    col["weight"] = 5
    col["sum_b"], col["sum_g"], col["sum_r"] = 100, 200, 1275
    return vol, col


def colour_volume(shape, seed):
    """Hand-set colour cells: weight 0 in about half of the cells, sums up to 255 x weight."""
    rng = np.random.default_rng(seed)
    out = np.zeros(shape, COLOR)
    w = rng.choice(np.array([0, 0, 1, 3, 1 << 20], np.int64), shape)
    out["weight"] = w
    for name in ("sum_b", "sum_g", "sum_r"):
        out[name] = (rng.integers(0, 256, shape) * w * rng.choice([0, 1, 1], shape)).astype(np.uint32)
    return out


def mesh_cases():
    """name -> dict(cells, lo, min_weight, color): map_tsdf_cases' mesh cases, each with a colour volume.  The 256 patterns put
    the one-sided gradients into play (weight-0 cells between the cubes), the sphere the two-sided one, the boxes 47 x 47 x 2 and
    2 x 2 x 3 have an axis of 2, the line of 300 cells spans two blocks."""
    base = tc.mesh_cases()
    rng = np.random.default_rng(27)  # weights 2 .. 5 against min_weight 0, 1 and 3: cells that count at one and not at another
    dense = tc.volume(rng.integers(-50, 50, (4, 5, 6)), rng.integers(2, 6, (4, 5, 6)))
    for mw in (0, 1, 3):
        base["weights 2 .. 5, min_weight %d" % mw] = dict(cells=dense, lo=(-2, 0, 9), min_weight=mw)
    return {name: dict(c, color=colour_volume(c["cells"].shape, zlib.crc32(name.encode()))) for name, c in base.items()}


@functools.lru_cache(maxsize=None)
def mesh_spec(name):
    """(vertices, triangles, info, normals, colours) of a case from the per-vertex loop, computed once."""
    c = mesh_cases()[name]
    return sf.mesh_attr(c["cells"], c["color"], c["lo"], V, c["min_weight"])


def wall_image(colour=(17, 130, 251)):
    """A constant-colour image for map_tsdf_cases.wall()."""
    return np.broadcast_to(np.array(colour, np.uint8), (12, 16, 3)).copy()


assert tr.CELL == tc.CELL
