"""The cases shared by the surface tracking tests (test_map_tsdf_track_cpu.py, test_gpu_map_tsdf_track.py), on map_tsdf_cases'
geometry: voxel edge 1/8 m and a 16 x 12 camera at the origin looking down +z.  The lattice camera KL has fx = fy = 8: with a depth
of exactly 1 m and the pose LATTICE (a shift of 1/16 m along z) pixel (x, y) lands exactly on the centre of the cell (x - 8, y - 6, 8)
-- every product, quotient and sum on the way is exact in float32 --, so r = 0 on every axis, F is that cell's own field and a case
decides what the rule sees.  Each case is one call: the smallest shape at which its rule can go wrong.  Test infrastructure only."""
import functools

import numpy as np

import map_carve_cases as cc
import map_seen_cases as sc
import map_tsdf_cases as tc
import map_tsdf_ray_cases as rc
import map_tsdf_ref as tfr
import map_tsdf_track_ref as kr

F = np.float32
V, I4 = tc.V, sc.I4
ZMIN, ZMAX = sc.ZMIN, sc.ZMAX
ZR = (ZMIN, ZMAX)
KC = sc.KC[:4]                  # the 16 x 12 camera of the plane (fx = 8.5)
KL = (8.0, 8.0, 7.5, 5.5)       # the lattice camera
LATTICE = rc.at(I4, 0.0, 0.0, 1.0 / 16.0)
LO, N = sc.LO, sc.N             # (-4, -3, 6), (9, 7, 5): the lattice plane is iz = 2; pixels 4 .. 12 x 3 .. 9 land on its cells
TRUNC = 0.5                     # kq = 2^-11: e = F * 2^-11 exactly; the default gate is 0.25 = 512 units
QUANTUM = F(TRUNC) / F(1024)

# The convergence of the contract (test_map_tsdf_track_cpu.test_convergence_on_the_scene_box), measured with mapfile.tsdf_track on the
# CPU on 2026-10-20 at stride 1 (about 3100 of the 76800 pixels fall on the box's surface): the largest end error over the 27 starts --
# the camera's displacement in metres, the angle in radians, and the RMS displacement of the box's corners (box_distance) in metres.
# 24 of the starts end at one pose, 8.24e-3 m and 4.30e-3 rad from the truth (box 5.0e-3 m): the zero of the model fused from four
# noisy views, not the truth's.  The test asserts twice these.
SCENE_END_ERR_T, SCENE_END_ERR_R, SCENE_END_BOX = 1.65e-2, 6.60e-3, 1.29e-2
SCENE_STRIDE = 1


def ones(n, value=100):
    return tc.volume(np.full(n, value, np.int64), np.ones(n, np.int64))


def flat(depth=1.0, size=(16, 12)):
    return np.full((size[1], size[0]), depth, F)


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    R = np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def about(T, centre, axis, deg):
    """T turned by deg about the axis through `centre` (world frame) -> float32."""
    C0, C1 = np.eye(4), np.eye(4)
    C0[:3, 3], C1[:3, 3] = np.asarray(centre, np.float64), -np.asarray(centre, np.float64)
    return (C0 @ rot(axis, deg) @ C1 @ np.asarray(T, np.float64)).astype(F)


def gate_volume():
    """Every cell valid; the lattice plane iz = 2 holds, by (i + j) % 6: 512 (|e| == max_dist: accepted), 513 (one quantum above: gated),
    -512, -513, 1024 (saturated: gated), 0 (e == 0)."""
    s = np.full(N, 300, np.int64)
    i, j = np.meshgrid(np.arange(N[0]), np.arange(N[1]), indexing="ij")
    s[:, :, 2] = np.array([512, 513, -512, -513, 1024, 0])[(i + j) % 6]
    return tc.volume(s, np.ones(N, np.int64))


def bad_depths():
    """The lattice image with a hole of every kind in the pixels that land in the box."""
    D = flat()
    for x, d in zip(range(4, 12), (np.nan, np.inf, -np.inf, 0.0, ZMIN, ZMAX, -1.0, sc.up(ZMAX))):
        D[4, x] = d
    D[5, 5], D[5, 6] = sc.up(ZMIN), sc.down(ZMAX)   # usable, but far from the box
    return D


def sized(size, seed):
    """A depth image of the given size over the tilted plane's box, with holes, and its camera: the 16 x 12 camera scaled."""
    w, h = size
    rng = np.random.default_rng(seed)
    D = (1.3 + 0.6 * rng.random((h, w))).astype(F)
    D[rng.random((h, w)) < 0.1] = 0.0
    k = (8.5 * w / 16.0, 8.5 * w / 16.0, (w - 1) / 2.0, (h - 1) / 2.0)
    return D, k


def sphere_depth(k=KC, size=(16, 12), centre=(0.0, 0.0, 1.25), radius=4.2 * V):
    """The depth image of map_tsdf_cases' sphere (12^3 cells at lo (-6, -6, 4)) seen from the origin: the ray through every pixel met
    with the ball, in float64, rounded; 0 where it misses."""
    w, h = size
    fx, fy, cx, cy = k
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones((h, w))], -1)
    c = np.asarray(centre)
    a, b, cc_ = (d * d).sum(-1), (d * c).sum(-1), c @ c - radius * radius
    disc = b * b - a * cc_
    z = (b - np.sqrt(np.maximum(disc, 0))) / a
    return np.where(disc > 0, z, 0.0).astype(F)


SPHERE_TRUNC = 1024 * V / 1000.0   # the sphere's sums are (d - r) * 1000 in cells: with this trunc e is (d - r) * V metres


@functools.lru_cache(maxsize=None)
def wall():
    """map_tsdf_cases' wall fused from one view -> (cells, lo, trunc, the view's depth image)."""
    w = tc.wall()
    cells = tfr.fuse(V, w["lo"], w["n"], w["views"], w["trunc"])[0]
    return cells, w["lo"], float(F(4) * F(V)), w["views"][0][0]


@functools.lru_cache(maxsize=None)
def scene():
    """The 64^3 box of DESIGN 19's scene fused from its four views (revo_amd.mapfile's volume, which test_map_tsdf_cpu.py pins to the
    per-cell loop) -> (cells, lo, trunc, views)."""
    from revo_amd import mapfile
    lo, n, views = tc.scene64()
    cells = mapfile.tsdf_records(cc.VOXEL, lo, n, views)[0]
    return cells, tuple(int(x) for x in lo), float(F(4) * F(cc.VOXEL)), views


def scene_centre():
    cells, lo, _, _ = scene()
    return ((np.asarray(lo, np.float64) + np.asarray(cells.shape) / 2.0) * float(F(cc.VOXEL))).astype(F)


def scene_starts():
    """name -> (start pose, truth) of the convergence table: the truth of view 0 moved by 0.5, 1, 2 voxel edges along each axis, turned
    by 0.5, 1, 2 degrees about each axis through the box's middle, and both at once."""
    truth = np.asarray(scene()[3][0][1], F)
    c = scene_centre()
    out = {}
    for lvl, (k, deg) in enumerate(((0.5, 0.5), (1.0, 1.0), (2.0, 2.0))):
        for axis in range(3):
            t = np.array(truth, np.float64)
            t[axis, 3] += k * cc.VOXEL
            out["t%d %s" % (lvl, "xyz"[axis])] = t.astype(F)
            out["r%d %s" % (lvl, "xyz"[axis])] = about(truth, c, axis, deg)
            both = about(truth, c, axis, -deg).astype(np.float64)
            both[(axis + 1) % 3, 3] -= k * cc.VOXEL
            out["tr%d %s" % (lvl, "xyz"[axis])] = both.astype(F)
    return out, truth


def box_distance(T, truth, lo, n, voxel):
    """How far the pose T puts the box from where the truth has it: the frame's camera coordinates of the box's eight corners (by the
    truth) carried into the world by T, against the corners themselves; the RMS distance in metres.  One number for translation
    and rotation together, taken where the model is."""
    lo, n = np.asarray(lo, np.float64), np.asarray(n, np.float64)
    corners = np.array([[(lo[a] + (n[a] if (i >> a) & 1 else 0.0)) * float(F(voxel)) for a in range(3)] for i in range(8)])
    Ti, T = np.linalg.inv(np.asarray(truth, np.float64)), np.asarray(T, np.float64)
    pc = corners @ Ti[:3, :3].T + Ti[:3, 3]
    return float(np.sqrt((((pc @ T[:3, :3].T + T[:3, 3]) - corners) ** 2).sum(1).mean()))


def pose_error(T, truth):
    """(metres, radians) between two poses."""
    D = np.linalg.inv(np.asarray(truth, np.float64)) @ np.asarray(T, np.float64)
    return float(np.linalg.norm(D[:3, 3])), float(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))


def _case(cells, lo, depth, camera, poses, kind, voxel=V, trunc=TRUNC, zrange=ZR, **prm):
    poses = np.asarray(poses, F).reshape(-1, 4, 4)
    return dict(cells=cells, lo=tuple(int(x) for x in lo), voxel=voxel, trunc=trunc, depth=np.asarray(depth, F), camera=tuple(float(x) for x in camera),
                zrange=tuple(zrange), poses=poses, kind=kind, max_dist=prm.get("max_dist"), stride=prm.get("stride", 1), min_weight=prm.get("min_weight", 1),
                centre=prm.get("centre"))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(cells, lo, voxel, trunc, depth, camera, zrange, poses, max_dist, stride, min_weight, centre, kind).  kind: what the
    case was built to show -- a tuple of map_tsdf_track_ref.CLASSES that must occur (test_map_tsdf_track_cpu.test_coverage)."""
    c = {}

    def add(name, cells, lo, depth, camera, poses, kind, **kw):
        c[name] = _case(cells, lo, depth, camera, poses, kind, **kw)

    nudged = rc.at(I4, 0.02, -0.01, 0.03)
    # one interpolation cube around the optical axis
    add("2x2x2", rc.layers((2, 2, 2), 2, [100, -100]), (-1, -1, 7), flat(), KC, [I4], ("outside", "accepted"))
    for n in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        add("axis of 1: %dx%dx%d" % n, ones(n), (-2 if n[0] > 1 else 0, -2 if n[1] > 1 else 0, 8 if n[2] == 1 else 6), flat(), KL, [LATTICE, I4], ("outside",))
    add("3x5x7 lo < 0", rc.layers((3, 5, 7), 2, [300, 200, 100, 30, -70, -170, -270], weight=3), (-1, -2, 5), flat(), KC, [nudged], ("outside", "accepted"),
        centre=(0.1, -0.2, 1.0))
    # weights
    hole = rc.layers((5, 5, 6), 2, [100, 100, 100, -100, -100, -100])
    hole["weight"][2, 2, 2] = 0
    add("weight 0 in one corner", hole, (-2, -2, 6), flat(), KL, [LATTICE, nudged], ("invalid_cell", "accepted"))
    rnd = tc.random_volume(29, (6, 5, 7), 4)
    for mw in (0, 1, 3):
        add("min_weight %d" % mw, rnd, (-3, -2, 6), flat(), KC, [nudged], ("invalid_cell",), min_weight=mw, max_dist=TRUNC)
    # residuals, on the lattice: F is the cell's own field
    add("the gate at equality", gate_volume(), LO, flat(), KL, [LATTICE], ("outside", "gated", "accepted"))
    add("the gate given", gate_volume(), LO, flat(), KL, [LATTICE], ("gated", "accepted"), max_dist=float(F(0.25) + QUANTUM))
    add("zero sums", rc.layers(N, 2, [100, 100, 0, -100, -100]), LO, flat(), KL, [LATTICE], ("accepted",))
    add("saturated", ones(N, 1024), LO, flat(), KL, [LATTICE, nudged], ("accepted",), max_dist=TRUNC)
    add("saturated and gated", ones(N, -1024), LO, flat(), KL, [LATTICE], ("gated",))
    # depths
    add("depths without a point", gate_volume(), LO, bad_depths(), KL, [LATTICE], ("no_depth", "outside", "accepted"))
    add("the rims", ones(N), LO, flat(), KL, [LATTICE], ("outside", "accepted"), max_dist=TRUNC)
    # strides and image sizes, over the tilted plane of the ray-cast cases
    tilted = rc.cases()["tilted plane 20x20x20"]["cells"]
    for size in ((1, 1), (16, 12), (33, 17), (64, 48)):
        D, k = sized(size, size[0])
        for stride in (1, 2, 3, 8):
            add("%dx%d stride %d" % (size + (stride,)), tilted, (-10, -10, 4), D, k, [nudged], ("no_depth", "gated", "accepted") if size[0] > 1 and stride == 1 else (),
                stride=stride, trunc=1.0, max_dist=0.4)
    # poses
    tilt = about(nudged, (0.0, 0.0, 1.0), 1, 3.0)
    skew = I4.copy()
    skew[0, 1] = 0.01
    nan = I4.copy()
    nan[1, 3] = np.nan
    rng = np.random.default_rng(29)
    many = [about(rc.at(I4, *rng.uniform(-0.05, 0.05, 3)), (0.0, 0.0, 1.0), int(rng.integers(3)), float(rng.uniform(-3, 3))) for _ in range(65)]
    many[7], many[40] = skew, nan
    D16, k16 = sized((16, 12), 5)
    add("2 poses", tilted, (-10, -10, 4), D16, k16, [tilt, nudged], ("accepted",), trunc=1.0, max_dist=0.4)
    add("a pose that is no rotation, a pose that is not finite", tilted, (-10, -10, 4), D16, k16, [skew, tilt, nan], ("accepted",), trunc=1.0, max_dist=0.4)
    add("65 poses", tilted, (-10, -10, 4), D16, k16, many, ("accepted",), trunc=1.0, max_dist=0.4, stride=2)
    # scenes
    cells, lo, trunc, D = wall()
    add("wall", cells, lo, D, KC, [I4, rc.at(I4, 0.0, 0.0, 0.04)], ("accepted",), trunc=trunc)
    add("sphere", tc.sphere(), (-6, -6, 4), sphere_depth(), KC, [I4, about(rc.at(I4, 0.01, 0.0, -0.02), (0, 0, 1.25), 0, 2.0)], ("no_depth", "accepted"),
        trunc=SPHERE_TRUNC, centre=(0.0, 0.0, 1.25))
    cells, lo, trunc, views = scene()
    k = cc.intrinsics320()
    add("scene 64^3", cells, lo, views[0][0], k[:4], [views[0][1], scene_starts()[0]["tr1 y"]], ("no_depth", "outside", "invalid_cell", "accepted"), voxel=cc.VOXEL, trunc=trunc,
        zrange=k[4:], stride=8, centre=scene_centre())
    return c


@functools.lru_cache(maxsize=None)
def spec(name):
    """The loop's result of a case, computed once: (records, per-pose class maps)."""
    return kr.track_eval(*args(cases()[name])[0], **args(cases()[name])[1])


def args(c):
    """A case as mapfile.tsdf_track_records and map_tsdf_track_ref.track_eval take it."""
    return (c["cells"], c["lo"], c["voxel"], c["trunc"], c["depth"], c["camera"], c["zrange"], c["poses"]), \
        dict(max_dist=c["max_dist"], stride=c["stride"], min_weight=c["min_weight"], centre=c["centre"])
