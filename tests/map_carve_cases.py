"""Hand-made voxels, depth images and the synthetic scene shared by the carving tests (test_map_carve_cpu.py,
test_gpu_map_carve.py).  Voxel means lie on the 2^-20 m grid (or, for the one-float-off cases, a count of 4 or 8
puts the mean one float32 step beside a grid point), and the cameras are chosen so that every projection is exact: what a case
says about z, u and v is what the rule sees.  Test infrastructure only."""
import functools

import numpy as np

import map_plane_cases as plc
import map_records_ref as mrr
import voxel_map_ref as ref

F = np.float32
I4 = np.eye(4, dtype=F)
VOXEL = 0.02
ZMIN, ZMAX = F(0.1), F(5.2)
K16 = (4.0, 4.0, 8.0, 6.0, ZMIN, ZMAX)   # the 16 x 12 camera: pixel iu is at x = (iu - 8) / 4 * z
K8 = (4.0, 4.0, 4.0, 4.0, ZMIN, ZMAX)    # the 8 x 8 camera
K64 = (16.0, 16.0, 32.0, 32.0, ZMIN, ZMAX)
M = 2.0 ** -6                            # the margin of the hand-made cases: exact in float32


def _row(p, n=1, dq=0):
    """A row for map_plane_cases.records-like packing: point p (on the grid), count n, and dq added to the z sum: the mean z is
    then p_z + dq / n * 2^-20."""
    return (np.asarray(p, np.float64), int(n), int(dq))


def pack(rows, voxel=VOXEL):
    """Rows of _row -> (records in ascending key order, the order's permutation).  The key is the voxel of the mean point."""
    rec = np.zeros(len(rows), mrr.DTYPE)
    for r, (p, n, dq) in zip(rec, rows):
        q = p * 2.0 ** 20
        assert np.all(q == np.rint(q))
        sq = (q * n).astype(np.int64)
        sq[2] += dq
        mean = ref.mean_position(sq[None], np.array([n]))[0]
        r["key"] = ref.pack_keys(np.floor(mean / F(voxel)).astype(np.int64)[None])[0]
        r["count"], r["sum_q"], r["sum_bgr"] = n, sq, (10 * n, 20 * n, 30 * n)
    assert len(np.unique(rec["key"])) == len(rec), "two hand-made voxels share a key"
    order = np.argsort(rec["key"])
    return rec[order], order


def at(k, iu, iv, z, du=0.0, dv=0.0):
    """The point that the camera k (identity pose) sees at u = iu + du, v = iv + dv and depth z."""
    fx, fy, cx, cy = k[:4]
    return ((iu + du - cx) / fx * z, (iv + dv - cy) / fy * z, z)


def depth16():
    """The 16 x 12 image of the class cases: 2 m everywhere but for the marked pixels."""
    D = np.full((12, 16), 2.0, F)
    D[3, 4], D[3, 5] = 3.0, 1.5      # the edge case: centre behind, a neighbour nearer
    D[2, 9] = np.nan                 # holes of the three kinds
    D[9, 2] = 0.0
    D[9, 13] = ZMAX
    D[6, 5] = 0.5                    # left of the pixel that u = 5.5 rounds to
    return D


# name -> (row, the class at radius 1 with margin M, margin_rel 0, in the view (depth16(), I4, K16))
def class_cases():
    c = {}
    c["free"] = (_row(at(K16, 7, 9, 1.0)), "free")
    c["confirmed"] = (_row(at(K16, 10, 5, 2.0)), "confirmed")
    c["occluded"] = (_row(at(K16, 12, 3, 3.0)), "occluded")
    c["edge"] = (_row(at(K16, 4, 3, 2.5)), "edge")
    c["unknown_nan"] = (_row(at(K16, 10, 3, 1.0)), "unknown")
    c["unknown_zero"] = (_row(at(K16, 2, 8, 1.0)), "unknown")
    c["unknown_zmax"] = (_row(at(K16, 13, 8, 1.0)), "unknown")
    c["free_boundary"] = (_row(at(K16, 4, 8, 2.0 - M)), "confirmed")           # z == dmin - m is not free; |z - dc| == mc is confirmed
    c["free_one_below"] = (_row(at(K16, 10, 8, 2.0 - M), 8, -1), "free")       # one float32 step (2^-23) nearer
    c["confirmed_boundary"] = (_row(at(K16, 7, 3, 2.0 + M)), "confirmed")      # |z - dc| == mc
    c["occluded_one_above"] = (_row(at(K16, 13, 5, 2.0 + M), 4, 1), "occluded")  # one float32 step (2^-22) farther
    c["border_left"] = (_row(at(K16, 0, 6, 1.0)), "outside")
    c["border_left_in"] = (_row(at(K16, 1, 5, 1.0)), "free")
    c["border_right"] = (_row(at(K16, 15, 6, 1.0)), "outside")
    c["border_right_in"] = (_row(at(K16, 14, 6, 1.0)), "free")
    c["border_top"] = (_row(at(K16, 7, 0, 1.0)), "outside")
    c["border_top_in"] = (_row(at(K16, 7, 1, 1.0)), "free")
    c["border_bottom"] = (_row(at(K16, 8, 11, 1.0)), "outside")
    c["border_bottom_in"] = (_row(at(K16, 8, 10, 1.0)), "free")
    c["off_image"] = (_row(at(K16, 40, 6, 1.0)), "outside")
    c["half_pixel"] = (_row(at(K16, 5, 6, 1.0, du=0.5)), "edge")               # u = 5.5 rounds to pixel 6; the window holds the 0.5 m pixel
    c["behind"] = (_row((0.25, 0.25, -1.0)), "outside")
    c["too_near"] = (_row(at(K16, 8, 6, 0.0625)), "outside")                   # z <= zmin
    c["too_far"] = (_row(at(K16, 8, 6, 6.0)), "outside")                       # z >= zmax
    return c


def class_records():
    """-> (records, {name: index into them}, {name: class at radius 1})."""
    c = class_cases()
    names = list(c)
    rec, order = pack([c[n][0] for n in names])
    where = {names[j]: i for i, j in enumerate(order)}
    return rec, where, {n: c[n][1] for n in names}


def filled_records(n_fill=460, seed=19):
    """The class cases plus voxels scattered through the 16 x 12 view's frustum and around it: about 480 records, which a
    1 024-slot table holds at a load just under 0.5 -- with keys that share slots."""
    rng = np.random.default_rng(seed)
    rows = [r for r, _ in class_cases().values()]
    seen = {tuple(np.floor(np.asarray(r[0]) / VOXEL).astype(int)) for r in rows}
    while len(rows) < len(class_cases()) + n_fill:
        z = rng.integers(1 << 17, 7 << 19) / 2.0 ** 20                      # 0.125 .. 3.5 m
        x, y = (rng.integers(-(1 << 21), 1 << 21, 2) / 2.0 ** 20)           # +-2 m: some outside the image
        cell = tuple(np.floor(np.array([x, y, z]) / VOXEL).astype(int))
        if cell in seen or any(tuple(np.add(cell, d)) in seen for d in ((0, 0, 1), (0, 0, -1))):
            continue
        seen.add(cell)
        rows.append(_row((x, y, z), int(rng.integers(1, 6))))
    return pack(rows)[0]


def map_hash(k):
    """The splitmix64 finaliser the table hashes a key with."""
    k = np.asarray(k, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(30)
        k *= np.uint64(0xbf58476d1ce4e5b9)
        k ^= k >> np.uint64(27)
        k *= np.uint64(0x94d049bb133111eb)
    return k ^ (k >> np.uint64(31))


def three_views():
    """Three views at the identity with different depth images: the `free` cases get one, two or three votes."""
    A = depth16()
    B = A.copy()
    B[8:11, 6:9] = 0.9      # in front of "free" (7, 9)
    C = B.copy()
    C[4:8, 13:16] = 0.9     # in front of "border_right_in" (14, 6) too
    return [(A, I4, K16), (B, I4, K16), (C, I4, K16)]


def free_grid(n, z=1.0):
    """n voxels at depth z, one per pixel of a 64 x 64 view (K64) from pixel (2, 2) on: all free against a 2 m image."""
    assert n <= 60 * 60
    return pack([_row(at(K64, 2 + i % 60, 2 + i // 60, z)) for i in range(n)])[0]


def depth64():
    return np.full((64, 64), 2.0, F)


def random_case(seed, h, w, k, n=300):
    """Random records in front of and behind a random depth image with holes, and a small random pose."""
    from revo_amd import synth
    rng = np.random.default_rng(seed)
    D = rng.choice(np.array([1.0, 1.5, 2.0, 2.0, 2.0, 3.0], F), (h, w))
    D[rng.uniform(size=(h, w)) < 0.05] = rng.choice(np.array([0.0, np.nan, np.inf, 6.0], F))
    r = ref.VoxelMapRef(VOXEL)
    xyz = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(-0.5, 4.0, n)], 1).astype(F)
    r.integrate(xyz, rng.integers(0, 256, (n, 3)).astype(np.uint8), I4)
    T = synth.se3_exp(np.concatenate([rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.03, 0.03, 3)])).astype(F)
    return mrr.records_of(r), (D, T, k)


# ------------------------------------------------------------------------------------------------------------ the scene --
TWISTS = ((0, 0, 0, 0, 0, 0), (0.05, 0.01, 0, 0, 0.03, 0), (-0.08, 0.02, 0.03, 0.01, -0.05, 0), (0.15, -0.03, 0.05, -0.02, 0.08, 0.01))
GHOST_BOX = 3


def settings320():
    from revo_amd.settings import ImgPyramidSettings
    return ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))


def poses():
    from revo_amd import synth
    return [synth.se3_exp(np.asarray(t, np.float64)) for t in TWISTS]


@functools.lru_cache(maxsize=None)
def scene_frames():
    """-> (frames of the scene as built, frames of the changed scene): four (bgr, depth) each.  Scene 902; the changed world
    is the same scene with box 3 moved 100 m away; view i is rendered with noise_seed i, the changed one with 10 + i."""
    from revo_amd import synth
    s = settings320()
    k = (s.width, s.height, s.fx, s.fy, s.cx, s.cy)
    sc, moved = synth.Scene(902), synth.Scene(902)
    moved.box_lo[GHOST_BOX] += 100.0
    moved.box_hi[GHOST_BOX] += 100.0
    P = poses()
    return ([sc.render(P[i], *k, noise_seed=i) for i in range(4)], [moved.render(P[i], *k, noise_seed=10 + i) for i in range(4)])


def intrinsics320():
    s = settings320()
    return (s.fx, s.fy, s.cx, s.cy, s.depth_min, s.depth_max)


def ghost_mask(rec):
    """The voxels whose point lies inside box 3's bounds padded by one voxel."""
    from revo_amd import synth
    sc = synth.Scene(902)
    p = ref.mean_position(rec["sum_q"], rec["count"].astype(np.int64)).reshape(-1, 3)
    return np.all((p >= sc.box_lo[GHOST_BOX] - VOXEL) & (p <= sc.box_hi[GHOST_BOX] + VOXEL), 1)


@functools.lru_cache(maxsize=None)
def scene_records():
    """The dense 0.02 m map of views 0 and 1 of the scene as built, without a GPU."""
    s = settings320()
    P = poses()
    r = ref.VoxelMapRef(VOXEL)
    for i in (0, 1):
        bgr, depth = scene_frames()[0][i]
        xyz, rgb = ref.select_points(depth, None, bgr, s.fx, s.fy, s.cx, s.cy, s.depth_min, s.depth_max, True)
        r.integrate(xyz, rgb, P[i].astype(F))
    return mrr.records_of(r)


def scene_views(changed):
    P, k = poses(), intrinsics320()
    return [(scene_frames()[1 if changed else 0][i][1], P[i].astype(F), k) for i in range(4)]


assert plc.VOXEL == VOXEL
