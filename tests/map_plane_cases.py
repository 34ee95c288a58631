"""Hand-made voxel maps and scenes shared by the point-to-plane tests (test_map_plane_cpu.py, test_gpu_map_plane.py): records with
means on the 2^-20 m grid, so a voxel's point is exactly what the row says.  Test infrastructure only."""
import numpy as np

import map_records_ref as mrr
import voxel_map_ref as ref

F = np.float32
VOXEL = 0.02
B = 0.5 + 2.0 ** -7          # 0.5078125: in voxel 25 of the 0.02 m grid
S = 2.0 ** -6 + 2.0 ** -8    # 0.01953125: B - S lies in voxel 24, B + S in voxel 26


def records(rows):
    """Rows of (index triple, mean point, count) -> records (map_records_ref.DTYPE) in ascending key order."""
    rec = np.zeros(len(rows), mrr.DTYPE)
    for r, (k, p, n) in zip(rec, rows):
        r["key"] = ref.pack_keys(np.array([k], np.int64))[0]
        q = np.asarray(p, np.float64) * 2.0 ** 20
        assert np.all(q == np.rint(q))  # on the 2^-20 m grid: the voxel's mean is exactly p
        r["count"], r["sum_q"], r["sum_bgr"] = n, (q * n).astype(np.int64), (10 * n, 20 * n, 30 * n)
    return rec[np.argsort(rec["key"])]


def patch(tilt=(0.0, 0.0), count=1):
    """3 x 3 voxels in the z-layer 25 around (25, 25, 25); z = B + tilt . (i - 25, j - 25)."""
    return [((i, j, 25), (B + (i - 25) * S, B + (j - 25) * S, B + tilt[0] * (i - 25) + tilt[1] * (j - 25)), count)
            for i in (24, 25, 26) for j in (24, 25, 26)]


TILT = (2.0 ** -8, 2.0 ** -9)  # the tilted patch stays inside layer 25: |dz| <= 3 * 2^-9 < 0.006


def three_patches():
    """Three flat 3 x 3 patches with the normals z, y and x, ten voxels apart: with min_neighbours = 3 every voxel has a valid
    normal, and together the planes fix all six degrees of freedom."""
    rows = []
    for axis, centre in ((2, (25, 25, 25)), (1, (35, 25, 35)), (0, (25, 35, 45))):
        for a in (-1, 0, 1):
            for b in (-1, 0, 1):
                off = [a, b]
                off.insert(axis, 0)
                k = tuple(c + o for c, o in zip(centre, off))
                rows.append((k, tuple(B + (i - 25) * S for i in k), 1))
    return rows


def line():
    return [((i, 25, 25), (B + (i - 25) * S, B, B), 1) for i in (24, 25, 26)]


def block():
    return [((i, j, k), (B + (i - 25) * S, B + (j - 25) * S, B + (k - 25) * S), 1)
            for i in (24, 25, 26) for j in (24, 25, 26) for k in (24, 25, 26)]


def plane_grid(n=20, shift=(0.0, 0.0, 0.0)):
    """n x n voxels of one z-layer, a single plane: point-to-plane registration against it is rank-deficient."""
    return [((25 + i, 25 + j, 25), (B + i * S + shift[0], B + j * S + shift[1], B + shift[2]), 1) for i in range(n) for j in range(n)]


def last_index():
    """A 3 x 3 patch whose x indices end at 2^20 - 1 (voxel 2^-9 m): the neighbours at 2^20 are out of key range."""
    v = 2.0 ** -9
    top = (1 << 20) - 1
    return [((top - a, j, 0), ((top - a) * v + v / 2, j * v + v / 2, v / 2), 1) for a in (0, 1, 2) for j in (0, 1, 2)]


def sheet(seed, n=20000, offset=(0.0, 0.0, 0.0)):
    """A bumpy sheet with a step in it (test_map_align_cpu's cloud, denser): points (keyframe frame) and colours."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-0.6, 0.6, n), rng.uniform(-0.5, 0.5, n)
    z = 1.5 + 0.15 * np.sin(4 * x) * np.cos(3 * y) + 0.2 * (x > 0.1) + 0.25 * y
    xyz = (np.stack([x, y, z], 1) + np.asarray(offset)).astype(F)
    return xyz, rng.integers(0, 256, (n, 3)).astype(np.uint8)


def sheet_records(voxel, poses, seeds=(1, 2)):
    r = ref.VoxelMapRef(voxel)
    for sd, T in zip(seeds, poses):
        r.integrate(*sheet(sd), T)
    return mrr.records_of(r)


def dense_scene_records(voxel, D=None, seeds=(902, 903)):
    """The dense 320x240 synthetic scene of DESIGN 16 without a GPU: the level-0 clouds of the seeds' reference frames
    (voxel_map_ref.select_points, dense) at the twists 0 and (0.05, 0.01, 0, 0, 0.03, 0), moved by D."""
    from revo_amd import synth
    from revo_amd.settings import ImgPyramidSettings
    s = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
    D = np.eye(4) if D is None else D
    r = ref.VoxelMapRef(voxel)
    for i, sd in enumerate(seeds):
        bgr, depth = synth.make_pair(sd, s)["ref"]
        xyz, rgb = ref.select_points(depth, None, bgr, s.fx, s.fy, s.cx, s.cy, s.depth_min, s.depth_max, True)
        T = synth.se3_exp(np.array([0.05 * i, 0.01 * i, 0, 0, 0.03 * i, 0]))
        r.integrate(xyz, rgb, (D @ T).astype(F))
    return mrr.records_of(r)


def normals_double(rec, min_count=1, min_neighbours=5, planarity=0.1, min_spread=0.1):
    """The normals in double by numpy.linalg.eigh of the centred covariance of the same neighbour points: (normal, valid)."""
    import map_align_ref as mar
    import map_plane_ref as mpr
    keys, m = mar.points_of(rec, min_count)
    k = mar.unpack_keys(keys)
    m = m.astype(np.float64)
    n = len(keys)
    s1, s2, nb = np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros(n)
    for off in mpr.OFFSETS:
        hit, j, _ = mpr._lookup(keys, k, off)
        d = np.where(hit[:, None], m[j] - m, 0.0)
        s1 += d
        s2 += d[:, :, None] * d[:, None, :]
        nb += hit
    Cm = s2 - s1[:, :, None] * s1[:, None, :] / nb[:, None, None]
    w, V = np.linalg.eigh(Cm)
    valid = (nb >= min_neighbours) & (w[:, 1] > 0) & (w[:, 0] <= planarity * w[:, 1]) & (w[:, 1] >= min_spread * w[:, 2])
    return V[:, :, 0], valid
