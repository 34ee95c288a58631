"""Hand-made distance fields, point sets and poses shared by the distance-field registration tests (test_map_df_align_cpu.py,
test_gpu_map_df_align.py).  Test infrastructure only."""
import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
V = 2.0 ** -5  # a power of two: cell coordinates times V are exact, so a point can be put ON a cell boundary


def field_of(n, solids, clamp=0):
    """The exact squared distance, in cells, from every cell of an n0 x n1 x n2 box to the nearest of `solids` (cell index
    triples inside the box), by brute force; all NONE without a solid; clamp > 0: min(value, clamp)."""
    n = tuple(int(x) for x in n)
    if not len(solids):
        return np.full(n, NONE, np.uint32)
    g = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1).astype(np.int64)
    d = np.min(((g[:, :, :, None, :] - np.asarray(solids, np.int64)[None, None, None]) ** 2).sum(-1), -1).astype(np.uint32)
    return np.minimum(d, np.uint32(clamp)) if clamp else d


def random_solids(n, count, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, k, count) for k in n], 1)


def cell_points(lo, cells, voxel=V):
    """Points at fractional cell coordinates (cell centres are the integers): p = (lo + cell + 0.5) * voxel per axis."""
    return ((np.asarray(lo, np.float64) + np.asarray(cells, np.float64) + 0.5) * float(voxel)).astype(F).reshape(-1, 3)


def random_points(lo, n, count, seed, voxel=V, margin=1.5):
    """Points spread over the interpolation cells of the box and `margin` cells around them."""
    rng = np.random.default_rng(seed)
    return cell_points(lo, rng.uniform(-margin, np.asarray(n) - 1 + margin, (count, 3)), voxel)


def rim_cells(n):
    """Per axis, fractional cell coordinates at a = 0 and a = n - 2 (inside, on the boundary and just inside the far end) and
    one cell further on each side (skipped); the other two coordinates well inside."""
    n = np.asarray(n)
    mid = (n - 1) / 2.0 + 0.25
    out = []
    for i in range(3):
        for x in (0.0, 0.25, n[i] - 2.0, n[i] - 1.25, -1.0, -0.25, n[i] - 1.0, n[i] - 0.5, -2 ** -20, n[i] - 1.0 - 2 ** -12):
            c = mid.copy()
            c[i] = x
            out.append(c)
    return np.array(out)


ODD_POINTS = np.array([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (3e38, 0, 0), (-3e38, 3e38, 0), (np.nan, np.nan, np.nan)], F)


def se3(x):
    """expm(hat(x)) for x = (v, w), float64."""
    from revo_amd import synth
    return synth.se3_exp(np.asarray(x, np.float64))


def poses(count, seed, scale=1.0):
    """`count` small rigid motions (4x4 float32): the first is the identity."""
    rng = np.random.default_rng(seed)
    out = [np.eye(4, dtype=F)]
    for _ in range(count - 1):
        out.append(se3(np.concatenate([rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.08, 0.08, 3)]) * scale).astype(F))
    return out


def bad_poses():
    skew, nan, flip = np.eye(4, dtype=F), np.eye(4, dtype=F), np.eye(4, dtype=F)
    skew[0, 1] = 0.01
    nan[1, 3] = np.nan
    flip[2, 2] = -1.0  # orthogonal with det -1
    return skew, nan, flip


def base():
    """A 9 x 7 x 11 box with a negative lo and a dozen solids: (d2, lo, n)."""
    n, lo = (9, 7, 11), (-4, -3, 2)
    return field_of(n, random_solids(n, 12, 5)), lo, n


def blob(n=(40, 36, 32), lo=(-20, -18, 6), seed=9):
    """A field whose solids are the surface of three bumps on a floor, for the loop: a cloud sampled from the same surface
    registers against it.  -> (d2, lo, n, the solids' cell indices)."""
    g = np.stack(np.meshgrid(np.arange(n[0]), np.arange(n[1]), indexing="ij"), -1).astype(np.float64)
    z = 8 + 6 * np.exp(-((g[..., 0] - 12) ** 2 + (g[..., 1] - 10) ** 2) / 30.0) + 5 * np.exp(-((g[..., 0] - 28) ** 2 + (g[..., 1] - 22) ** 2) / 50.0) \
        + 4 * np.exp(-((g[..., 0] - 10) ** 2 + (g[..., 1] - 27) ** 2) / 20.0) + 0.08 * g[..., 0]
    zi = np.rint(z).astype(np.int64)
    ij = np.argwhere((g[..., 0] >= 4) & (g[..., 0] < n[0] - 4) & (g[..., 1] >= 4) & (g[..., 1] < n[1] - 4))
    solids = np.array([(i, j, zi[i, j]) for i, j in ij], np.int64)
    # a field by the three min-plus passes is what the library builds; here any exact field will do: brute force in chunks
    d2 = np.empty(n, np.uint32)
    cells = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    for a in range(0, len(cells), 4096):
        c = cells[a:a + 4096]
        d2.reshape(-1)[a:a + 4096] = ((c[:, None, :] - solids[None]) ** 2).sum(-1).min(1)
    return d2, lo, n, solids
