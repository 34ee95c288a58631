"""numpy restatement of the voxel map's contract (include/revo_hip.h revo_map_*), bit for bit.

Input points: the level-0 points of generateColoredPcl(0, dense) -- X, Y, Z and the colour bytes (the cloud's colours are the
correctly rounded c / 255, so rint(colour * 255) gives the byte back).  Per point, float32 with every operation rounded on
its own: pw[i] = ((R[i,0] X + R[i,1] Y) + R[i,2] Z) + t[i]; key k = floor(pw / v); q = rint(pw * 2^20) as int64.  Dropped:
some |pw| >= 2048, some key outside [-2^20, 2^20 - 1], some pw not finite.  Per voxel: count, sum q, sum of each colour byte.
Extraction in ascending packed-key order: xyz = float32(float64(sum q) / float64(count) * 2^-20), colour = (sum + count // 2)
// count."""
import numpy as np

F = np.float32
KEY_BIAS = 1 << 20
KEY_MIN, KEY_MAX = -(1 << 20), (1 << 20) - 1
RANGE_M = 2048.0
FIX = F(1 << 20)


def points_from_pcl(pcl8):
    """generateColoredPcl rows (X,Y,Z,1,r,g,b,1) -> (xyz N x 3 float32, rgb N x 3 uint8 as R,G,B)."""
    pcl8 = np.asarray(pcl8, np.float32).reshape(-1, 8)
    rgb = np.rint(pcl8[:, 4:7].astype(np.float64) * 255.0).astype(np.uint8)
    return np.ascontiguousarray(pcl8[:, :3]), rgb


def select_points(depth, edges, bgr, fx, fy, cx, cy, dmin, dmax, dense):
    """The selection and back-projection of generateColoredPcl at level 0 (k_pcl_walk): dense or edge pixel, finite depth in
    (dmin, dmax); X = Z (x - cx) / fx, Y = Z (y - cy) / fy.  -> (xyz, rgb as R,G,B)."""
    depth = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(depth) & (depth > F(dmin)) & (depth < F(dmax))
    if not dense:
        ok &= np.asarray(edges) != 0
    y, x = np.nonzero(ok)
    Z = depth[y, x]
    X = (Z * (x.astype(F) - F(cx))) / F(fx)
    Y = (Z * (y.astype(F) - F(cy))) / F(fy)
    px = np.asarray(bgr, np.uint8)[y, x]
    return np.stack([X, Y, Z], 1).astype(F), px[:, ::-1].copy()


def world_points(xyz, T):
    """pw = ((R0 X + R1 Y) + R2 Z) + t in float32, each operation rounded (T: 4x4 keyframe -> world)."""
    T = np.asarray(T, np.float32)
    X, Y, Z = (np.asarray(xyz, F)[:, i] for i in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((T[i, 0] * X + T[i, 1] * Y) + T[i, 2] * Z) + T[i, 3] for i in range(3)], 1).astype(F)


def keys_and_fixed(pw, voxel):
    """-> (ok mask, keys N x 3 int64, q N x 3 int64) of world points."""
    pw = np.asarray(pw, F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        f = np.floor(pw / F(voxel))
        ok = np.all(np.abs(pw) < F(RANGE_M), 1) & np.all((f >= KEY_MIN) & (f <= KEY_MAX), 1)
        k = np.where(ok[:, None], f, 0).astype(np.int64)
        q = np.where(ok[:, None], np.rint(pw * FIX), 0).astype(np.int64)
    return ok, k, q


def pack_keys(k):
    k = np.asarray(k, np.int64) + KEY_BIAS
    return ((k[:, 0].astype(np.uint64) << np.uint64(42)) | (k[:, 1].astype(np.uint64) << np.uint64(21)) | k[:, 2].astype(np.uint64))


def mean_position(sq, cnt):
    """float32(float64(sum q) / float64(count) * 2^-20)."""
    return ((np.asarray(sq, np.int64).astype(np.float64) / np.asarray(cnt, np.float64)[..., None]) * 2.0 ** -20).astype(F)


def mean_colour(sc, cnt):
    cnt = np.asarray(cnt, np.int64)[..., None]
    return ((np.asarray(sc, np.int64) + cnt // 2) // cnt).astype(np.uint8)


class VoxelMapRef:
    def __init__(self, voxel):
        self.voxel = F(voxel)
        self.keys, self.q, self.rgb = [], [], []
        self.points_integrated = 0
        self.points_dropped = 0
        self.keyframes = 0

    def integrate(self, xyz, rgb, T):
        pw = world_points(xyz, T)
        ok, k, q = keys_and_fixed(pw, self.voxel)
        self.keys.append(pack_keys(k[ok]))
        self.q.append(q[ok])
        self.rgb.append(np.asarray(rgb, np.int64)[ok])
        self.points_integrated += int(ok.sum())
        self.points_dropped += int((~ok).sum())
        self.keyframes += 1

    def integrate_pcl(self, pcl8, T):
        self.integrate(*points_from_pcl(pcl8), T)

    def voxels(self):
        keys = np.concatenate(self.keys) if self.keys else np.zeros(0, np.uint64)
        return len(np.unique(keys))

    def points(self, min_count=1):
        """(xyz N x 3 float32, rgb N x 3 uint8, count N uint32) in ascending key order."""
        if not self.keys:
            return np.zeros((0, 3), F), np.zeros((0, 3), np.uint8), np.zeros(0, np.uint32)
        keys = np.concatenate(self.keys)
        uk, inv = np.unique(keys, return_inverse=True)
        cnt = np.bincount(inv, minlength=len(uk)).astype(np.int64)
        sq = np.zeros((len(uk), 3), np.int64)
        sc = np.zeros((len(uk), 3), np.int64)
        np.add.at(sq, inv, np.concatenate(self.q))
        np.add.at(sc, inv, np.concatenate(self.rgb))
        sel = cnt >= max(1, int(min_count))
        return mean_position(sq[sel], cnt[sel]), mean_colour(sc[sel], cnt[sel]), cnt[sel].astype(np.uint32)
