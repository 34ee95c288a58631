"""numpy restatement of the voxel map's view contract (include/revo_hip.h revo_map_render), bit for bit.

Input: the voxel list revo_map_extract returns (tests/voxel_map_ref.py VoxelMapRef.points(min_count)): xyz float32, colour bytes
R,G,B.  All arithmetic is float32 with every operation rounded on its own.

  Rc = R^T of T_w_c;  tc_i = -(((Rc_i0 tx) + (Rc_i1 ty)) + (Rc_i2 tz))
  pc = ((Rc[:,0] px + Rc[:,1] py) + Rc[:,2] pz) + tc;  skipped unless pc is finite, z > zmin, z < zmax
  u = (fx x) / z + cx, v = (fy y) / z + cy;  skipped unless |u|, |v| < 2^20;  iu = floor(u), iv = floor(v)
  ru = min(splat_max, ceil(((0.5 voxel) fx) / z)), rv with fy (the minimum is taken before the conversion to an integer)
  every pixel of [iu - ru, iu + ru] x [iv - rv, iv + rv] inside the image takes min(word), word = bits(z) << 32 | R << 16 | G << 8 | B
  depth = z of the kept word (0 where none), bgr = its colour (0 where none), covered = pixels with a word."""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
U_LIMIT = F(1 << 20)


class View:
    def __init__(self, width, height, fx, fy, cx, cy, zmin, zmax, T_w_c, splat_max=4):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = F(fx), F(fy), F(cx), F(cy)
        self.zmin, self.zmax = F(zmin), F(zmax)
        self.T = np.asarray(T_w_c, F).reshape(4, 4)
        self.splat_max = int(splat_max)


def view_of(s, T_w_c, splat_max=4):
    """The view revo_map_render takes for all-zero intrinsics: the level-0 camera and depth range of the settings."""
    return View(s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.depth_min, s.depth_max, T_w_c, splat_max)


def world_to_camera(T):
    T = np.asarray(T, F)
    Rc = T[:3, :3].T.copy()
    t = T[:3, 3]
    tc = np.array([-(((Rc[i, 0] * t[0]) + (Rc[i, 1] * t[1])) + (Rc[i, 2] * t[2])) for i in range(3)], F)
    return Rc, tc


def words(xyz, rgb, voxel, view):
    """-> (word uint64 N, iu, iv, ru, rv int64 N) of the voxels that write at all."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    Rc, tc = world_to_camera(view.T)
    px, py, pz = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        pc = [((Rc[i, 0] * px + Rc[i, 1] * py) + Rc[i, 2] * pz) + tc[i] for i in range(3)]
        x, y, z = pc
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z > view.zmin) & (z < view.zmax)
        x, y, z, rgb = x[ok], y[ok], z[ok], rgb[ok]
        u = (view.fx * x) / z + view.cx
        v = (view.fy * y) / z + view.cy
        ok = (np.abs(u) < U_LIMIT) & (np.abs(v) < U_LIMIT)  # NaN / inf fail the comparison
        u, v, z, rgb = u[ok], v[ok], z[ok], rgb[ok]
        iu = np.floor(u).astype(np.int64)
        iv = np.floor(v).astype(np.int64)
        hv = F(0.5) * F(voxel)
        ru = np.minimum(F(view.splat_max), np.ceil((hv * view.fx) / z)).astype(np.int64)
        rv = np.minimum(F(view.splat_max), np.ceil((hv * view.fy) / z)).astype(np.int64)
    c = rgb.astype(np.uint64)
    word = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (c[:, 0] << np.uint64(16)) | (c[:, 1] << np.uint64(8)) | c[:, 2]
    return word, iu, iv, ru, rv


def zbuffer(xyz, rgb, voxel, view):
    w, h = view.width, view.height
    zb = np.full(w * h, EMPTY, np.uint64)
    word, iu, iv, ru, rv = words(xyz, rgb, voxel, view)
    if len(word):
        for dy in range(-int(rv.max()), int(rv.max()) + 1):
            yy = iv + dy
            my = (abs(dy) <= rv) & (yy >= 0) & (yy < h)
            for dx in range(-int(ru.max()), int(ru.max()) + 1):
                xx = iu + dx
                m = my & (abs(dx) <= ru) & (xx >= 0) & (xx < w)
                if m.any():
                    np.minimum.at(zb, yy[m] * w + xx[m], word[m])
    return zb.reshape(h, w)


def resolve(zb):
    hit = zb != EMPTY
    depth = np.where(hit, (zb >> np.uint64(32)).astype(np.uint32).view(F), F(0)).astype(F)
    bgr = np.zeros(zb.shape + (3,), np.uint8)
    for k in range(3):  # B, G, R are bits 0-7, 8-15, 16-23
        bgr[..., k] = np.where(hit, (zb >> np.uint64(8 * k)) & np.uint64(0xFF), 0).astype(np.uint8)
    return depth, bgr, int(hit.sum())


def render(xyz, rgb, voxel, view):
    """-> (depth [h, w] float32, bgr [h, w, 3] uint8, covered)."""
    return resolve(zbuffer(xyz, rgb, voxel, view))
