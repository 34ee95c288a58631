"""The view contract of the voxel map (revo_map_render) without a GPU: the C ABI's declaration, export and struct
layout, the properties of the numpy restatement (tests/map_render_ref.py), and the plane condition that fixes the footprint
rule.  The device is checked against the restatement in tests/test_gpu_map_render.py."""
import ctypes as C
import re

import numpy as np

import map_render_ref as mr
import voxel_map_ref as ref
from revo_amd import _lib
from revo_amd.settings import ImgPyramidSettings, MapView

F = np.float32
I4 = np.eye(4, dtype=np.float32)
S640 = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))


def test_header_declares_and_library_exports_render():
    assert "revo_map_render" in _lib.declared_symbols()
    L = _lib.lib()
    assert hasattr(L, "revo_map_render")
    assert all(hasattr(L, s) for s in _lib.declared_symbols() if s.startswith("revo_map_"))


def test_map_view_mirrors_the_header_struct():
    txt = open(_lib.HEADER).read()
    body = re.search(r"typedef struct revo_map_view \{(.*?)\} revo_map_view;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        t, names = decl.split(None, 1)
        for name in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", name.strip())
            fields.append((m.group(1), ctype[t] * int(m.group(2)) if m.group(2) else ctype[t]))

    class Header(C.Structure):
        _fields_ = fields

    assert [n for n, _ in fields] == [n for n, _ in MapView._fields_]
    assert C.sizeof(Header) == C.sizeof(MapView) == 104
    for n, _ in fields:
        assert getattr(Header, n).offset == getattr(MapView, n).offset, n
        assert getattr(Header, n).size == getattr(MapView, n).size, n


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(0.3, 4.0, n)], 1).astype(F)
    return xyz, rng.integers(0, 256, (n, 3)).astype(np.uint8)


def _bytes(out):
    return out[0].tobytes() + out[1].tobytes() + bytes([out[2] & 255])


def test_a_permutation_of_the_voxels_gives_identical_bytes():
    xyz, rgb = _cloud(20000, 1)
    T = I4.copy()
    T[:3, 3] = [0.1, -0.05, 0.2]
    for splat in (0, 4):
        v = mr.view_of(S640, T, splat)
        a = mr.render(xyz, rgb, 0.02, v)
        for seed in (2, 3):
            p = np.random.default_rng(seed).permutation(len(xyz))
            b = mr.render(xyz[p], rgb[p], 0.02, v)
            assert a[2] == b[2] > 0 and _bytes(a) == _bytes(b)


def test_splat_zero_writes_at_most_one_pixel_per_voxel():
    xyz, rgb = _cloud(500, 4)
    v = mr.view_of(S640, I4, 0)
    _, _, covered = mr.render(xyz, rgb, 0.05, v)
    assert 0 < covered <= len(xyz)
    one = mr.render(xyz[:1], rgb[:1], 0.05, v)
    assert one[2] <= 1
    wide = mr.render(xyz[:1], rgb[:1], 0.05, mr.view_of(S640, I4, 4))
    assert wide[2] > one[2] or one[2] == 0


def test_a_view_turned_away_is_empty():
    xyz, rgb = _cloud(5000, 5)
    T = I4.copy()
    T[:3, :3] = np.diag([-1.0, 1.0, -1.0])  # half a turn about y: the map is behind the camera
    depth, bgr, covered = mr.render(xyz, rgb, 0.02, mr.view_of(S640, T, 4))
    assert covered == 0 and not depth.any() and not bgr.any()


def test_nearer_hides_farther_and_equal_depth_takes_the_smaller_colour_word():
    v = mr.view_of(S640, I4, 0)
    xyz = np.array([[0, 0, 2.0], [0, 0, 1.0], [0, 0, 3.0]], F)  # all on the optical axis: one pixel
    rgb = np.array([[10, 20, 30], [200, 100, 50], [1, 2, 3]], np.uint8)
    depth, bgr, covered = mr.render(xyz, rgb, 0.01, v)
    iu, iv = int(np.floor(v.cx)), int(np.floor(v.cy))
    assert covered == 1 and depth[iv, iu] == F(1.0) and bgr[iv, iu].tolist() == [50, 100, 200]
    xyz = np.array([[0, 0, 1.5]] * 3, F)
    rgb = np.array([[9, 0, 255], [8, 255, 255], [9, 0, 0]], np.uint8)  # words 0x0900ff, 0x08ffff, 0x090000
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        depth, bgr, covered = mr.render(xyz[order], rgb[order], 0.01, v)
        assert covered == 1 and depth[iv, iu] == F(1.5) and bgr[iv, iu].tolist() == [255, 255, 8]


def test_world_to_camera_rounds_every_operation():
    T = np.array([[0.36, 0.48, -0.8, 0.3], [-0.8, 0.6, 0.0, -1.1], [0.48, 0.64, 0.6, 2.2], [0, 0, 0, 1]], F)
    Rc, tc = mr.world_to_camera(T)
    assert np.array_equal(Rc, T[:3, :3].T)
    for i in range(3):
        a, b, c = F(Rc[i, 0] * T[0, 3]), F(Rc[i, 1] * T[1, 3]), F(Rc[i, 2] * T[2, 3])
        assert tc[i] == -F(F(a + b) + c)


def test_constant_depth_plane_is_fully_covered_at_its_own_pose():
    """The condition behind ru = ceil(0.5 v f / z): the dense points of a 640x480 frame at Z0 = 1 m, fused at the identity into
    1 cm voxels (ceil(0.5 * 0.01 * 517.3 / 1) = 3 <= splat_max = 4) and rendered at the identity with the same camera, cover
    every pixel that contributed a point, at a depth within 2^-20 m of Z0: every voxel's mean has z = Z0 and projects to the
    centroid of its pixel span, and the footprint reaches at least half that span to either side."""
    s = S640
    rng = np.random.default_rng(6)
    depth = np.full((s.height, s.width), 1.0, F)
    bgr = rng.integers(0, 256, (s.height, s.width, 3)).astype(np.uint8)
    xyz, rgb = ref.select_points(depth, None, bgr, s.fx, s.fy, s.cx, s.cy, s.depth_min, s.depth_max, True)
    assert len(xyz) == s.width * s.height
    m = ref.VoxelMapRef(0.01)
    m.integrate(xyz, rgb, I4)
    assert m.points_dropped == 0
    pxyz, prgb, _ = m.points()
    assert int(np.ceil(F(0.5) * F(0.01) * F(s.fx) / F(1.0))) == 3
    d, _, covered = mr.render(pxyz, prgb, 0.01, mr.view_of(s, I4, 4))
    assert covered == s.width * s.height, "uncovered pixels: %d" % (s.width * s.height - covered)
    assert np.abs(d.astype(np.float64) - 1.0).max() <= 2.0 ** -20
