"""Views of the voxel map on the device (revo_map_render, api.VoxelMap.render): bit for bit the numpy restatement of
tests/map_render_ref.py over the voxels of tests/voxel_map_ref.py; the same bytes whatever the integration order, the table
size, the batching of views, the output side or the process; stream-ordered behind integrations; the map is not changed; the
TUM-layout data set run_tum --map-views writes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import synth  # noqa: E402
from revo_amd.settings import ImgPyramidSettings, MapView  # noqa: E402

import map_render_ref as mr  # noqa: E402
import voxel_map_ref as ref  # noqa: E402

INVALID_ARG = -1
S320 = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
S640 = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
# keyframe poses that overlap (voxels fused from several keyframes, so min_count = 2 selects a real subset)
KF_TWISTS = [[0, 0, 0, 0, 0, 0], [0.05, 0.01, 0.0, 0.0, 0.03, 0.0], [-0.04, 0.02, 0.03, 0.02, -0.02, 0.01],
             [0.02, -0.03, 0.05, -0.01, 0.04, 0.0]]


def _T(tw):
    return synth.se3_exp(np.asarray(tw, np.float64)).astype(np.float32)


KF_POSES = [_T(t) for t in KF_TWISTS]
BETWEEN = _T([0.01, 0.015, 0.01, 0.01, 0.005, 0.005])
AWAY = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], np.float32)  # half a turn about y


def _keyframes(api, s, seeds):
    cam = api.CameraPyr(s)
    return cam, [api.ImgPyramidRGBD(s, cam, *synth.make_pair(sd, s)["ref"]) for sd in seeds]


def _restate(pyrs, Ts, voxel, dense):
    r = ref.VoxelMapRef(voxel)
    for p, T in zip(pyrs, Ts):
        r.integrate_pcl(p.generateColoredPcl(0, dense), T)
    return r


def _half_camera(s):
    """Another camera: half the resolution, intrinsics that are not the settings' halved."""
    return (s.fx * 0.45, s.fy * 0.55, s.width * 0.26, s.height * 0.23, s.width // 2, s.height // 2)


def _ref_view(s, T, splat, camera=None):
    if camera is None:
        return mr.view_of(s, T, splat)
    fx, fy, cx, cy, w, h = camera
    return mr.View(w, h, fx, fy, cx, cy, s.depth_min, s.depth_max, T, splat)


def _assert_view(got, want, what):
    d, b, c = got
    rd, rb, rc = want
    print("%s: covered %d (restatement %d), depth words differing %d, colour bytes differing %d"
          % (what, c, rc, int(np.sum(d.view(np.uint32) != rd.view(np.uint32))), int(np.sum(b != rb))))
    assert d.dtype == np.float32 and b.dtype == np.uint8 and d.shape == rd.shape and b.shape == rb.shape, what
    assert d.tobytes() == rd.tobytes(), what
    assert b.tobytes() == rb.tobytes(), what
    assert c == rc, what


def _bytes(out):
    d, b, c = out
    if isinstance(d, list):
        return b"".join(x.tobytes() for x in d) + b"".join(x.tobytes() for x in b) + np.asarray(c, np.uint32).tobytes()
    return d.tobytes() + b.tobytes() + np.uint32(c).tobytes()


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("splat", [0, 4])
@pytest.mark.parametrize("s", [S320, S640], ids=["320x240", "640x480"])
@pytest.mark.parametrize("dense", [False, True], ids=["edges", "dense"])
def test_bit_exact_against_restatement(dense, s, splat, min_count):
    from revo_amd import api
    cam, pyrs = _keyframes(api, s, [901, 902, 903])
    Ts = KF_POSES[:3]
    voxel = 0.01 if s is S320 else 0.02
    m = api.VoxelMap(cam, voxel, dense=dense)
    m.integrate_many(pyrs, Ts)
    xyz, rgb, cnt = _restate(pyrs, Ts, voxel, dense).points(min_count)
    assert len(xyz) > 100
    if min_count == 2:
        assert len(xyz) < m.info()["voxels"]
    poses = Ts + [BETWEEN, AWAY]
    got = m.render(poses, splat_max=splat, min_count=min_count)
    for k, T in enumerate(poses):
        want = mr.render(xyz, rgb, voxel, _ref_view(s, T, splat))
        _assert_view((got[0][k], got[1][k], got[2][k]), want, "view %d" % k)
        assert (want[2] == 0) == (k == len(poses) - 1)
    assert not got[0][-1].any() and not got[1][-1].any() and got[2][-1] == 0  # looking away: empty
    cam2 = _half_camera(s)
    for T in (Ts[1], BETWEEN):
        want = mr.render(xyz, rgb, voxel, _ref_view(s, T, splat, cam2))
        _assert_view(m.render(T, camera=cam2, splat_max=splat, min_count=min_count), want, "other camera")
        assert want[2] > 0


def test_same_bytes_whatever_the_order_table_batching_and_output_side():
    import torch
    from revo_amd import _lib, api
    cam, pyrs = _keyframes(api, S320, [911, 912, 913, 914])
    Ts = KF_POSES
    poses = Ts[:3] + [BETWEEN]
    cam2 = _half_camera(S320)
    base = None
    for order, init in (([0, 1, 2, 3], 1 << 22), ([3, 1, 0, 2], 1 << 22), ([2, 0, 3, 1], 16)):
        m = api.VoxelMap(cam, 0.01, dense=True, initial_voxels=init)
        for i in order:
            m.integrate(pyrs[i], Ts[i])
        assert (m.info()["rehashes"] >= 2) == (init == 16)
        out = m.render(poses)
        small = m.render(poses[:2], camera=cam2)
        b = _bytes(out) + _bytes(small)
        base = base or b
        assert b == base and sum(out[2]) > 0
    # n views in one call == n single calls == the same call again (the z-buffer is reset), mixed sizes in one call included
    singles = [m.render(T) for T in poses]
    assert _bytes(([x[0] for x in singles], [x[1] for x in singles], [x[2] for x in singles])) == _bytes(out)
    assert _bytes(m.render(poses)) == _bytes(out)
    views = (MapView * 3)()
    sizes = []
    for v, (T, c) in zip(views, ((poses[0], None), (poses[1], cam2), (poses[3], None))):
        fx, fy, cx, cy, w, h = c or (0, 0, 0, 0, S320.width, S320.height)
        v.width, v.height, v.fx, v.fy, v.cx, v.cy = int(w), int(h), fx, fy, cx, cy
        v.zmin, v.zmax = (S320.depth_min, S320.depth_max) if c else (0, 0)
        v.T_w_c[:] = np.asarray(T, np.float32).T.reshape(16).tolist()
        v.splat_max, v.min_count = 4, 1
        sizes.append((int(h), int(w)))
    d = [np.empty(sz, np.float32) for sz in sizes]
    b = [np.empty(sz + (3,), np.uint8) for sz in sizes]
    cov = np.zeros(3, np.uint32)
    _lib.check(_lib.lib().revo_map_render(m._h, 3, views, (C.c_void_p * 3)(*[a.ctypes.data for a in d]),
                                          (C.c_void_p * 3)(*[a.ctypes.data for a in b]), cov.ctypes.data_as(C.c_void_p), 0))
    mixed = [(d[k], b[k], int(cov[k])) for k in range(3)]
    assert _bytes(mixed[0]) == _bytes(singles[0]) and _bytes(mixed[2]) == _bytes(singles[3])
    assert _bytes(mixed[1]) == _bytes((small[0][1], small[1][1], small[2][1]))
    # device output == host output
    dd = torch.full((len(poses), S320.height, S320.width), -1.0, dtype=torch.float32, device="cuda")
    db = torch.full((len(poses), S320.height, S320.width, 3), 7, dtype=torch.uint8, device="cuda")
    dc = torch.full((len(poses),), -1, dtype=torch.int32, device="cuda")
    m.render_into(dd, db, poses, d_covered=dc)
    dev = (list(dd.cpu().numpy()), list(db.cpu().numpy()), [int(x) for x in dc.cpu().numpy()])
    assert _bytes(dev) == _bytes(out)
    d1 = torch.empty((S320.height, S320.width), dtype=torch.float32, device="cuda")
    b1 = torch.empty((S320.height, S320.width, 3), dtype=torch.uint8, device="cuda")
    m.render_into(d1, b1, poses[2])
    assert d1.cpu().numpy().tobytes() == out[0][2].tobytes() and b1.cpu().numpy().tobytes() == out[1][2].tobytes()
    assert m.last_render_ms() > 0


def test_two_processes_give_identical_bytes(tmp_path):
    script = tmp_path / "run_render.py"
    script.write_text(
        "import sys, numpy as np\n"
        "sys.path[:0] = [%r, %r]\n"
        "from revo_amd import api, synth\n"
        "from revo_amd.settings import ImgPyramidSettings\n"
        "s = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))\n"
        "cam = api.CameraPyr(s)\n"
        "m = api.VoxelMap(cam, 0.005, dense=True)\n"
        "Ts = [synth.se3_exp(np.array([0.02 * k, 0.01, -0.01 * k, 0.01, 0.02 * k, 0.0])).astype(np.float32) for k in range(3)]\n"
        "for sd, T in zip((921, 922, 923), Ts):\n"
        "    m.integrate(api.ImgPyramidRGBD(s, cam, *synth.make_pair(sd, s)['ref']), T)\n"
        "d, b, c = m.render(Ts)\n"
        "open(sys.argv[1], 'wb').write(b''.join(x.tobytes() for x in d + b) + np.asarray(c, np.uint32).tobytes())\n"
        % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(__file__)))
    outs = []
    for k in range(2):
        p = str(tmp_path / ("v%d.bin" % k))
        subprocess.run([sys.executable, str(script), p], check=True, timeout=300)
        outs.append(open(p, "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) == 3 * 320 * 240 * 7 + 12
    assert any(outs[0][:320 * 240 * 4])


def test_constant_depth_plane_is_fully_covered_on_the_device():
    """tests/test_map_render_cpu.py::test_constant_depth_plane_is_fully_covered_at_its_own_pose on the device."""
    from revo_amd import api
    s = S640
    rng = np.random.default_rng(6)
    depth = np.full((s.height, s.width), 1.0, np.float32)
    bgr = rng.integers(0, 256, (s.height, s.width, 3)).astype(np.uint8)
    cam = api.CameraPyr(s)
    pyr = api.ImgPyramidRGBD(s, cam, bgr, depth)
    I4 = np.eye(4, dtype=np.float32)
    m = api.VoxelMap(cam, 0.01, dense=True)
    m.integrate(pyr, I4)
    r = _restate([pyr], [I4], 0.01, True)
    assert r.points_integrated == s.width * s.height
    xyz, rgb, _ = r.points()
    got = m.render(I4, splat_max=4)
    _assert_view(got, mr.render(xyz, rgb, 0.01, mr.view_of(s, I4, 4)), "plane")
    assert got[2] == s.width * s.height
    assert np.abs(got[0].astype(np.float64) - 1.0).max() <= 2.0 ** -20


def test_render_follows_integrations_and_leaves_the_map_alone():
    from revo_amd import api
    cam, pyrs = _keyframes(api, S320, [931, 932, 933])
    Ts = KF_POSES[:3]
    m = api.VoxelMap(cam, 0.01, dense=True)
    m.integrate(pyrs[0], Ts[0])
    first = m.render(BETWEEN)
    xyz, rgb, _ = _restate(pyrs[:1], Ts[:1], 0.01, True).points()
    _assert_view(first, mr.render(xyz, rgb, 0.01, mr.view_of(S320, BETWEEN, 4)), "one keyframe")
    m.integrate(pyrs[1], Ts[1])  # asynchronous: the render right behind it must see it
    m.integrate(pyrs[2], Ts[2])
    second = m.render(BETWEEN)
    xyz, rgb, _ = _restate(pyrs, Ts, 0.01, True).points()
    _assert_view(second, mr.render(xyz, rgb, 0.01, mr.view_of(S320, BETWEEN, 4)), "three keyframes")
    assert _bytes(first) != _bytes(second)
    before = b"".join(a.tobytes() for a in m.points())
    info = m.info()
    for splat in (0, 4, 8):
        m.render(Ts + [AWAY], splat_max=splat, min_count=2)
    assert b"".join(a.tobytes() for a in m.points()) == before and m.info() == info
    # an empty map renders empty views
    e = api.VoxelMap(cam, 0.01)
    d, b, c = e.render(BETWEEN)
    assert c == 0 and not d.any() and not b.any()
    m.clear()
    d, b, c = m.render(BETWEEN)
    assert c == 0 and not d.any() and not b.any()


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_run_tum_map_views(tmp_path, monkeypatch):
    from test_gpu_configs import SAME_PARTITION
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    from revo_amd import ply, run_tum, tum
    from test_gpu_vo_multi import _tum_yaml
    from test_gpu_voxel_map import BIASES
    names = ["rgbd_synth_a", "rgbd_synth_b"]
    for k, (n, lens) in enumerate(zip(names, (40, 33))):
        seq = synth.make_sequence(951 + k, S320, lens, max_t=0.01, max_rot_deg=0.4, bias=BIASES[3 + k])
        tum.write_synthetic_dataset(str(tmp_path / "data" / n), seq)
    _tum_yaml(tmp_path, S320, names)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "2", "--map", "0.01"]
    runs = (("plain", []), ("seq", ["--map-views", "views"]), ("multi", ["--map-views", "views", "--streams", "2"]),
            ("every", ["--map-views", "views", "--map-views-every", "5"]))
    for sub, extra in runs:
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra) == 0
    assert run_tum.main(args[:4] + ["--map-views", "views"]) == 2  # --map-views without --map: a usage error
    monkeypatch.chdir(tmp_path)
    n_views = 0
    for n in names:
        for f in ("poses_%s.txt" % n, "map_%s.ply" % n):  # the run's own files do not depend on --map-views
            assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "seq" / f).read_bytes(), f
        seq_dir, multi_dir = tmp_path / "seq" / "views" / n, tmp_path / "multi" / "views" / n
        files = _tree(seq_dir)
        assert files == _tree(multi_dir) and "associate.txt" in files and "poses.txt" in files
        for f in files:
            assert (seq_dir / f).read_bytes() == (multi_dir / f).read_bytes(), f
        rows = tum.read_associate(str(seq_dir / "associate.txt"))
        poses = tum.read_poses(str(seq_dir / "poses.txt"))
        assert len(rows) == len(poses) >= 1
        n_views += len(rows)
        # the finished map is what map_<dataset>.ply holds; the restatement over it equals VoxelMap.render (tests above)
        xyz, rgb, cnt = ply.read_voxel_ply(str(tmp_path / "seq" / ("map_%s.ply" % n)))
        for (rts, rf, dts, df), (ts, T) in zip(rows, poses):
            bgr, d16 = tum.load_frame(str(seq_dir), rf, df)
            assert abs(rts - ts) < 1e-6 and rts == dts and rf == "rgb/%.6f.png" % rts and df == "depth/%.6f.png" % rts
            want = mr.render(xyz, rgb, 0.01, mr.view_of(S320, T, 4))
            raw = np.clip(np.rint(want[0].astype(np.float64) * 5000.0), 0, 65535).astype(np.uint16)
            assert d16.dtype == np.uint16 and d16.tobytes() == raw.tobytes()
            assert bgr.tobytes() == want[1].tobytes()
            assert want[2] > 100
        every = tum.read_associate(str(tmp_path / "every" / "views" / n / "associate.txt"))
        n_frames = len((tmp_path / "plain" / ("poses_%s.txt" % n)).read_text().splitlines())
        assert len(every) == (n_frames + 4) // 5
    assert n_views >= 3  # one view per keyframe: the first frame of each sequence and the keyframes promoted later


def test_argument_errors_leave_the_handle_usable():
    from revo_amd import _lib, api
    L = _lib.lib()
    cam, pyrs = _keyframes(api, S320, [941])
    m = api.VoxelMap(cam, 0.01, dense=True)
    m.integrate(pyrs[0], np.eye(4))
    good = m.render(BETWEEN)
    d = np.empty((S320.height, S320.width), np.float32)
    b = np.empty((S320.height, S320.width, 3), np.uint8)
    dp, bp = (C.c_void_p * 1)(d.ctypes.data), (C.c_void_p * 1)(b.ctypes.data)

    def view(**kw):
        v = (MapView * 1)()
        v[0].width, v[0].height, v[0].splat_max, v[0].min_count = S320.width, S320.height, 4, 1
        v[0].T_w_c[:] = np.asarray(BETWEEN, np.float32).T.reshape(16).tolist()
        for k, x in kw.items():
            if k == "T":
                v[0].T_w_c[x[0]] = x[1]
            else:
                setattr(v[0], k, x)
        return v

    cam_ok = dict(fx=200.0, fy=200.0, cx=160.0, cy=120.0, zmin=0.1, zmax=5.0)
    bad = [view(width=0), view(width=2049), view(height=0), view(height=2049), view(splat_max=-1), view(splat_max=9),
           view(T=(13, float("nan"))), view(T=(0, float("inf"))),
           view(**dict(cam_ok, fx=float("nan"))), view(**dict(cam_ok, cy=float("inf"))), view(**dict(cam_ok, zmax=float("nan"))),
           view(**dict(cam_ok, zmin=5.0)), view(**dict(cam_ok, zmin=6.0))]
    for k, v in enumerate(bad):
        assert L.revo_map_render(m._h, 1, v, dp, bp, None, 0) == INVALID_ARG, k
        assert L.revo_last_error()
    ok = view()
    assert L.revo_map_render(m._h, 0, ok, dp, bp, None, 0) == INVALID_ARG
    assert L.revo_map_render(m._h, -1, ok, dp, bp, None, 0) == INVALID_ARG
    assert L.revo_map_render(m._h, 1, None, dp, bp, None, 0) == INVALID_ARG
    assert L.revo_map_render(m._h, 1, ok, None, bp, None, 0) == INVALID_ARG
    assert L.revo_map_render(m._h, 1, ok, dp, None, None, 0) == INVALID_ARG
    assert L.revo_map_render(m._h, 1, ok, (C.c_void_p * 1)(None), bp, None, 0) == INVALID_ARG
    assert L.revo_map_render(None, 1, ok, dp, bp, None, 0) == INVALID_ARG
    assert L.revo_map_render(m._h, 1, ok, (C.c_void_p * 1)((d.ctypes.data & ~15) + 4), bp, None, 1) == INVALID_ARG  # misaligned
    assert L.revo_map_render(m._h, 1, view(**cam_ok), dp, bp, None, 0) == 0
    assert L.revo_map_render(m._h, 1, ok, dp, bp, None, 0) == 0
    assert d.tobytes() == good[0].tobytes() and b.tobytes() == good[1].tobytes()
    assert _bytes(m.render(BETWEEN)) == _bytes(good)
