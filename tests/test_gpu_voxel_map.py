"""World-frame voxel map on the device (revo_map_*, api.VoxelMap): bit for bit the numpy restatement of tests/voxel_map_ref.py
over generateColoredPcl(0, dense) of the same pyramids; independent of order, batching, table growth and driver; all-or-nothing
at max_voxels; the same map from vo.REVO, vo.MultiREVO and run_tum with or without --streams."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import synth  # noqa: E402
from revo_amd.settings import ImgPyramidSettings  # noqa: E402

from test_gpu_configs import SAME_PARTITION  # noqa: E402
import voxel_map_ref as ref  # noqa: E402

INVALID_ARG, CAPACITY = -1, -5
S320 = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
S640 = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
BIASES = [[0.004, 0, 0, 0, np.deg2rad(1.0), 0], [0, 0.003, 0, np.deg2rad(1.0), 0, 0], [0.002, 0, 0.003, 0, np.deg2rad(1.2), 0],
          [0, 0, 0, 0, np.deg2rad(1.5), 0], [0.005, 0.002, 0, 0, np.deg2rad(0.8), np.deg2rad(0.5)]]


def _poses(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        T = synth.se3_exp(np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-0.6, 0.6, 3)])).astype(np.float32)
        out.append(T)
    return out


def _keyframes(api, s, seeds):
    cam = api.CameraPyr(s)
    pyrs = []
    for sd in seeds:
        bgr, depth = synth.make_pair(sd, s)["ref"]
        pyrs.append(api.ImgPyramidRGBD(s, cam, bgr, depth))
    return cam, pyrs


def _restate(pyrs, Ts, voxel, dense):
    r = ref.VoxelMapRef(voxel)
    for p, T in zip(pyrs, Ts):
        r.integrate_pcl(p.generateColoredPcl(0, dense), T)
    return r


def _bytes(pts):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in pts)


def _assert_equal(got, want):
    for g, w, name in zip(got, want, ("xyz", "rgb", "count")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, int(np.sum(g != w)))


@pytest.mark.parametrize("s", [S320, S640], ids=["320x240", "640x480"])
@pytest.mark.parametrize("dense", [False, True], ids=["edges", "dense"])
def test_bit_exact_against_restatement(s, dense):
    from revo_amd import api
    cam, pyrs = _keyframes(api, s, [901, 902, 903])
    Ts = _poses(3, 5)
    for voxel in (0.002, 0.02, 0.15):
        m = api.VoxelMap(cam, voxel, dense=dense)
        for p, T in zip(pyrs, Ts):
            m.integrate(p, T)
        r = _restate(pyrs, Ts, voxel, dense)
        got = m.points()
        _assert_equal(got, r.points())
        info = m.info()
        assert info["voxels"] == r.voxels() and info["keyframes"] == 3
        assert info["points_integrated"] == r.points_integrated and info["points_dropped"] == r.points_dropped == 0
        if voxel == 0.002:
            assert np.mean(got[2] == 1) > 0.3  # many voxels hold a single point
        assert info["capacity"] >= 2 * info["voxels"]
        _assert_equal(m.points(min_count=3), r.points(min_count=3))


def test_order_batching_and_repeat_independent():
    from revo_amd import api
    cam, pyrs = _keyframes(api, S320, [911, 912, 913, 914])
    Ts = _poses(4, 6)
    outs = []
    for order, batch in (([0, 1, 2, 3], False), ([3, 1, 0, 2], False), ([2, 3, 1, 0], True), ([0, 1, 2, 3], True)):
        for dense in (False, True):
            m = api.VoxelMap(cam, 0.01, dense=dense)
            if batch:
                m.integrate_many([pyrs[i] for i in order], [Ts[i] for i in order])
            else:
                for i in order:
                    m.integrate(pyrs[i], Ts[i])
            outs.append((dense, _bytes(m.points())))
    for dense in (False, True):
        b = [o for d, o in outs if d == dense]
        assert all(x == b[0] for x in b)
    # clear, then the same integrations again
    m = api.VoxelMap(cam, 0.01, dense=True)
    m.integrate(pyrs[0], Ts[0])
    m.clear()
    assert m.info()["voxels"] == 0 and m.points()[0].shape == (0, 3)
    for i in range(4):
        m.integrate(pyrs[i], Ts[i])
    assert _bytes(m.points()) == [o for d, o in outs if d][0]


def test_two_processes_give_identical_bytes(tmp_path):
    script = tmp_path / "run_map.py"
    script.write_text(
        "import sys, numpy as np\n"
        "sys.path[:0] = [%r, %r]\n"
        "from revo_amd import api, synth\n"
        "from revo_amd.settings import ImgPyramidSettings\n"
        "s = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))\n"
        "cam = api.CameraPyr(s)\n"
        "m = api.VoxelMap(cam, 0.005, dense=True)\n"
        "for sd in (921, 922):\n"
        "    p = api.ImgPyramidRGBD(s, cam, *synth.make_pair(sd, s)['ref'])\n"
        "    m.integrate(p, synth.se3_exp(np.array([0.1 * (sd - 920), 0.2, -0.3, 0.1, 0.2, 0.3])).astype(np.float32))\n"
        "m.save_ply(sys.argv[1])\n" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(__file__)))
    outs = []
    for k in range(2):
        p = str(tmp_path / ("m%d.ply" % k))
        subprocess.run([sys.executable, str(script), p], check=True, timeout=300)
        outs.append(open(p, "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 1000


def test_growth_gives_the_large_table_bytes():
    from revo_amd import api
    cam, pyrs = _keyframes(api, S640, [931, 932, 933, 934, 935])
    Ts = _poses(5, 7)
    small = api.VoxelMap(cam, 0.004, dense=True, initial_voxels=16)
    big = api.VoxelMap(cam, 0.004, dense=True, initial_voxels=1 << 23)
    for p, T in zip(pyrs, Ts):
        small.integrate(p, T)
        big.integrate(p, T)
    i_small, i_big = small.info(), big.info()
    assert i_small["rehashes"] >= 2 and i_big["rehashes"] == 0, (i_small, i_big)
    assert i_small["capacity"] < i_big["capacity"]
    assert _bytes(small.points()) == _bytes(big.points())
    _assert_equal(small.points(), _restate(pyrs, Ts, 0.004, True).points())


def test_capacity_is_all_or_nothing_and_drops_are_counted():
    from revo_amd import api
    from revo_amd._lib import RevoError
    cam, pyrs = _keyframes(api, S320, [941, 942, 943])
    Ts = _poses(3, 8)
    first = _restate(pyrs[:1], Ts[:1], 0.01, True)
    two = _restate(pyrs[:2], Ts[:2], 0.01, True)
    cap = (first.voxels() + two.voxels()) // 2
    assert first.voxels() < cap < two.voxels()
    m = api.VoxelMap(cam, 0.01, dense=True, max_voxels=cap)
    m.integrate(pyrs[0], Ts[0])
    with pytest.raises(RevoError) as e:
        m.integrate(pyrs[1], Ts[1])
    assert e.value.code == CAPACITY
    info = m.info()
    assert info["voxels"] == first.voxels() and info["keyframes"] == 1 and info["keyframes_rejected"] == 1
    _assert_equal(m.points(), first.points())
    with pytest.raises(RevoError):
        m.integrate_many(pyrs[1:], Ts[1:])
    _assert_equal(m.points(), first.points())
    # the map stays usable: a keyframe that fits goes in
    m.integrate(pyrs[0], Ts[0])
    r = _restate([pyrs[0], pyrs[0]], [Ts[0], Ts[0]], 0.01, True)
    _assert_equal(m.points(), r.points())
    # beyond +-2048 m and the 21-bit key range: dropped and counted like the restatement
    far = np.eye(4, dtype=np.float32)
    far[:3, 3] = [2047.5, -2047.2, 3.0]
    tiny = api.VoxelMap(cam, 0.0009765625, dense=True)  # 2^-10 m: |k| reaches 2^20 at 1024 m
    for mm, v in ((api.VoxelMap(cam, 0.05, dense=True), 0.05), (tiny, 0.0009765625)):
        mm.integrate(pyrs[2], far)
        rr = _restate([pyrs[2]], [far], v, True)
        assert 0 < rr.points_dropped and mm.info()["points_dropped"] == rr.points_dropped
        assert mm.info()["points_integrated"] == rr.points_integrated
        _assert_equal(mm.points(), rr.points())


def test_revo_with_voxel_map_and_drawer():
    from revo_amd import api, ply, vo
    frames = synth.make_sequence(951, S320, 40, max_t=0.01, max_rot_deg=0.4, bias=BIASES[3])
    for dense in (False, True):
        cam = api.CameraPyr(S320)
        drawer = ply.ModelExporter()
        vm = api.VoxelMap(cam, 0.01, dense=dense)
        g = vo.REVO(S320, cameraPyr=cam, mapDrawer=drawer, generate_dense_pcl=dense, voxelMap=vm)
        for f in frames:
            g.push(f[0], f[1], f[2])
        assert g.nKeyFrames >= 3 and len(drawer.vpKfsF) == g.nKeyFrames
        r = ref.VoxelMapRef(0.01)
        for pcl, T in zip(drawer.pclKfHost, drawer.vpKfsF):
            r.integrate_pcl(pcl, T)
        _assert_equal(vm.points(), r.points())
        assert vm.info()["keyframes"] == g.nKeyFrames


def _solo_map(s, frames, voxel, dense):
    from revo_amd import api, vo
    cam = api.CameraPyr(s)
    vm = api.VoxelMap(cam, voxel, dense=dense)
    g = vo.REVO(s, cameraPyr=cam, voxelMap=vm)
    for f in frames:
        g.push(f[0], f[1], f[2])
    return _bytes(vm.points()), g.nKeyFrames


@pytest.mark.parametrize("dense", [False, True], ids=["edges", "dense"])
def test_multi_revo_maps_equal_solo_revo(monkeypatch, dense):
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    from revo_amd import vo
    lens = [30, 18, 26, 12, 22]
    seqs = [[f[:3] for f in synth.make_sequence(960 + k, S320, n, max_t=0.01, max_rot_deg=0.4, bias=BIASES[k])]
            for k, n in enumerate(lens)]
    m = vo.MultiREVO(S320, 4, map_voxel=0.01, map_dense=dense)
    res = m.run(seqs)
    for k, r in enumerate(res):
        b, nkf = _solo_map(S320, seqs[k], 0.01, dense)
        assert r.map is not None and r.map.info()["keyframes"] == nkf == sum(1 for _, kf in r if kf), k
        assert _bytes(r.map.points()) == b, k
    assert sum(r.map.info()["keyframes"] for r in res) >= 10


def test_multi_revo_maps_equal_solo_revo_640x480(monkeypatch):
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    from revo_amd import vo
    seqs = [[f[:3] for f in synth.make_sequence(970 + k, S640, n, max_t=0.01, max_rot_deg=0.4, bias=BIASES[k + 1])]
            for k, n in enumerate((16, 11, 13))]
    m = vo.MultiREVO(S640, 2, map_voxel=0.02, map_dense=True)
    res = m.run(seqs)
    for k, r in enumerate(res):
        b, nkf = _solo_map(S640, seqs[k], 0.02, True)
        assert r.map.info()["keyframes"] == nkf and _bytes(r.map.points()) == b, k


def test_run_tum_map_sequential_equals_streams(tmp_path, monkeypatch):
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    from revo_amd import ply, run_tum, tum
    from test_gpu_vo_multi import _tum_yaml
    names = ["rgbd_synth_a", "rgbd_synth_b", "rgbd_synth_c"]
    for k, (n, lens) in enumerate(zip(names, (14, 22, 9))):
        seq = synth.make_sequence(40 + k, S320, lens, max_t=0.01, max_rot_deg=0.4, bias=BIASES[k])
        tum.write_synthetic_dataset(str(tmp_path / "data" / n), seq)
    _tum_yaml(tmp_path, S320, names)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "2", "--map", "0.02"]
    for sub, extra in (("seq", []), ("multi", ["--streams", "2"]), ("gpu", ["--streams", "2", "--gpu-decode"])):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra) == 0
    for n in names:
        a = (tmp_path / "seq" / ("map_%s.ply" % n)).read_bytes()
        assert a == (tmp_path / "multi" / ("map_%s.ply" % n)).read_bytes() == (tmp_path / "gpu" / ("map_%s.ply" % n)).read_bytes()
        xyz, rgb, cnt = ply.read_voxel_ply(str(tmp_path / "seq" / ("map_%s.ply" % n)))
        assert len(xyz) > 100 and cnt.min() >= 1


def test_argument_errors():
    from revo_amd import _lib, api, vo
    L = _lib.lib()
    cam, pyrs = _keyframes(api, S320, [981])
    other = api.CameraPyr(S320)
    h = C.c_void_p()
    for voxel in (0.0, -0.01, float("nan"), float("inf")):
        assert L.revo_map_create(cam._h, C.c_float(voxel), 0, 1024, 1 << 20, C.byref(h)) == INVALID_ARG
    assert L.revo_map_create(cam._h, C.c_float(0.01), 2, 1024, 1 << 20, C.byref(h)) == INVALID_ARG
    assert L.revo_map_create(cam._h, C.c_float(0.01), 0, 1024, 0, C.byref(h)) == INVALID_ARG
    assert L.revo_map_create(None, C.c_float(0.01), 0, 1024, 1 << 20, C.byref(h)) == INVALID_ARG
    m = api.VoxelMap(cam, 0.01)
    T = np.eye(4, dtype=np.float32).T.copy().reshape(16)
    bad = T.copy()
    bad[13] = np.nan
    f32p = _lib.f32p
    assert L.revo_map_integrate(m._h, pyrs[0]._h, bad.ctypes.data_as(f32p)) == INVALID_ARG
    assert b"finite" in L.revo_last_error()
    assert L.revo_map_integrate(m._h, None, T.ctypes.data_as(f32p)) == INVALID_ARG
    p_other = api.ImgPyramidRGBD(S320, other, *synth.make_pair(981, S320)["ref"])
    assert L.revo_map_integrate(m._h, p_other._h, T.ctypes.data_as(f32p)) == INVALID_ARG
    assert b"context" in L.revo_last_error()
    assert m.info()["keyframes"] == 0
    mv = vo.MultiREVO(S320, 2, cameraPyr=cam)
    for s in (-1, 2):
        assert L.revo_vo_multi_attach_map(mv._h, s, m._h) == INVALID_ARG
    mo = vo.MultiREVO(S320, 2, cameraPyr=other)
    assert L.revo_vo_multi_attach_map(mo._h, 0, m._h) == INVALID_ARG
    assert L.revo_vo_multi_attach_map(mv._h, 1, m._h) == 0
    m.close()  # destroying an attached map detaches it
    assert L.revo_vo_multi_attach_map(mv._h, 1, None) == 0
    n = C.c_size_t()
    m2 = api.VoxelMap(cam, 0.01, dense=True)
    m2.integrate(pyrs[0], np.eye(4))
    L.revo_map_extract(m2._h, 1, None, None, None, 0, C.byref(n))
    buf = np.empty((max(1, n.value - 1), 3), np.float32)
    assert L.revo_map_extract(m2._h, 1, buf.ctypes.data_as(f32p), None, None, n.value - 1, C.byref(n)) == CAPACITY
