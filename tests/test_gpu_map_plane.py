"""Point-to-plane registration of voxel maps on the device (revo_map_normals / revo_map_align_plane_eval / revo_map_align_plane,
api.align_maps(metric="plane")): normals and records bit for bit the numpy specification's (tests/map_plane_ref.py),
whatever the table size, the integration order, the batching of poses, the output side or the grid; the maps are not changed and
the fault word stays clear; the iteration follows the specification's loop; the ladder recovers a known twist; the default metric
is untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile, ply, synth  # noqa: E402
from revo_amd.settings import ImgPyramidSettings, ALIGN_CONVERGED, ALIGN_LOST  # noqa: E402

import map_align_ref as mar  # noqa: E402
import map_plane_cases as mc  # noqa: E402
import map_plane_ref as mpr  # noqa: E402
import map_records_ref as mrr  # noqa: E402
import voxel_map_ref as ref  # noqa: E402

F = np.float32
INVALID_ARG = -1
S320 = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
SEEDS = [902, 903]
I4 = np.eye(4, dtype=F)
VOXEL = 0.02
KF_POSES = [synth.se3_exp(np.asarray(t, np.float64)).astype(F) for t in ([0, 0, 0, 0, 0, 0], [0.05, 0.01, 0.0, 0.0, 0.03, 0.0])]
D_SMALL = synth.se3_exp(np.array([0.006, -0.004, 0.005, 0.002, -0.001, 0.0015]))
NEAR = (synth.se3_exp(np.array([0.003, -0.002, 0.002, 0.001, -0.001, 0.0005])) @ np.linalg.inv(D_SMALL)).astype(F)
OFF = (synth.se3_exp(np.array([0.03, 0.0, 0.0, 0.0, 0.0, 0.0])) @ np.linalg.inv(D_SMALL)).astype(F)  # a voxel and a half off
D_LADDER = synth.se3_exp(np.array([0.02, -0.015, 0.012, 0.006, -0.005, 0.004]))
# The specification's own point-to-plane ladder (shifts 2, 1, 0; dense clouds of SEEDS at KF_POSES, voxel 0.02, source at
# D_LADDER * pose, from identity) ends 1.77e-5 m and 1.48e-5 rad from D_LADDER^-1 after 4 + 4 + 3 iterations, measured on the CPU
# (point-to-point on the same maps: 4.66e-4 m, 2.48e-3 rad, 3 + 17 + 9).  The bounds are twice that.
PLANE_LADDER_ERR_T, PLANE_LADDER_ERR_R = 2 * 1.77e-5, 2 * 1.48e-5


@functools.lru_cache(maxsize=None)
def _scene():
    from revo_amd import api
    cam = api.CameraPyr(S320)
    pyrs = [api.ImgPyramidRGBD(S320, cam, *synth.make_pair(sd, S320)["ref"]) for sd in SEEDS]
    clouds = {d: [ref.points_from_pcl(p.generateColoredPcl(0, d)) for p in pyrs] for d in (False, True)}
    return api, cam, pyrs, clouds


def _poses(D_key=None):
    D = {None: np.eye(4), "small": D_SMALL, "ladder": D_LADDER}[D_key]
    return [(D @ T.astype(np.float64)).astype(F) for T in KF_POSES]


@functools.lru_cache(maxsize=None)
def _records(dense, D_key=None):
    r = ref.VoxelMapRef(VOXEL)
    for (xyz, rgb), T in zip(_scene()[3][dense], _poses(D_key)):
        r.integrate(xyz, rgb, T)
    return mrr.records_of(r)


@functools.lru_cache(maxsize=None)
def _target(dense, min_count=1):
    return mpr.Target(_records(dense), F(VOXEL), min_count)


def _build(dense, D_key=None, order=(0, 1), **kw):
    api, cam, pyrs, _ = _scene()
    m = api.VoxelMap(cam, VOXEL, dense=dense, **kw)
    Ts = _poses(D_key)
    for i in order:
        m.integrate(pyrs[i], Ts[i])
    return m


def _hand(rows, voxel=VOXEL, **kw):
    api, cam = _scene()[:2]
    rec = mc.records(rows)
    m = api.VoxelMap(cam, voxel, **kw)
    m.merge_raw(rec.astype(mapfile.RAW_DTYPE))
    return m, rec


def _check_normals(m, rec, what, **prm):
    """normals on the device against the specification: all four outputs bit for bit; -> the specification's."""
    xyz, nv, lam, nb = m.normals(**prm)
    want = mpr.normals(rec, **prm)
    print("%s: %d voxels, %d valid" % (what, len(want[0]), int(want[5].sum())))
    assert xyz.tobytes() == want[1].tobytes() and nb.tobytes() == want[4].astype(np.uint32).tobytes(), what
    assert lam.tobytes() == want[3].tobytes(), (what, int(np.sum(lam.view(np.uint32) != want[3].view(np.uint32))))
    assert nv.tobytes() == want[2].tobytes(), (what, int(np.sum(nv.view(np.uint32) != want[2].view(np.uint32))))
    return want


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("dense", [False, True], ids=["edges", "dense"])
def test_normals_bit_exact(dense, min_count):
    m = _build(dense)
    before = m.export_raw().tobytes()
    assert before == _records(dense).tobytes()
    w = _check_normals(m, _records(dense), "scene", min_count=min_count)
    assert len(w[0]) == int((_records(dense)["count"] >= min_count).sum()) and (w[5].sum() > 1000 or not dense)
    xyz = m.points(min_count)[0]
    assert xyz.tobytes() == w[1].tobytes()  # revo_map_extract's voxels in its order
    assert m.export_raw().tobytes() == before


def test_normals_of_hand_made_maps():
    api, cam = _scene()[:2]
    for name, rows in (("patch", mc.patch()), ("tilted", mc.patch(mc.TILT)), ("line", mc.line()), ("block", mc.block()),
                       ("three patches", mc.three_patches())):
        m, rec = _hand(rows)
        for mn in (5, 3):
            _check_normals(m, rec, "%s, min_neighbours %d" % (name, mn), min_neighbours=mn)
    m, rec = _hand(mc.patch())
    assert m.normals()[1][4].tolist() == [0.0, 0.0, 1.0]
    # index 2^20 - 1: the neighbours past it are out of key range
    m, rec = _hand(mc.last_index(), voxel=2.0 ** -9)
    w = _check_normals(m, rec, "last index")
    assert w[4].tolist() == [4, 6, 4, 6, 9, 6, 4, 6, 4] and w[5].sum() == 5
    # a subtracted voxel is no neighbour; min_count 2 leaves out the voxels of count 1
    m, rec = _hand(mc.patch())
    m.subtract_raw(rec[4:5].astype(mapfile.RAW_DTYPE))
    w = _check_normals(m, np.delete(rec, 4), "after subtract")
    assert w[4].tolist() == [3, 5, 3, 5, 5, 3, 5, 3]
    m, rec = _hand([(k, p, 2 if i != 8 else 1) for i, (k, p, _) in enumerate(mc.patch())])
    assert len(_check_normals(m, rec, "min_count 2", min_count=2)[0]) == 8
    # an empty map
    empty = api.VoxelMap(cam, VOXEL)
    assert all(len(a) == 0 for a in empty.normals())
    # parameters outside their ranges
    from revo_amd import _lib
    from revo_amd.settings import MapNormalsParams
    n = C.c_size_t()
    for bad in ((1, 2, 0.1, 0.1), (1, 5, 0.0, 0.1), (1, 5, 1.0, 0.1), (1, 5, float("nan"), 0.1), (1, 5, 0.1, -0.1), (1, 5, 0.1, 1.0)):
        assert _lib.lib().revo_map_normals(m._h, C.byref(MapNormalsParams(*bad)), None, None, None, None, 0, C.byref(n)) == INVALID_ARG, bad
    assert _lib.lib().revo_map_normals(None, None, None, None, None, None, 0, C.byref(n)) == INVALID_ARG
    assert _lib.lib().revo_map_normals(m._h, None, None, None, None, None, 0, C.byref(n)) == 0 and n.value == 9


def _check(dst, tgt, src, src_rec, poses, what, **prm):
    """align_plane_eval on the device against the specification, record by record; -> the specification's records."""
    got = dst.align_plane_eval(src, poses, **prm)
    spec = {k: v for k, v in prm.items() if k in ("max_dist", "min_count_src", "centre")}
    spec.setdefault("max_dist", F(dst.voxel))
    want = [mpr.align_plane_eval(tgt, src_rec, T, **spec) for T in poses]
    for i, (g, w) in enumerate(zip(got, want)):
        a, b = np.frombuffer(bytes(g), np.uint32), np.frombuffer(bytes(w), np.uint32)
        print("%s, pose %d: matched %d of %d (skipped %d), %d normals, words differing %d"
              % (what, i, w.matched, w.considered, w.skipped, w.dst_normals, int(np.sum(a != b))))
        assert bytes(g) == bytes(w), (what, i)
    return want


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("dense", [False, True], ids=["edges", "dense"])
def test_records_bit_exact(dense, min_count):
    dst, src = _build(dense), _build(dense, "small")
    sr = _records(dense, "small")
    tgt = _target(dense, min_count)
    c = mar.default_centre(sr, I4, min_count)
    w = _check(dst, tgt, src, sr, [NEAR, OFF], "gate 1 voxel", min_count_dst=min_count, min_count_src=min_count, centre=c)
    assert w[0].considered == int((sr["count"] >= min_count).sum()) and w[0].dst_normals == tgt.dst_normals
    if dense:
        assert w[0].matched > 1000 and 0 < w[1].matched < w[0].matched
    w = _check(dst, tgt, src, sr, [NEAR, OFF], "gate 1/4 voxel", max_dist=0.005, min_count_dst=min_count, min_count_src=min_count, centre=c)
    assert all(x.matched < x.considered for x in w)


def test_same_bytes_whatever_the_launch():
    import torch
    sr, dr = _records(True, "small"), _records(True)
    assert len(sr) > 1500 and len(sr) > 8 * 512  # several workgroups: the cross-workgroup partials and the last-ticket reduce
    src = _build(True, "small")
    skew, nan = I4.copy(), I4.copy()
    skew[0, 1] = 0.01
    nan[1, 3] = np.nan
    poses = [NEAR, OFF, I4, skew, nan, NEAR, OFF, I4]
    c = (0.1, 0.2, 0.3)
    base = [bytes(w) for w in _check(_build(True), _target(True), src, sr, poses, "dense", centre=c)]
    assert [mpr.PlaneInfo.from_buffer_copy(b).flags for b in base] == [0, 0, 0, 1, 1, 0, 0, 0]
    bad = mpr.PlaneInfo.from_buffer_copy(base[3])
    assert bad.matched == 0 and not any(bad.S) and bad.dst_normals == 0 and tuple(bad.centre) == tuple(F(c)) and bad.max_dist == F(VOXEL)
    small, large = _build(True, initial_voxels=1 << 10), _build(True, initial_voxels=1 << 20, order=(1, 0))
    assert small.info()["capacity"] != large.info()["capacity"]
    before = small.export_raw().tobytes(), src.export_raw().tobytes(), small.info(), src.info()
    for m in (small, large):
        assert [bytes(g) for g in m.align_plane_eval(src, poses, centre=c)] == base          # 8 poses in one call
        assert [bytes(m.align_plane_eval(src, T, centre=c)) for T in poses] == base          # against 8 single calls
    rsrc = _build(True, "small", order=(1, 0), initial_voxels=1 << 10)
    assert [bytes(g) for g in small.align_plane_eval(rsrc, poses, centre=c)] == base
    d = torch.zeros(208 * 8 + 16, dtype=torch.uint8, device="cuda")
    assert small.align_plane_eval(src, poses, centre=c, d_out=d) is None
    out = d.cpu().numpy()
    assert out[:208 * 8].tobytes() == b"".join(base) and not out[208 * 8:].any()
    assert (small.export_raw().tobytes(), src.export_raw().tobytes(), small.info(), src.info()) == before
    small.integrate(_scene()[2][0], KF_POSES[1])  # the fault word is clear: the map goes on working
    assert small.info()["keyframes"] == 3


def test_a_destination_without_normals_and_argument_errors():
    from revo_amd import _lib
    from revo_amd.settings import MapAlignParams, MapNormalsParams, MapPlaneInfo
    dst, dr = _hand(mc.line())
    src, sr = _hand(mc.patch())
    w = _check(dst, mpr.Target(dr, F(VOXEL)), src, sr, [I4], "no normals")[0]
    assert (w.matched, w.considered, w.dst_normals) == (0, 9, 0) and not any(w.S)
    L = _lib.lib()
    T = np.ascontiguousarray(I4.T).reshape(16)
    Tp = T.ctypes.data_as(C.POINTER(C.c_float))
    out = MapPlaneInfo()
    p = MapAlignParams()
    p.max_dist, p.min_count_dst, p.min_count_src = VOXEL, 2, 1
    assert L.revo_map_align_plane_eval(dst._h, src._h, 1, Tp, C.byref(p), C.byref(MapNormalsParams(2, 5, 0.1, 0.1)), C.byref(out), 0) == 0
    assert L.revo_map_align_plane_eval(dst._h, src._h, 1, Tp, C.byref(p), None, C.byref(out), 0) == 0
    assert L.revo_map_align_plane_eval(dst._h, src._h, 1, Tp, C.byref(p), C.byref(MapNormalsParams(1, 5, 0.1, 0.1)), C.byref(out), 0) == INVALID_ARG
    assert L.revo_map_align_plane_eval(dst._h, src._h, 1, Tp, C.byref(p), C.byref(MapNormalsParams(2, 2, 0.1, 0.1)), C.byref(out), 0) == INVALID_ARG
    assert L.revo_map_align_plane_eval(dst._h, src._h, 0, Tp, C.byref(p), None, C.byref(out), 0) == INVALID_ARG
    assert L.revo_map_align_plane_eval(dst._h, None, 1, Tp, C.byref(p), None, C.byref(out), 0) == INVALID_ARG


def test_align_plane_follows_the_specification_loop():
    from revo_amd import api
    dst, src = _build(True), _build(True, "small")
    sr = _records(True, "small")
    c = mar.default_centre(sr, I4)
    got = dst.align_plane(src, centre=c)
    T, info, it, status = mpr.align_plane(_target(True), F(VOXEL), sr, I4, F(VOXEL), centre=c)
    dt = float(np.linalg.norm(got["T"][:3, 3].astype(np.float64) - T[:3, 3]))
    da = synth.rot_angle(got["T"][:3, :3], T[:3, :3])
    print("device %d iterations, status %d; specification %d, %d; poses differ by %.3g m, %.3g rad"
          % (got["iterations"], got["status"], it, status, dt, da))
    assert dt < 1e-5 and da < 1e-5  # the project's pose-parity tolerance
    assert (got["iterations"], got["status"]) == (it, status) and status == ALIGN_CONVERGED and it > 2
    assert bytes(got["info"]) == bytes(mpr.align_plane_eval(_target(True), sr, got["T"], F(VOXEL), centre=c))
    H, _ = mpr.system(got["info"])
    s2 = got["sigma2"]
    assert s2 == float(got["info"].S[27]) / (got["info"].matched - 6) and np.allclose(got["cov"] @ H, s2 * np.eye(6), atol=1e-9 * s2 + 1e-15)
    Ha, ga = api.align_plane_system(got["info"])
    assert np.array_equal(Ha, H) and np.array_equal(ga, mpr.system(got["info"])[1])
    assert dst.align_plane(src, centre=c, max_iters=2)["status"] == 1
    # a single plane leaves H rank-deficient: lost at the first system
    flat, _ = _hand(mc.plane_grid())
    flat_src, fr = _hand(mc.plane_grid(shift=(2.0 ** -9, 0.0, 2.0 ** -9)))
    lost = flat.align_plane(flat_src, centre=mar.default_centre(fr, I4))
    assert lost["status"] == ALIGN_LOST and lost["iterations"] == 0 and lost["T"].tobytes() == I4.tobytes() and lost["info"].matched >= 300


def test_plane_ladder_recovers_the_twist():
    from revo_amd import api
    dst, src = _build(True), _build(True, "ladder")
    r = api.align_maps(dst, src, metric="plane")
    E = r["T"].astype(np.float64) @ D_LADDER
    et, er = float(np.linalg.norm(E[:3, 3])), synth.rot_angle(np.eye(3), E[:3, :3])
    print("plane ladder: %s iterations, status %d, %d of %d matched, error %.3g m %.3g rad (bounds %.3g, %.3g)"
          % ([lv["iterations"] for lv in r["levels"]], r["status"], r["info"].matched, r["info"].considered, et, er,
             PLANE_LADDER_ERR_T, PLANE_LADDER_ERR_R))
    assert r["status"] == ALIGN_CONVERGED and len(r["levels"]) == 3 and r["info"].dst_normals > 1000
    assert et < PLANE_LADDER_ERR_T and er < PLANE_LADDER_ERR_R


def test_the_default_metric_is_unchanged():
    from revo_amd import api
    dst, src = _build(False), _build(False, "ladder")
    r = api.align_maps(dst, src)
    T, c = I4, r["centre"]
    for sh, lv in zip((2, 1, 0), r["levels"]):
        d, s = (dst, src) if sh == 0 else (dst.coarsen(sh), src.coarsen(sh))
        one = d.align(s, T, max_dist=d.voxel, centre=c)
        assert one["T"].tobytes() == lv["T"].tobytes() and bytes(one["info"]) == bytes(lv["info"])
        assert (one["iterations"], one["status"]) == (lv["iterations"], lv["status"])
        T = one["T"]
    assert C.sizeof(r["info"]) == 160 and r["T"].tobytes() == T.tobytes()
    assert api.align_maps(dst, src, metric="point")["T"].tobytes() == T.tobytes()
    with pytest.raises(ValueError):
        api.align_maps(dst, src, metric="planes")


def test_save_ply_with_normals(tmp_path):
    m = _build(True)
    a, b, c = (str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply"))
    m.save_ply(a)
    ply.write_voxel_ply(b, *m.points())
    assert open(a, "rb").read() == open(b, "rb").read()  # without normals: the existing writer's bytes
    m.save_ply(c, normals=True)
    xyz, rgb, cnt, nv = ply.read_voxel_ply_normals(c)
    pts, want = m.points(), m.normals()
    assert xyz.tobytes() == pts[0].tobytes() and rgb.tobytes() == pts[1].tobytes() and cnt.tobytes() == pts[2].tobytes()
    assert nv.tobytes() == want[1].tobytes() and np.any(nv)
    raw = open(c, "rb").read()
    assert b"property float nx\nproperty float ny\nproperty float nz\nend_header\n" in raw[:400]
    with pytest.raises(ValueError):
        ply.read_voxel_ply(c)
