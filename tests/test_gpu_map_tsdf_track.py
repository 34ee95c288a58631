"""Tracking a depth frame against the TSDF surface on the device (revo_map_tsdf_track_eval / revo_map_tsdf_track, api.VoxelMap.surface_track_eval
/ surface_track, api.TsdfVolume.track, api.SurfaceVolume.track, api.MapWindow, vo.REVO(surface_track=), run_tum --surface-track):
the records bit for bit revo_amd.mapfile's restatement (which test_map_tsdf_track_cpu.py pins to the per-pixel loop) on the shared cases,
with the volume, the frame and the output each in host and in device memory; the pyramid form against the raw image; the same bytes
whatever the number of workgroups; every argument error with sentinel-filled outputs; the loop equal to mapfile.tsdf_track; the device
volumes of a running sequence; the window; the driver and the command."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile  # noqa: E402
from revo_amd.settings import MapAlignOpts, MapCarveView, MapTsdfTrackInfo, MapTsdfTrackParams  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_tsdf_track_cases as kc  # noqa: E402
import test_gpu_map_raycast as tr  # noqa: E402
import test_gpu_map_tsdf as tt  # noqa: E402

F = np.float32
INVALID_ARG = -1
REC = 208
FILL = 0x2B
vp = C.c_void_p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = ((False, False, False), (True, True, True), (True, False, True), (False, True, False))  # (device volume, device frame, device output)
f32p = C.POINTER(C.c_float)


def _frame(depth, camera, zrange, device):
    """One revo_map_carve_view of a raw depth image; its pose is filled with NaN: it is not read."""
    import torch
    v = MapCarveView()
    if device:
        keep = torch.from_numpy(np.ascontiguousarray(depth, F)).cuda()
        v.depth = keep.data_ptr()
        torch.cuda.synchronize()
    else:
        keep = np.ascontiguousarray(depth, F)
        v.depth = keep.ctypes.data
    v.height, v.width = depth.shape
    v.fx, v.fy, v.cx, v.cy = [float(x) for x in camera]
    v.zmin, v.zmax = [float(x) for x in zrange]
    v.T_w_c[:] = [float("nan")] * 16
    return v, keep


def _call(m, c, device_tsdf=False, device_in=False, device_out=False, raw=None, poses=None):
    """revo_map_tsdf_track_eval on a case with the volume, the frame and the output on either side, the output filled with FILL bytes
    first -> (return code, the records as a mapfile.TSDF_TRACK_DTYPE array).  raw: a dict that replaces arguments of the call."""
    import torch
    L = _lib.lib()
    raw = raw or {}
    poses = c["poses"] if poses is None else np.asarray(poses, F).reshape(-1, 4, 4)
    n = len(poses)
    box = tt._box(c["lo"], c["cells"].shape)
    if device_tsdf:
        vol = tt._as_tensor(c["cells"])
        p_vol = vp(vol.data_ptr())
    else:
        vol = np.ascontiguousarray(c["cells"])
        p_vol = vol.ctypes.data_as(vp)
    frame, keep = _frame(c["depth"], c["camera"], c["zrange"], device_in)
    flat = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(T.T).reshape(16) for T in poses]), F)
    prm = MapTsdfTrackParams()
    prm.max_dist, prm.stride, prm.min_weight = 0.0 if c["max_dist"] is None else float(c["max_dist"]), int(c["stride"]), int(c["min_weight"])
    prm.centre[:] = [0.0, 0.0, 0.0] if c["centre"] is None else [float(x) for x in c["centre"]]
    rows = max(n, 1) + 1  # an argument error with a refused nposes still has an output to look at
    if device_out:
        out = torch.full((rows * REC,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        p_out = vp(out.data_ptr())
    else:
        out = np.full(rows * REC, FILL, np.uint8)
        p_out = out.ctypes.data_as(vp)
    a = dict(m=m._h, box=C.byref(box), tsdf=p_vol, device_tsdf=1 if device_tsdf else 0, trunc=float(c["trunc"]), frame=C.byref(frame), device_in=1 if device_in else 0,
             nposes=n, T=flat.ctypes.data_as(f32p), prm=C.byref(prm), out=p_out, device_out=1 if device_out else 0)
    a.update({k: x for k, x in raw.items() if k in a})
    code = L.revo_map_tsdf_track_eval(a["m"], a["box"], a["tsdf"], a["device_tsdf"], a["trunc"], a["frame"], a["device_in"], a["nposes"], a["T"], a["prm"], a["out"],
                                      a["device_out"])
    m.sync()
    if device_out:
        torch.cuda.synchronize()
        out = out.cpu().numpy()
    del keep, vol
    return code, out


def _records(out, n):
    assert np.all(out[n * REC:] == FILL), "written past the records"
    return np.frombuffer(out[:n * REC].tobytes(), mapfile.TSDF_TRACK_DTYPE)


@functools.lru_cache(maxsize=None)
def _want(name):
    a, kw = kc.args(kc.cases()[name])
    return mapfile.tsdf_track_records(*a, **kw)


# ---------------------------------------------------------------------------------------------------------------- the cases --
@pytest.mark.parametrize("name", list(kc.cases()))
def test_cases_bit_exact(name):
    c = kc.cases()[name]
    want = _want(name)
    m = tt._map(voxel=c["voxel"])
    for sides in SIDES:
        code, out = _call(m, c, *sides)
        assert code == 0, (sides, _lib.lib().revo_last_error())
        got = _records(out, len(want))
        assert got.tobytes() == want.tobytes(), (name, sides, [(int(g["matched"]), int(w["matched"])) for g, w in zip(got, want)])
    print(name, [(int(r["matched"]), int(r["considered"]), int(r["skipped"])) for r in want][:4])
    m.close()


def test_a_pose_alone_and_among_others():
    c = kc.cases()["65 poses"]
    want = _want("65 poses")
    m = tt._map()
    for i in (0, 7, 33, 64):
        code, out = _call(m, c, True, True, True, poses=c["poses"][i])
        assert code == 0 and _records(out, 1).tobytes() == want[i:i + 1].tobytes(), i
    m.close()


def test_the_pyramid_form_is_the_raw_image():
    """A pyramid's level-0 depth plane as the frame: the records of the same plane passed as a raw image, with the context's camera by
    six zeros and by its own numbers, and mapfile's."""
    _, cam, pyrs, _ = tr._scene()
    cells, lo, trunc, views = kc.scene()
    m = tt._map(voxel=cc.VOXEL)
    k = cc.intrinsics320()
    poses = [views[0][1], kc.scene_starts()[0]["tr1 y"]]
    centre = kc.scene_centre()
    plane = pyrs[0].returnDepth(0).copy()
    kw = dict(stride=2, centre=centre)
    got = m.surface_track_eval(cells, lo, trunc, pyrs[0], poses, **kw)
    raw0 = m.surface_track_eval(cells, lo, trunc, (plane, None), poses, **kw)
    raw1 = m.surface_track_eval(cells, lo, trunc, (plane, k[:4], k[4:]), poses, **kw)
    want = mapfile.tsdf_track_records(cells, lo, cc.VOXEL, trunc, plane, k[:4], k[4:], poses, **kw)
    as_bytes = lambda recs: b"".join(bytes(r) for r in recs)  # noqa: E731
    assert as_bytes(got) == as_bytes(raw0) == as_bytes(raw1) == want.tobytes() and want["matched"][0] > 500
    m.close()


CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_map_tsdf_track as t
import map_tsdf_track_cases as kc
import test_gpu_map_tsdf as tt
m = tt._map()
for name in %r:
    code, out = t._call(m, kc.cases()[name], True, True, True)
    assert code == 0
    print(name, bytes(out).hex())
"""
GROUP_CASES = ("64x48 stride 1", "33x17 stride 2", "65 poses", "the gate at equality")


def test_the_workgroups_do_not_show():
    """REVO_MAP_TSDF_TRACK_GROUPS=1, 3 and the default (12 for the 64 x 48 image, which has 12 blocks), each in a fresh process: the same
    bytes, mapfile's."""
    outs = []
    for groups in ("1", "3", None):
        env = dict(os.environ)
        env.pop("REVO_MAP_TSDF_TRACK_GROUPS", None)
        if groups is not None:
            env["REVO_MAP_TSDF_TRACK_GROUPS"] = groups
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), GROUP_CASES)], capture_output=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(dict(ln.rsplit(" ", 1) for ln in r.stdout.decode().splitlines() if ln.rsplit(" ", 1)[0] in GROUP_CASES))
    assert outs[0] == outs[1] == outs[2] and set(outs[0]) == set(GROUP_CASES)
    for name in GROUP_CASES:
        want = _want(name)
        assert bytes.fromhex(outs[0][name])[:len(want) * REC] == want.tobytes(), name


def test_argument_errors_write_nothing():
    import torch
    c = kc.cases()["3x5x7 lo < 0"]
    m = tt._map()

    def prm(md=0.0, stride=1, mw=1, centre=(0.0, 0.0, 0.0), res=(0, 0)):
        p = MapTsdfTrackParams(md, stride, mw, (C.c_float * 3)(*centre), (C.c_uint32 * 2)(*res))
        return dict(prm=C.byref(p), _keep=p)

    def box(lo, n):
        b = tt._box(lo, n)
        return dict(box=C.byref(b), _keep=b)

    def frame(**kw):
        v, keep = _frame(c["depth"], c["camera"], c["zrange"], False)
        for k, x in kw.items():
            setattr(v, k, x)
        return dict(frame=C.byref(v), _keep=(v, keep))

    nan, inf = float("nan"), float("inf")
    raws = [dict(m=None), dict(box=None), dict(tsdf=None), dict(frame=None), dict(T=None), dict(out=None), dict(nposes=0), dict(nposes=4097), dict(nposes=-1),
            dict(device_tsdf=2), dict(device_in=-1), dict(device_out=2), dict(trunc=0.0), dict(trunc=-0.5), dict(trunc=nan), dict(trunc=inf),
            prm(md=-0.1), prm(md=nan), prm(md=inf), prm(md=float(np.nextafter(F(c["trunc"]), F(9)))), prm(stride=9), prm(centre=(0.0, nan, 0.0)),
            prm(centre=(inf, 0.0, 0.0)), prm(res=(1, 0)), prm(res=(0, 1)),
            box(c["lo"], (0, 5, 7)), box(c["lo"], (3, 5, 1025)), box(((1 << 20) - 2, 0, 0), (3, 5, 7)), box((0, 0, 0), (1024, 1024, 256)),
            frame(depth=None), frame(width=0), frame(height=2049), frame(fx=0.0), frame(fy=-1.0), frame(cx=nan), frame(zmin=1.0, zmax=1.0), frame(zmin=-0.5),
            frame(zmax=inf)]
    for sides in ((False, False, False), (True, False, True)):
        for raw in raws:
            code, out = _call(m, c, *sides, raw=raw)
            shown = {x: y for x, y in raw.items() if x != "_keep"}
            assert code == INVALID_ARG, (sides, shown)
            assert np.all(out == FILL), (sides, shown)
    # misaligned device pointers: the volume and the output to 16 bytes, the image to 4
    d = torch.zeros(4096, dtype=torch.float32, device="cuda")
    vol = tt._as_tensor(c["cells"])
    img = torch.from_numpy(c["depth"]).cuda()
    torch.cuda.synchronize()
    assert _call(m, c, True, True, True, raw=dict(tsdf=vp(vol.data_ptr() + 8)))[0] == INVALID_ARG
    assert _call(m, c, True, True, True, raw=dict(out=vp(d.data_ptr() + 8)))[0] == INVALID_ARG
    assert _call(m, c, True, True, True, raw=frame(depth=img.data_ptr() + 2))[0] == INVALID_ARG
    assert _call(m, c, True, True, True, raw=dict(out=vp(d.data_ptr())))[0] == 0
    # the frame's pose is not read: NaN there is no error (every call above had it); the defaults by NULL parameters
    code, out = _call(m, dict(c, centre=None), raw=dict(prm=None))
    assert code == 0 and _records(out, 1).tobytes() == mapfile.tsdf_track_records(*kc.args(c)[0]).tobytes()
    # revo_map_tsdf_track's own: a T_init that is not finite, max_iters < 1, NULL outputs
    L = _lib.lib()
    b = tt._box(c["lo"], c["cells"].shape)
    v, keep = _frame(c["depth"], c["camera"], c["zrange"], False)
    cells = np.ascontiguousarray(c["cells"])
    T0, T1 = np.eye(4, dtype=F).reshape(16), np.full(16, 7.0, F)
    info, it, st = MapTsdfTrackInfo(), C.c_int32(77), C.c_int32(77)
    bad_T = T0.copy()
    bad_T[12] = nan
    loop = lambda T=T0, opt=None, out=T1, status=st: L.revo_map_tsdf_track(  # noqa: E731
        m._h, C.byref(b), cells.ctypes.data_as(vp), 0, float(c["trunc"]), C.byref(v), 0, None if T is None else T.ctypes.data_as(f32p), None,
        None if opt is None else C.byref(opt), None if out is None else out.ctypes.data_as(f32p), C.byref(info), C.byref(it), None if status is None else C.byref(status))
    for kw in (dict(T=bad_T), dict(T=None), dict(out=None), dict(status=None), dict(opt=MapAlignOpts(0, 0, 1e-6, 1e-6, 12))):
        assert loop(**kw) == INVALID_ARG and np.all(T1 == 7.0) and it.value == 77 and st.value == 77, list(kw)
    assert loop() == 0 and st.value in (0, 1, 2)
    # the API's own checks
    with pytest.raises(ValueError):
        m.surface_track_eval(c["cells"].view(np.int64), c["lo"], c["trunc"], (c["depth"], c["camera"], c["zrange"]), np.eye(4))
    with pytest.raises(ValueError):
        m.surface_track_eval(c["cells"], c["lo"], c["trunc"], (c["depth"],), np.eye(4))
    with pytest.raises(ValueError):
        m.surface_track_eval(c["cells"], c["lo"], c["trunc"], (c["depth"], None, c["zrange"]), np.eye(4))
    with pytest.raises(ValueError):
        api.TsdfVolume(c["cells"], c["lo"], 0.5, c["trunc"]).track((c["depth"], c["camera"], c["zrange"]), np.eye(4), map=m)  # another voxel edge
    with pytest.raises(api.RevoError):
        m.surface_track(c["cells"], c["lo"], c["trunc"], (c["depth"], c["camera"], c["zrange"]), np.eye(4), stride=9)
    m.close()


# ----------------------------------------------------------------------------------------------------------------- the loop --
STARTS = ("t1 x", "r2 y", "tr2 z")


def _same_track(got, want, what):
    T, rec, it, status = want
    assert got["T"].tobytes() == T.tobytes(), (what, got["T"], T)
    assert bytes(got["info"]) == rec.tobytes(), what
    assert (got["iterations"], got["status"]) == (it, status), (what, got["iterations"], got["status"], it, status)


def test_the_loop_is_mapfiles():
    """revo_map_tsdf_track / api.TsdfVolume.track on the scene box from three of the convergence table's starts: the pose, the record,
    the iterations and the status are mapfile.tsdf_track's exactly -- the loop is double on the host over identical records."""
    cells, lo, trunc, views = kc.scene()
    k = cc.intrinsics320()
    starts, truth = kc.scene_starts()
    centre = kc.scene_centre()
    m = tt._map(voxel=cc.VOXEL)
    vol = api.TsdfVolume(cells, lo, cc.VOXEL, trunc, map=m)
    frame = (views[0][0], k[:4], k[4:])
    for name in STARTS:
        want = mapfile.tsdf_track(cells, lo, cc.VOXEL, trunc, views[0][0], k[:4], k[4:], starts[name], centre=centre)
        got = vol.track(frame, starts[name], centre=centre)
        _same_track(got, want, name)
        assert got["status"] == mapfile.ALIGN_CONVERGED and got["cov"] is not None and got["cov"].shape == (6, 6) and got["sigma2"] > 0
        assert got["centre"].tobytes() == centre.tobytes()
    # the default centre is the middle of the box; the options reach the loop
    want = mapfile.tsdf_track(cells, lo, cc.VOXEL, trunc, views[0][0], k[:4], k[4:], starts["t1 x"], stride=2, max_iters=3)
    got = vol.track(frame, starts["t1 x"], stride=2, max_iters=3)
    _same_track(got, want, "three iterations")
    assert got["iterations"] == 3 and got["status"] == mapfile.ALIGN_ITER_LIMIT and got["centre"].tobytes() == mapfile.tsdf_track_centre(lo, cells.shape, cc.VOXEL).tobytes()
    # track_eval: one pose gives one record, several a list; the system is the host function's
    recs = vol.track_eval(frame, [starts[n] for n in STARTS], centre=centre)
    wr = mapfile.tsdf_track_records(cells, lo, cc.VOXEL, trunc, views[0][0], k[:4], k[4:], [starts[n] for n in STARTS], centre=centre)
    assert b"".join(bytes(r) for r in recs) == wr.tobytes()
    one = vol.track_eval(frame, starts["r2 y"], centre=centre)
    assert bytes(one) == wr[1:2].tobytes()
    H, g = api.tsdf_track_system(one)
    Hw, gw = mapfile.df_align_system(wr[1])
    assert np.array_equal(H, Hw) and np.array_equal(g, gw)
    # the wall alone is rank-deficient: LOST, the pose stays
    w = kc.cases()["wall"]
    mw = tt._map()
    got = api.TsdfVolume(w["cells"], w["lo"], w["voxel"], w["trunc"], map=mw).track((w["depth"], w["camera"], w["zrange"]), w["poses"][1], min_matched=6)
    assert got["status"] == mapfile.ALIGN_LOST and got["iterations"] == 0 and got["T"].tobytes() == w["poses"][1].tobytes()
    mw.close()
    m.close()


def test_the_device_volumes_of_a_running_sequence():
    """api.SurfaceVolume.track / track_eval on the device volume: the host-volume call's results, without a host copy."""
    import torch
    lo, n, views = kc.tc.scene64()
    k = cc.intrinsics320()
    starts, truth = kc.scene_starts()
    centre = kc.scene_centre()
    m = tt._map(voxel=cc.VOXEL)
    surf = api.SurfaceVolume(m, lo, n, color=False)
    for d, T, kk in views:
        surf.integrate((torch.from_numpy(d).cuda(), T, kk))
    d_frame = torch.from_numpy(views[0][0]).cuda()
    d_out = torch.zeros(2 * REC, dtype=torch.uint8, device="cuda")
    poses = [starts["t1 x"], starts["tr2 z"]]
    assert surf.track_eval((d_frame, k[:4], k[4:]), poses, centre=centre, d_out=d_out) is None  # enqueued behind the four fuse calls
    got = surf.track((d_frame, k[:4], k[4:]), starts["tr2 z"], centre=centre)
    vol = surf.volume()
    assert vol.cells.tobytes() == kc.scene()[0].tobytes()
    host = vol.track((views[0][0], k[:4], k[4:]), starts["tr2 z"], centre=centre)
    assert got["T"].tobytes() == host["T"].tobytes() and bytes(got["info"]) == bytes(host["info"])
    assert (got["iterations"], got["status"]) == (host["iterations"], host["status"]) and got["status"] == mapfile.ALIGN_CONVERGED
    want = mapfile.tsdf_track_records(vol.cells, lo, cc.VOXEL, vol.trunc, views[0][0], k[:4], k[4:], poses, centre=centre)
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    m.close()


def test_the_window_forwards():
    _, cam, _, _ = tr._scene()
    c = kc.cases()["sphere"]
    win = api.MapWindow(cam, c["voxel"], dense=True, window=2)
    frame = (c["depth"], c["camera"], c["zrange"])
    recs = win.surface_track_eval(c["cells"], c["lo"], c["trunc"], frame, c["poses"], centre=c["centre"])
    assert b"".join(bytes(r) for r in recs) == _want("sphere").tobytes()
    got = win.surface_track(c["cells"], c["lo"], c["trunc"], frame, c["poses"][1], centre=c["centre"])
    _same_track(got, mapfile.tsdf_track(c["cells"], c["lo"], c["voxel"], c["trunc"], c["depth"], c["camera"], c["zrange"], c["poses"][1], centre=c["centre"]), "window")
    win.close()


def test_interleaved_with_the_calls_that_share_the_host_volumes_buffer():
    """A host volume goes through the handle's tsdfvol, which fuse, mesh and the surface ray cast stage through too: on one handle, in
    both sizes of map_shared_cases and in every order of two, each call gives what it gives alone (map_shared_cases' rule)."""
    import map_shared_cases as ms

    def track(m, size):
        cells, _ = ms.tsdf_volume(size)
        cam, (w, h) = ms.BOX_CAM[size]
        depth = np.full((h, w), 0.98, F) + (np.arange(w, dtype=F) / F(w))[None, :] * F(0.06)  # a ramp through both boxes, 0.96 .. 1.06 m deep
        recs = m.surface_track_eval(cells, ms.BOX[size][0], mapfile.tsdf_trunc(ms.VOXEL), (depth, cam, ms.ZR), np.stack(ms.POSES[:ms.NV[size]]),
                                    max_dist=float(mapfile.tsdf_trunc(ms.VOXEL)))
        return [bytes(r) for r in recs]

    others = {name: ms.FEATURES[name] for name in ("fuse", "mesh", "surface_raycast", "surface_raycast_plain", "fuse_color", "mesh_attr")}
    alone = {}
    for size in ms.SIZES:
        for name, fn in list(others.items()) + [("track", track)]:
            m = tt._map(ms.base_records(), ms.VOXEL)
            alone[name, size] = fn(m, size)
            m.close()
        assert any(int(np.frombuffer(r, mapfile.TSDF_TRACK_DTYPE)["matched"][0]) > 0 for r in alone["track", size]), size
    m = tt._map(ms.base_records(), ms.VOXEL)
    for big, small in (("large", "small"), ("small", "large")):
        for name, fn in others.items():
            assert fn(m, big) == alone[name, big], (name, big)
            assert track(m, small) == alone["track", small], (name, "then track", small)
            assert track(m, big) == alone["track", big], (name, "then track", big)
            assert fn(m, small) == alone[name, small], ("track then", name, small)
    m.close()


# --------------------------------------------------------------------------------------------------------------- the driver --
def _run_sequence(surface_track):
    from lm_settings_cases import S160
    from revo_amd import vo
    import test_gpu_map_surface as ts
    frames = ts._two_keyframes(S160)
    cam = api.CameraPyr(S160)
    vm = api.VoxelMap(cam, 0.05, dense=True)
    surf = api.SurfaceVolume(vm, (-40, -40, 0), (80, 80, 100))
    g = vo.REVO(S160, cameraPyr=cam, voxelMap=vm, surface=surf, surface_track=surface_track)
    kfs = 0
    for f in frames:
        _, kf = g.push(f[0], f[1], f[2])
        kfs += int(kf)
        if kfs == 2:
            break
    out = (g, [(ts_, T.copy()) for ts_, T in g.poses], vm.export_raw().tobytes(), surf.volume(), kfs)
    g.truth = {float(f[2]): np.linalg.inv(np.asarray(frames[0][3], np.float64)) @ np.asarray(f[3], np.float64) for f in frames}  # the sequence's own poses
    return out, vm


def test_the_driver_tracks_every_keyframe():
    """vo.REVO(surface=s, surface_track=True): one entry per keyframe, the first LOST against the empty volume, the later ones CONVERGED;
    the reported poses and the voxel map are those of the run without it, byte for byte; off, the surface is the parent's."""
    from revo_amd import vo
    (g, poses, raw, vol, kfs), vm = _run_sequence(True)
    (g0, poses0, raw0, vol0, kfs0), vm0 = _run_sequence(None)
    assert kfs == kfs0 == 2 == len(g.surface_tracks) and g0.surface_tracks == [] and g0.surface_track is None
    assert [s for *_, s in g.surface_tracks] == [mapfile.ALIGN_LOST] + [mapfile.ALIGN_CONVERGED] * (kfs - 1)
    ts0, T0, Tf0, info0, _ = g.surface_tracks[0]
    assert info0.matched == 0 and Tf0.tobytes() == T0.tobytes()  # the empty volume: nothing matches, the keyframe is fused where the tracker has it
    ts1, T1, Tf1, info1, _ = g.surface_tracks[1]
    print("keyframe 2: %d of %d pixels matched, moved %.2e m %.2e rad" % ((info1.matched, info1.considered) + kc.pose_error(Tf1, T1)))
    print("keyframe 2 against the sequence's own pose: the tracker's %.2e m %.2e rad, the refined %.2e m %.2e rad"
          % (kc.pose_error(T1, g.truth[float(ts1)]) + kc.pose_error(Tf1, g.truth[float(ts1)])))
    assert info1.matched > 1000 and ts1 > ts0
    assert len(poses) == len(poses0) and all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(poses, poses0))
    assert raw == raw0
    # off: the parent's surface -- the two keyframes fused at the tracker's poses; on: the second one at the refined pose
    (_, _, _, again, _), vm1 = _run_sequence(False)
    assert again.cells.tobytes() == vol0.cells.tobytes() and again.color.tobytes() == vol0.color.tobytes()
    if Tf1.tobytes() == T1.tobytes():
        assert vol.cells.tobytes() == vol0.cells.tobytes()
    with pytest.raises(ValueError):
        vo.REVO(g.settingsPyr, cameraPyr=g.camPyr, voxelMap=vm, surface_track=True)  # without a surface
    for v in (vm, vm0, vm1):
        v.close()


def test_run_tum_surface_track(tmp_path, monkeypatch, capsys):
    from lm_settings_cases import S160
    from revo_amd import run_tum, tum
    import test_gpu_map_surface as ts
    from test_gpu_vo_multi import _tum_yaml
    name = "rgbd_synth_s"
    tum.write_synthetic_dataset(str(tmp_path / "data" / name), ts._two_keyframes(S160)[:12])
    _tum_yaml(tmp_path, S160, [name])
    monkeypatch.chdir(tmp_path)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "0", "--map", "0.05"]
    surface = ["--surface", "surface.ply", "--surface-box", "-40", "-40", "0", "80", "80", "100", "--surface-trunc", "0.2"]
    assert run_tum.main(args + surface + ["--surface-track"]) == 0
    out = capsys.readouterr().out
    assert "Surface track:" in out
    listed = tum.read_poses(str(tmp_path / ("surface_poses_%s.txt" % name)))
    notes = [ln.split() for ln in open(str(tmp_path / ("surface_poses_%s.txt" % name))) if ln.startswith("# ") and ln.split()[1][0].isdigit()]
    assert len(listed) == len(notes) >= 1 and notes[0][-1] == "lost"
    assert np.allclose(listed[0][1], np.eye(4), atol=1e-6)  # the first keyframe: lost against the empty volume, fused where the tracker has it
    assert run_tum.main(args + ["--surface-track"]) == 2  # without --surface
    capsys.readouterr()
