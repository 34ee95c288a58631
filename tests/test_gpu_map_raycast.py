"""Rays through the voxel map on the device (revo_map_raycast / revo_map_cast_rays, api.VoxelMap.raycast / raycast_into /
cast_rays): depth bytes, colour bytes, keys, hits and the info record bit for bit revo_amd.mapfile's restatement
(which test_map_raycast_cpu.py pins to the per-ray loop) -- hand-made maps whose keys share slots, tiny views, one case per rule
of the march, the 35 000-voxel scene --, from the host and from the device side; the same bytes whatever the order of the
records, the table size, the batching of views, the output side and the block table; the map is not changed; stream order
behind an integration; every argument error; and run_tum --map-views-raycast."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile, synth  # noqa: E402
from revo_amd.settings import MapRayInfo, MapRayParams, MapView  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_raycast_cases as rc  # noqa: E402
import map_records_ref as mrr  # noqa: E402
import voxel_map_ref as ref  # noqa: E402

F = np.float32
RAW = mapfile.RAW_DTYPE
INVALID_ARG = -1
I4 = cc.I4
VOXEL = cc.VOXEL
V = rc.V
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("depth", "bgr", "key")


@functools.lru_cache(maxsize=None)
def _scene():
    """The context, the pyramids of views 0 .. 2 of the scene as built, and their dense level-0 clouds."""
    from revo_amd import api
    s = cc.settings320()
    cam = api.CameraPyr(s)
    pyrs = [api.ImgPyramidRGBD(s, cam, *cc.scene_frames()[0][i]) for i in (0, 1, 2)]
    clouds = [ref.points_from_pcl(p.generateColoredPcl(0, True)) for p in pyrs]
    return api, cam, pyrs, clouds


def _kf_poses():
    return [T.astype(F) for T in cc.poses()[:3]]


@functools.lru_cache(maxsize=None)
def _scene_records(n=2):
    r = ref.VoxelMapRef(VOXEL)
    for (xyz, rgb), T in list(zip(_scene()[3], _kf_poses()))[:n]:
        r.integrate(xyz, rgb, T)
    return mrr.records_of(r).astype(RAW)


def _scene_views():
    """The map's own two keyframe poses with the context's camera, and a half-resolution camera at a third pose."""
    s = cc.settings320()
    k = cc.intrinsics320()
    half = (s.fx * 0.45, s.fy * 0.55, s.width * 0.26, s.height * 0.23, s.depth_min, s.depth_max)
    P = _kf_poses()
    return [(P[0], k, (s.width, s.height)), (P[1], k, (s.width, s.height)), (P[2], half, (s.width // 2, s.height // 2))]


@functools.lru_cache(maxsize=None)
def _scene_spec():
    """The restatement on the scene map from the three views, computed once."""
    return mapfile.raycast_records(_scene_records(), VOXEL, _scene_views())


def _hand(rec, voxel=VOXEL, **kw):
    api, cam = _scene()[:2]
    m = api.VoxelMap(cam, voxel, **kw)
    if len(rec):
        m.merge_raw(rec.astype(RAW))
    return m


def _views(views, min_count=1):
    v = (MapView * len(views))()
    for x, (T, k, (w, h)) in zip(v, views):
        x.width, x.height = w, h
        x.fx, x.fy, x.cx, x.cy, x.zmin, x.zmax = [float(a) for a in k]
        x.T_w_c[:] = np.ascontiguousarray(np.asarray(T, F).T).reshape(16).tolist()
        x.splat_max, x.min_count = 77, min_count  # splat_max is not read
    return v


def _info(i):
    return {k: int(getattr(i, k)) for k in mapfile.RAY_INFO_KEYS}


def _cast(m, views, min_count=1, max_steps=4096, device=False):
    """revo_map_raycast with views of any sizes in one call, host or device outputs -> the dict mapfile.raycast_records gives
    (without s, cells, status)."""
    from revo_amd import _lib
    n = len(views)
    v = _views(views, min_count)
    prm = MapRayParams(max_steps)
    shapes = [(h, w) for _, _, (w, h) in views]
    if device:
        import torch
        dev = "cuda:%d" % m.cameraPyr.device
        t = {"depth": [torch.full(s, -1.0, dtype=torch.float32, device=dev) for s in shapes],
             "bgr": [torch.full(s + (3,), 7, dtype=torch.uint8, device=dev) for s in shapes],
             "key": [torch.full(s, 5, dtype=torch.int64, device=dev) for s in shapes]}
        hits = torch.full((n,), 9, dtype=torch.int32, device=dev)
        info = torch.full((8,), 9, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ptr = {k: (C.c_void_p * n)(*[a.data_ptr() for a in t[k]]) for k in OUT}
        _lib.check(_lib.lib().revo_map_raycast(m._h, n, v, C.byref(prm), ptr["depth"], ptr["bgr"], ptr["key"], C.c_void_p(hits.data_ptr()), 1,
                                               C.c_void_p(info.data_ptr())))
        m.sync()
        out = {k: [a.cpu().numpy() for a in t[k]] for k in OUT}
        out["key"] = [a.view(np.uint64) for a in out["key"]]
        out["hits"] = [int(x) for x in hits.cpu().numpy()]
        i = info.cpu().numpy()
        assert not i[6:].any()
        out["info"] = dict(zip(mapfile.RAY_INFO_KEYS, (int(x) for x in i[:6])))
        return out
    out = {"depth": [np.full(s, -1, F) for s in shapes], "bgr": [np.full(s + (3,), 7, np.uint8) for s in shapes],
           "key": [np.full(s, 5, np.uint64) for s in shapes]}
    hits = np.full(n, 9, np.uint32)
    info = MapRayInfo()
    ptr = {k: (C.c_void_p * n)(*[a.ctypes.data for a in out[k]]) for k in OUT}
    _lib.check(_lib.lib().revo_map_raycast(m._h, n, v, C.byref(prm), ptr["depth"], ptr["bgr"], ptr["key"], hits.ctypes.data_as(C.c_void_p), 0,
                                           C.byref(info)))
    assert not any(info.reserved)
    out["hits"], out["info"] = [int(x) for x in hits], _info(info)
    return out


def _assert_same(got, want, what):
    print("%s: hits %s, info %s" % (what, want["hits"], want["info"]))
    for k in OUT:
        assert len(got[k]) == len(want[k])
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, i, int(np.sum(a != b)))
    assert got["hits"] == want["hits"] and got["info"] == want["info"], (what, got["hits"], got["info"])


def _bytes(out):
    return b"".join(a.tobytes() for k in OUT for a in out[k]) + repr((out["hits"], out["info"])).encode()


def _check(m, rec, views, what, **kw):
    want = mapfile.raycast_records(rec.astype(RAW), m.voxel, views, **kw)
    _assert_same(_cast(m, views, **kw), want, what + ", host outputs")
    _assert_same(_cast(m, views, device=True, **kw), want, what + ", device outputs")
    return want


HAND_VIEWS = [(I4, cc.K16, (16, 12)), (I4, cc.K8, (8, 8)), (I4, cc.K64, (64, 64))]


def _tiny_views():
    T = synth.se3_exp(np.array([0.02, -0.03, 0.01, 0.05, -0.04, 0.02])).astype(F)
    return [(T, cc.K8, (1, 1)), (T, cc.K16, (1, 7)), (T, cc.K16, (9, 1))]


@pytest.mark.parametrize("initial_voxels", [1, 1 << 16], ids=["1024 slots", "default table"])
def test_views_hand_made_bit_exact(initial_voxels):
    rec = cc.filled_records()
    m = _hand(rec, initial_voxels=initial_voxels)
    if initial_voxels == 1:
        assert m.info()["capacity"] == 1024
        assert len(np.unique(cc.map_hash(rec["key"]) & np.uint64(1023))) < len(rec) - 50  # keys that share slots
    want = _check(m, rec, HAND_VIEWS, "K16, K8 and K64 in one call")
    assert all(h > 0 for h in want["hits"]) and want["info"]["rays"] == 192 + 64 + 4096
    _check(m, rec, _tiny_views(), "1 x 1, 1 x 7 and 9 x 1")
    _check(m, rec, HAND_VIEWS[:2], "min_count 3", min_count=3)
    for steps in (1, 2, 16, 40):
        w = _check(m, rec, HAND_VIEWS[:2] + _tiny_views(), "max_steps %d" % steps, max_steps=steps)
        assert w["info"]["exhausted"] > 0
    # the api: one pose, a list of poses (one library call), with and without keys
    want = mapfile.raycast_records(rec.astype(RAW), VOXEL, [HAND_VIEWS[0]] * 2)
    cam16 = cc.K16[:4] + (16, 12)
    d, b, h, k = m.raycast(I4, camera=cam16, zrange=cc.K16[4:], keys=True)
    assert (d.tobytes(), b.tobytes(), h, k.tobytes()) == (want["depth"][0].tobytes(), want["bgr"][0].tobytes(), want["hits"][0], want["key"][0].tobytes())
    assert m.ray_info == {n: x // 2 for n, x in want["info"].items()}
    ds, bs, hs = m.raycast([I4, I4], camera=cam16, zrange=cc.K16[4:])
    assert [a.tobytes() for a in ds] == [a.tobytes() for a in want["depth"]] and [a.tobytes() for a in bs] == [a.tobytes() for a in want["bgr"]]
    assert hs == want["hits"] and m.ray_info == want["info"] and m.last_raycast_ms() > 0


def test_raycast_into_and_the_window():
    import torch
    api, cam = _scene()[:2]
    rec = cc.filled_records()
    m = _hand(rec)
    want = mapfile.raycast_records(rec.astype(RAW), VOXEL, [HAND_VIEWS[0]] * 2)
    cam16 = cc.K16[:4] + (16, 12)
    d = torch.full((2, 12, 16), -1.0, device="cuda")
    b = torch.full((2, 12, 16, 3), 9, dtype=torch.uint8, device="cuda")
    k = torch.zeros((2, 12, 16), dtype=torch.int64, device="cuda")
    h = torch.zeros(4, dtype=torch.int32, device="cuda")
    i = torch.zeros(8, dtype=torch.int64, device="cuda")
    m.raycast_into(d, b, [I4, I4], camera=cam16, zrange=cc.K16[4:], d_keys=k, d_hits=h[:2], d_info=i)
    assert d.cpu().numpy().tobytes() == b"".join(a.tobytes() for a in want["depth"])
    assert b.cpu().numpy().tobytes() == b"".join(a.tobytes() for a in want["bgr"])
    assert k.cpu().numpy().tobytes() == b"".join(a.tobytes() for a in want["key"])
    assert h.cpu().numpy().tolist() == want["hits"] + [0, 0] and i.cpu().numpy().tolist()[:6] == [want["info"][n] for n in mapfile.RAY_INFO_KEYS]
    d1 = torch.full((12, 16), -1.0, device="cuda")  # one pose, depth only
    m.raycast_into(d1, None, I4, camera=cam16, zrange=cc.K16[4:])
    assert d1.cpu().numpy().tobytes() == want["depth"][0].tobytes()
    # MapWindow forwards to its inner map
    w = api.MapWindow(cam, VOXEL, window=2)
    w.map.merge_raw(rec.astype(RAW))
    got = w.raycast(I4, camera=cam16, zrange=cc.K16[4:])
    assert got[0].tobytes() == want["depth"][0].tobytes() and got[2] == want["hits"][0]
    rays = np.asarray([rc.ray((0, 0, 0.2), 0.0, (0, 0, 1), 3.0)], F)
    assert w.cast_rays(rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7])[4] == m.cast_rays(rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7])[4]
    w.close()


def _cast_rays(m, rays, **kw):
    rays = np.asarray(rays, F).reshape(-1, 8)
    return m.cast_rays(rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7], **kw)


def _same_rays(got, want, what):
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got[:4], want[:4])) and got[4] == want[4], (what, got, want)


def test_one_case_per_rule():
    from test_map_raycast_cpu import _check_ray_case
    maps = {}
    for case in rc.ray_cases():
        name, rows, ray, min_count, max_steps, _ = case
        rec = rc.records(rows).astype(RAW)
        m = maps.get(rec.tobytes()) or maps.setdefault(rec.tobytes(), _hand(rec, V, initial_voxels=1))
        want = mapfile.cast_rays_records(rec, V, np.asarray([ray], F), min_count, max_steps)
        for device in (False, True):
            got = _cast_rays(m, [ray], min_count=min_count, max_steps=max_steps, device=device)
            _same_rays(got, want, name)
            _check_ray_case(case, [x[0] for x in got[:4]])
    for name, rows, min_count, z in rc.view_cases():
        rec = rc.records(rows)
        m = _hand(rec, V, initial_voxels=1)
        want = _check(m, rec, [(I4, rc.VIEW_K, rc.VIEW_SIZE)], name, min_count=min_count)
        assert want["depth"][0][4, 4] == (F(z) if z is not None else 0)
    # the wall that is only 26-connected, and occlusion: the nearer voxel, and after it is subtracted the farther one
    rec = rc.wall_records()
    want = _check(_hand(rec, V), rec, [(I4, rc.WALL_K, rc.WALL_SIZE)], "the diagonal wall")
    assert all(want["depth"][0][y, x] > 0 for x, y in rc.wall_reaching_pixels())
    rec = rc.records([rc.cell(1, 0, 0, 2), rc.cell(3, 0, 0, 1)]).astype(RAW)
    m = _hand(rec, V)
    ray = rc.ray(rc.C0, 0.0, (1, 0, 0), 1.0)
    assert int(_cast_rays(m, [ray])[0][0]) == rc.key_of(1, 0, 0)
    m.subtract_raw(rec[rec["key"] == np.uint64(rc.key_of(1, 0, 0))])
    got = _cast_rays(m, [ray])
    assert (int(got[0][0]), got[1][0], int(got[2][0]), int(got[3][0])) == (rc.key_of(3, 0, 0), F(2.5 * V), 4, rc.HIT)


def _mixed_rays(n, seed):
    """n rays from around the origin towards voxels of the filled map, with the hand-made odd ones in between: not finite, empty, zero components."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.3, 0.3, (n, 3))
    xyz = mapfile.to_points(cc.filled_records().astype(RAW))[0]
    aim = xyz[rng.integers(0, len(xyz), n)] + rng.uniform(-0.03, 0.03, (n, 3))  # at a voxel or just past it
    d = (aim - o) * rng.uniform(0.5, 2.0, (n, 1))  # not normalised: the voxel lies at s = 0.5 .. 2
    rays = np.concatenate([o, rng.uniform(0.0, 0.2, (n, 1)), d, rng.uniform(0.4, 3.0, (n, 1))], 1).astype(F)
    odd = [c[2] for c in rc.ray_cases() if c[5][0] == rc.OUTSIDE and c[5][3] == 0]
    odd += [rc.ray((0.1, 0.1, 0.2), 0.0, (0, 0, 1), 3.0), rc.ray((0.1, 0.1, 0.2), 0.0, (0, 1, 0), 3.0), rc.ray((0.1, 0.1, 0.2), 0.0, (0, 0, 0), 3.0),
            rc.ray((0.1, 0.1, 3.0), 0.0, (-0.0, 0, -1), 3.0), rc.ray((0.1, 0.1, 0.2), 0.0, (1e-40, 0, 1), 3.0)]
    for i, r in enumerate(odd):
        if 3 * i + 1 < n:
            rays[3 * i + 1] = r
    return rays


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_cast_rays_bit_exact(n):
    rec = cc.filled_records().astype(RAW)
    m = _hand(rec, initial_voxels=1)
    rays = _mixed_rays(n, n)
    hits = 0
    for kw in (dict(), dict(max_steps=1), dict(max_steps=2), dict(max_steps=16), dict(min_count=3)):
        want = mapfile.cast_rays_records(rec, VOXEL, rays, **kw)
        _same_rays(_cast_rays(m, rays, **kw), want, "host")
        _same_rays(_cast_rays(m, rays, device=True, **kw), want, "device")
        hits += want[4]["hits"]
        assert ("max_steps" not in kw) or want[4]["exhausted"] > 0 or n == 1
    print(n, "rays:", want[4])
    assert hits > 0 or n == 1
    if n >= 63:
        assert want[4]["outside"] >= 10


CHILD = """
import sys
sys.path[:0] = %r
import numpy as np
from revo_amd import api, mapfile
import map_carve_cases as cc
import test_gpu_map_raycast as t
rec = cc.filled_records().astype(mapfile.RAW_DTYPE)
m = api.VoxelMap(api.CameraPyr(cc.settings320()), cc.VOXEL)
m.merge_raw(rec)
rays = t._mixed_rays(257, 257)
r = t._cast_rays(m, rays)
sys.stdout.buffer.write(t._bytes(t._cast(m, t.HAND_VIEWS + t._tiny_views())) + b"".join(a.tobytes() for a in r[:4]) + repr(r[4]).encode())
"""


def test_same_bytes_whatever_the_conditions():
    rec = cc.filled_records().astype(RAW)
    views = HAND_VIEWS + _tiny_views()
    m = _hand(rec, initial_voxels=16)
    base = _cast(m, views)
    rays = _mixed_rays(257, 257)
    base_rays = _cast_rays(m, rays)
    assert m.info()["capacity"] == 1024
    # the order of the records, and the initial table size
    rng = np.random.default_rng(3)
    shuffled = _hand(rec[rng.permutation(len(rec))], initial_voxels=16)
    big = _hand(rec, initial_voxels=1 << 22)
    assert big.info()["capacity"] >= 1 << 23
    for other in (shuffled, big):
        assert _bytes(_cast(other, views)) == _bytes(base)
        _same_rays(_cast_rays(other, rays), base_rays, "another table")
    big.close()
    # the batching of views: one call of three against three calls; the output side
    for i in range(3):
        one = _cast(m, views[i:i + 1])
        assert all(one[k][0].tobytes() == base[k][i].tobytes() for k in OUT) and one["hits"] == base["hits"][i:i + 1]
    parts = [_cast(m, views[i:i + 1])["info"] for i in range(len(views))]
    assert base["info"] == {n: sum(p[n] for p in parts) for n in mapfile.RAY_INFO_KEYS}
    assert _bytes(_cast(m, views, device=True)) == _bytes(base)
    # without the block table: a fresh process that looks every cell up
    code = CHILD % ([ROOT, os.path.join(ROOT, "tests")],)
    want = _bytes(base) + b"".join(a.tobytes() for a in base_rays[:4]) + repr(base_rays[4]).encode()
    for blocks in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, REVO_MAP_RAYCAST_BLOCKS=blocks), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        assert r.stdout == want, "REVO_MAP_RAYCAST_BLOCKS=" + blocks


def test_the_scene_map_and_stream_order():
    """The map of two 320 x 240 keyframes from its own two poses and a half-resolution camera at a third, in one call, against
    the restatement; the call enqueued directly behind an integration sees that keyframe; the map is not changed."""
    api, cam, pyrs, _ = _scene()
    spec = _scene_spec()
    P = _kf_poses()
    m = api.VoxelMap(cam, VOXEL, dense=True)
    m.integrate(pyrs[0], P[0])
    first = _cast(m, _scene_views())  # no waiting call in between
    m.integrate(pyrs[1], P[1])
    both = _cast(m, _scene_views())
    _assert_same(both, spec, "the scene map, three views in one call")
    assert m.export_raw().tobytes() == _scene_records().tobytes()
    alone = mapfile.raycast_records(_scene_records(1), VOXEL, _scene_views()[2:])  # the first keyframe alone, the small view
    assert all(first[k][2].tobytes() == alone[k][0].tobytes() for k in OUT) and first["hits"][2] == alone["hits"][0]
    assert _bytes(first) != _bytes(both) and first["hits"][0] > 70000 and first["info"]["hits"] < both["info"]["hits"]
    one = api.VoxelMap(cam, VOXEL, dense=True)
    one.integrate(pyrs[0], P[0])
    one.sync()
    assert _bytes(_cast(one, _scene_views())) == _bytes(first)
    assert one.export_raw().tobytes() == _scene_records(1).tobytes()
    # the map is not changed, whatever is cast
    before = m.export_raw().tobytes(), m.info()
    _assert_same(_cast(m, _scene_views(), device=True), spec, "device outputs")
    _cast(m, _scene_views(), min_count=2, max_steps=7)
    _cast_rays(m, _mixed_rays(257, 1), min_count=2)
    assert (m.export_raw().tobytes(), m.info()) == before
    usable = [np.isfinite(d) & (d > cc.settings320().depth_min) & (d < cc.settings320().depth_max) for d in (cc.scene_frames()[0][i][1] for i in (0, 1))]
    assert all(np.all(both["depth"][i][usable[i]] > 0) for i in (0, 1))
    print("scene: last call %.3f ms on the device" % m.last_raycast_ms())
    # an empty map gives all misses, before and after a clear
    for e in (api.VoxelMap(cam, VOXEL), m):
        if e is m:
            m.clear()
        got = _cast(e, _scene_views()[2:])
        assert got["hits"] == [0] and not got["depth"][0].any() and not got["bgr"][0].any() and np.all(got["key"][0] == mapfile.RAY_EMPTY)
        assert got["info"]["range"] == got["info"]["rays"] == 160 * 120
        r = _cast_rays(e, _mixed_rays(65, 2))
        assert r[4]["hits"] == 0 and np.all(r[0] == mapfile.RAY_EMPTY)


def test_argument_errors_write_nothing():
    from revo_amd import _lib
    import torch
    L = _lib.lib()
    rec = cc.filled_records().astype(RAW)
    m = _hand(rec)
    good = _cast(m, HAND_VIEWS[:2])
    shapes = [(12, 16), (8, 8)]
    out = {"depth": [np.full(s, -1, F) for s in shapes], "bgr": [np.full(s + (3,), 7, np.uint8) for s in shapes], "key": [np.full(s, 5, np.uint64) for s in shapes]}
    hits, info = np.full(2, 9, np.uint32), np.full(8, 9, np.uint64)
    sentinel = b"".join(a.tobytes() for k in OUT for a in out[k]) + hits.tobytes() + info.tobytes()
    ptr = {k: (C.c_void_p * 2)(*[a.ctypes.data for a in out[k]]) for k in OUT}
    hp, ip = hits.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)
    prm = MapRayParams(4096)

    def view(i=0, **kw):
        v = _views(HAND_VIEWS[:2])
        for k, x in kw.items():
            if k == "T":
                v[i].T_w_c[x[0]] = x[1]
            else:
                setattr(v[i], k, x)
        return v

    def call(v=None, n=2, p=prm, d=ptr["depth"], b=ptr["bgr"], k=ptr["key"], h=hp, dev=0, i=ip, mm=m):
        return L.revo_map_raycast(mm._h if mm is not None else None, n, view() if v is None else v, C.byref(p) if p is not None else None, d, b, k, h, dev, i)

    nan, inf = float("nan"), float("inf")
    bad_views = [view(width=0), view(1, width=2049), view(height=0), view(1, height=2049), view(T=(13, nan)), view(1, T=(0, inf)), view(fx=nan),
                 view(1, cy=inf), view(zmax=nan), view(fx=0.0), view(1, fy=-1.0), view(zmin=-0.5), view(1, zmin=6.0), view(zmin=float(cc.ZMAX)),
                 view(1, min_count=2), view(min_count=3)]
    for j, v in enumerate(bad_views):
        assert call(v) == INVALID_ARG and L.revo_last_error(), j
    for p in (MapRayParams(0), MapRayParams((1 << 20) + 1), MapRayParams(16, (C.c_uint32 * 3)(1, 0, 0)), MapRayParams(16, (C.c_uint32 * 3)(0, 0, 1))):
        assert call(p=p) == INVALID_ARG
    none2 = (C.c_void_p * 2)(out["depth"][0].ctypes.data, None)
    assert [call(n=0), call(n=-1), call(n=65), call(mm=None), call(d=None), call(d=none2), call(b=none2), call(k=none2), call(dev=2), call(dev=-1)] == [INVALID_ARG] * 10
    assert L.revo_map_raycast(m._h, 2, None, None, ptr["depth"], None, None, None, 0, None) == INVALID_ARG
    # device outputs: every pointer 16-byte aligned
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    base = t.data_ptr()
    ok2, off2 = (C.c_void_p * 2)(base, base + 1024), (C.c_void_p * 2)(base, base + 1024 + 4)
    for kw in (dict(d=off2, b=ok2, k=ok2), dict(d=ok2, b=off2, k=ok2), dict(d=ok2, b=ok2, k=off2), dict(d=ok2, b=ok2, k=ok2, h=C.c_void_p(base + 8)),
               dict(d=ok2, b=ok2, k=ok2, h=None, i=C.c_void_p(base + 8))):
        assert call(dev=1, **dict(dict(h=None, i=None), **kw)) == INVALID_ARG
    m.sync()
    assert not t.cpu().numpy().any()
    assert b"".join(a.tobytes() for k in OUT for a in out[k]) + hits.tobytes() + info.tobytes() == sentinel
    # cast_rays
    rays = _mixed_rays(65, 5)
    res = np.full(16 * 65, 7, np.uint8)
    rp, op = rays.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)

    def rcall(n=65, r=rp, din=0, mc=1, p=prm, o=op, dev=0, i=ip, mm=m):
        return L.revo_map_cast_rays(mm._h if mm is not None else None, n, r, din, mc, C.byref(p) if p is not None else None, o, dev, i)

    assert [rcall(n=0), rcall(n=(1 << 24) + 1), rcall(r=None), rcall(o=None), rcall(mm=None), rcall(din=2), rcall(dev=2), rcall(din=-1),
            rcall(p=MapRayParams(0)), rcall(p=MapRayParams(1, (C.c_uint32 * 3)(0, 1, 0))), rcall(r=C.c_void_p(base + 4), din=1, o=C.c_void_p(base), dev=1, i=None),
            rcall(r=C.c_void_p(base), din=1, o=C.c_void_p(base + 8), dev=1, i=None),
            rcall(r=C.c_void_p(base), din=1, o=C.c_void_p(base + 2048), dev=1, i=C.c_void_p(base + 4))] == [INVALID_ARG] * 13
    m.sync()
    assert np.all(res == 7) and not t.cpu().numpy().any() and info.tobytes() == np.full(8, 9, np.uint64).tobytes()
    # the handle is as usable as before; NULL parameters are max_steps 4096; bgr, key, hits and info may all be NULL
    assert call() == 0 and call(p=None) == 0
    assert b"".join(a.tobytes() for k in OUT for a in out[k]) == b"".join(a.tobytes() for k in OUT for a in good[k]) and hits.tolist() == good["hits"]
    d_only = [np.full(s, -1, F) for s in shapes]
    assert L.revo_map_raycast(m._h, 2, view(), None, (C.c_void_p * 2)(*[a.ctypes.data for a in d_only]), None, None, None, 0, None) == 0
    assert [a.tobytes() for a in d_only] == [a.tobytes() for a in good["depth"]]
    assert rcall(p=None, i=None) == 0
    want = mapfile.cast_rays_records(rec, VOXEL, rays)
    r = res.view(np.dtype([("key", "<u8"), ("s", "<f4"), ("cells", "<u4")]))
    assert r["key"].tobytes() == want[0].tobytes() and r["s"].tobytes() == want[1].tobytes()
    assert ((r["cells"] & 0xFFFFFF).tobytes(), (r["cells"] >> 30).astype(np.uint8).tobytes()) == (want[2].tobytes(), want[3].tobytes())
    fresh = _hand(rec)
    ms = C.c_float()
    assert L.revo_map_raycast_last_ms(fresh._h, C.byref(ms)) == INVALID_ARG and L.revo_map_raycast_last_ms(m._h, None) == INVALID_ARG
    assert L.revo_map_raycast_last_ms(m._h, C.byref(ms)) == 0 and ms.value > 0


def test_run_tum_map_views_raycast(tmp_path, monkeypatch):
    from revo_amd import api, run_tum, tum
    from test_gpu_map_render import S320
    from test_gpu_vo_multi import _tum_yaml
    from test_gpu_voxel_map import BIASES
    name = "rgbd_synth_b"
    seq = synth.make_sequence(952, S320, 33, max_t=0.01, max_rot_deg=0.4, bias=BIASES[4])
    tum.write_synthetic_dataset(str(tmp_path / "data" / name), seq)
    _tum_yaml(tmp_path, S320, [name])
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "2", "--map", "0.02"]
    for sub, extra in (("splat", ["--map-views", "views"]), ("rays", ["--map-views", "views", "--map-views-raycast", "--map-save", "map.rvm"])):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra) == 0
    assert run_tum.main(args + ["--map-views-raycast"]) == 2  # without --map-views: a usage error
    monkeypatch.chdir(tmp_path)
    for f in ("poses_%s.txt" % name, "map_%s.ply" % name):  # the run's own files do not depend on the option
        assert (tmp_path / "splat" / f).read_bytes() == (tmp_path / "rays" / f).read_bytes(), f
    a, b = tmp_path / "splat" / "views", tmp_path / "rays" / "views"
    assert (a / "poses.txt").read_bytes() == (b / "poses.txt").read_bytes() and (a / "associate.txt").read_bytes() == (b / "associate.txt").read_bytes()
    rows = tum.read_associate(str(b / "associate.txt"))
    poses = tum.read_poses(str(b / "poses.txt"))
    assert len(rows) == len(poses) >= 1
    m = api.VoxelMap.load(api.CameraPyr(S320), str(tmp_path / "rays" / "map.rvm"))
    differ = 0
    for (rts, rf, dts, df), (ts, T) in zip(rows, poses):
        bgr, d16 = tum.load_frame(str(b), rf, df)
        d, c, hits = m.raycast(T)
        raw = np.clip(np.rint(d.astype(np.float64) * 5000.0), 0, 65535).astype(np.uint16)
        assert d16.dtype == np.uint16 and d16.tobytes() == raw.tobytes() and bgr.tobytes() == c.tobytes() and hits > 100
        differ += int(np.sum(tum.load_frame(str(a), rf, df)[1] != d16))
    assert differ > 0  # not the splat's views
