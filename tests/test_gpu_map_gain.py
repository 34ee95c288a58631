"""View gain on the device (revo_map_view_gain, api.VoxelMap.view_gain / view_gain_into, api.next_view): every shared
case bit for bit revo_amd.mapfile's gain_records (which test_map_gain_cpu.py pins to the per-cell specification), from host and
device poses and volumes into host and device records, the info record included; the composition it replaces (raycast, observe
into a copy, count) on the device; chunking, order and repeated runs; nothing but the records is written; every argument error;
a 64^3 box of DESIGN 19's scene; next_view; MapWindow."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile  # noqa: E402
from revo_amd.settings import MapDfBox, MapGainParams, MapView  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_gain_cases as gc  # noqa: E402
import map_seen_cases as sc  # noqa: E402
import test_gpu_map_raycast as tr  # noqa: E402

F = np.float32
RAW = mapfile.RAW_DTYPE
INVALID_ARG = -1
FIELDS = ("unknown_free", "unknown_surface", "unknown_inside", "hits")
SIDES = ((0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0))  # (device seen, device poses, device records)


def _box(lo, n):
    return MapDfBox((C.c_int32 * 3)(*[int(x) for x in lo]), (C.c_int32 * 3)(*[int(x) for x in n]))


def _map(rec, voxel=gc.V):
    return tr._hand(np.asarray(rec).astype(RAW), voxel)


def _cam(view, min_count=1):
    k, (w, h) = view
    v = MapView()
    v.width, v.height = w, h
    v.fx, v.fy, v.cx, v.cy, v.zmin, v.zmax = [float(x) for x in k]
    v.T_w_c[:] = [float("nan")] * 16  # the camera's own pose and splat_max are not read
    v.splat_max, v.min_count = 77, min_count
    return v


def _params(m, radius=1, min_views=1, margin=None, margin_rel=0.0, miss_depth=0.0, max_steps=4096, **_):
    return MapGainParams(int(radius), int(min_views), float(m.voxel if margin is None else margin), float(margin_rel), float(miss_depth), int(max_steps))


def _gain(m, c, sides=(0, 0, 0), poses=None, **over):
    """revo_map_view_gain of a case with each of the volume, the poses and the records in host or device memory -> (records
    [poses, 8] uint32, info [8]); the outputs start as nines, and the volume must come back as it went in."""
    import torch
    dev_seen, dev_in, dev_out = sides
    p = dict(c["params"], **over)
    poses = np.ascontiguousarray(np.asarray(c["poses"] if poses is None else poses, F).reshape(-1, 4, 4).transpose(0, 2, 1))
    k = len(poses)
    seen = np.ascontiguousarray(c["seen"], np.uint8)
    prm, cam, box = _params(m, **p), _cam(c["view"], p.get("min_count", 1)), _box(c["lo"], c["n"])
    d_seen = torch.from_numpy(seen.copy()).cuda() if dev_seen else None
    d_poses = torch.from_numpy(poses).cuda() if dev_in else None
    out, info = np.full((k, 8), 9, np.uint32), np.full(8, 9, np.uint64)
    d_out = torch.from_numpy(out.view(np.int32)).cuda() if dev_out else None
    d_info = torch.from_numpy(info.view(np.int64)).cuda() if dev_out else None
    torch.cuda.synchronize()
    ptr = lambda t, a: C.c_void_p(t.data_ptr()) if t is not None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _lib.check(_lib.lib().revo_map_view_gain(m._h, C.byref(box), ptr(d_seen, seen), dev_seen, C.byref(cam), k, ptr(d_poses, poses), dev_in, C.byref(prm),
                                             ptr(d_out, out), dev_out, ptr(d_info, info)))
    m.sync()
    if dev_out:
        out, info = d_out.cpu().numpy().view(np.uint32), d_info.cpu().numpy().view(np.uint64)
    if dev_seen:
        assert d_seen.cpu().numpy().tobytes() == seen.tobytes()
    assert seen.tobytes() == np.ascontiguousarray(c["seen"], np.uint8).tobytes()
    return out, info


def _want(c, poses=None, device_poses=False, **over):
    g = mapfile.gain_records(c["rec"].astype(RAW), gc.V, c["lo"], c["n"], c["seen"], c["view"], c["poses"] if poses is None else poses,
                             device_poses=device_poses, **dict(c["params"], **over))
    return np.stack([g[f] for f in FIELDS], 1), [g.info[k] for k in mapfile.GAIN_INFO_KEYS]


def _same(got, want, what):
    assert got[0][:, :4].tolist() == want[0].tolist(), what
    assert not got[0][:, 4:].any() and got[1].tolist() == want[1], (what, got[1].tolist(), want[1])


@pytest.mark.parametrize("name", list(gc.cases()))
def test_hand_made_cases_bit_exact(name):
    c = gc.cases()[name]
    want = _want(c)
    m = _map(c["rec"])
    before = m.export_raw().tobytes()
    for sides in SIDES:
        _same(_gain(m, c, sides), want, (name, sides))
    print(name, dict(zip(mapfile.GAIN_INFO_KEYS, want[1])), want[0][:3].tolist())
    assert m.export_raw().tobytes() == before
    m.close()


def test_device_poses_that_break_the_rules_give_zero_records():
    c = gc.device_case()
    want = _want(c, device_poses=True)
    m = _map(c["rec"])
    for sides in ((1, 1, 1), (0, 1, 0)):
        got = _gain(m, c, sides)
        _same(got, want, sides)
        assert not got[0][[3, 40, 64]].any() and got[0][[2, 39, 63], 2].all()
    # the same poses in host memory are refused, whichever it is
    for j in (3, 40, 64):
        with pytest.raises(_lib.RevoError):
            _gain(m, c, (0, 0, 0), poses=c["poses"][[0, j]])
    m.close()


@pytest.mark.parametrize("name", ["wall, real volume", "wall, miss depth", "box 9x7x5", "tail 3x3x5", "radius 2", "empty map"])
def test_the_composition_on_the_device(name):
    """raycast -> observe(into = a copy) -> the count over the unknown cells, per pose, equals the record."""
    c = gc.cases()[name]
    p = dict(c["params"])
    rec = c["rec"].astype(RAW)
    m = _map(rec)
    got = _gain(m, c, (1, 1, 1))[0]
    k, (w, h) = c["view"]
    solid = mapfile.solid_cells(rec, np.asarray(c["lo"]), np.asarray(c["n"]))[0]
    unknown = ~mapfile.seen_known(c["seen"], 1, solid)
    vol = api.SeenVolume(c["seen"], c["lo"], gc.V)
    for j, T in enumerate(c["poses"]):
        D, _, hits = m.raycast(T, camera=k[:4] + (w, h), zrange=k[4:], max_steps=p.get("max_steps", 4096))
        assert hits == got[j, 3]
        if p.get("miss_depth", 0.0):
            D = np.where(D == 0, F(p["miss_depth"]), D)
        after = m.observe([(D, T, k)], radius=p.get("radius", 1), margin=p.get("margin"), margin_rel=p.get("margin_rel", 0.0), into=vol).seen
        assert int(((after != c["seen"]) & unknown).sum()) == int(got[j, 0]) + int(got[j, 1]), (name, j)
        assert int(((after & 0x80 != 0) & unknown).sum()) == int(got[j, 1])
    m.close()


def test_chunks_order_and_repeated_runs():
    c = gc.cases()["65 poses"]
    m = _map(c["rec"])
    whole = _gain(m, c, (1, 1, 1))
    _same(whole, _want(c), "65 poses")
    for sides in ((1, 1, 1), (0, 0, 0)):
        for _ in range(3):
            again = _gain(m, c, sides)
            assert again[0].tobytes() == whole[0].tobytes() and again[1].tobytes() == whole[1].tobytes()
        one = np.concatenate([_gain(m, c, sides, poses=c["poses"][j:j + 1])[0] for j in range(65)])
        assert one.tobytes() == whole[0].tobytes()
        perm = np.random.default_rng(4).permutation(65)
        assert _gain(m, c, sides, poses=c["poses"][perm])[0].tobytes() == whole[0][perm].tobytes()
        parts = [_gain(m, c, sides, poses=c["poses"][a:b]) for a, b in ((0, 64), (64, 65))]
        assert np.concatenate([x[0] for x in parts]).tobytes() == whole[0].tobytes()
        assert [int(parts[0][1][i] + parts[1][1][i]) for i in (3, 4, 5, 6, 7)] == [int(whole[1][i]) for i in (3, 4, 5, 6, 7)]
    m.close()


def test_argument_errors_write_nothing():
    import torch
    L = _lib.lib()
    c = gc.cases()["box 3x5x7"]
    m = _map(c["rec"])
    before = m.export_raw().tobytes()
    good_box, cam, prm = _box(c["lo"], c["n"]), _cam(c["view"]), _params(m, miss_depth=1.5)
    seen = np.ascontiguousarray(c["seen"]).copy()
    poses = np.ascontiguousarray(c["poses"].transpose(0, 2, 1))
    out, info = np.full((len(poses), 8), 9, np.uint32), np.full(8, 9, np.uint64)
    t = torch.full((8192,), 0x77, dtype=torch.uint8, device="cuda")
    base = t.data_ptr()
    assert base % 16 == 0
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    dp = lambda off: C.c_void_p(base + off)  # noqa: E731

    def call(mm=m, box=good_box, s=hp(seen), ds=0, cm=cam, k=len(poses), T=hp(poses), di=0, p=prm, o=hp(out), do=0, i=hp(info)):
        return L.revo_map_view_gain(mm._h if mm is not None else None, C.byref(box) if box is not None else None, s, ds,
                                    C.byref(cm) if cm is not None else None, k, T, di, C.byref(p) if p is not None else None, o, do, i)

    def cam_with(**kw):
        v = _cam(c["view"])
        for name, x in kw.items():
            setattr(v, name, x)
        return v

    def prm_with(**kw):
        v = _params(m, miss_depth=1.5)
        for name, x in kw.items():
            if name == "reserved":
                v.reserved[x] = 1
            else:
                setattr(v, name, x)
        return v

    R = 1 << 20
    bad = [dict(mm=None), dict(box=None), dict(s=None), dict(cm=None), dict(T=None), dict(o=None), dict(k=0), dict(k=4097),
           dict(ds=2), dict(di=-1), dict(do=2)]
    bad += [dict(box=b) for b in (_box((0, 0, 0), (0, 3, 5)), _box((0, 0, 0), (4, 3, 1025)), _box((0, 0, 0), (1024, 1024, 129)),
                                  _box((-R - 1, 0, 0), (4, 3, 5)), _box((0, 0, R - 5), (4, 3, 6)))]
    bad += [dict(cm=cam_with(**kw)) for kw in (dict(width=0), dict(height=2049), dict(fx=0.0), dict(fy=-1.0), dict(cx=float("nan")), dict(zmin=-0.5),
                                               dict(zmin=6.0), dict(zmax=float("inf")))]
    bad += [dict(p=prm_with(**kw)) for kw in (dict(radius=4), dict(radius=-1), dict(margin=-0.1), dict(margin=float("nan")), dict(margin=float("inf")),
                                              dict(margin_rel=-1.0), dict(margin_rel=float("nan")), dict(miss_depth=0.05), dict(miss_depth=5.2),
                                              dict(miss_depth=-1.0), dict(miss_depth=float("nan")), dict(max_steps=0), dict(max_steps=R + 1),
                                              dict(reserved=0), dict(reserved=1))]
    for kind in ("nan", "inf", "skew"):
        T = poses.copy()
        T[2] = gc.bad_pose(kind).T
        bad.append(dict(T=hp(T)))
        bad[-1]["_keep"] = T
    bad += [dict(s=dp(8), ds=1), dict(T=dp(1024 + 4), di=1), dict(o=dp(2048 + 8), do=1, i=dp(4096)), dict(o=dp(2048), do=1, i=dp(4096 + 8))]
    for kw in bad:
        kw.pop("_keep", None)
        assert call(**kw) == INVALID_ARG, kw
    m.sync()
    assert np.all(out == 9) and np.all(info == 9) and seen.tobytes() == np.ascontiguousarray(c["seen"]).tobytes()
    assert np.all(t.cpu().numpy() == 0x77) and m.export_raw().tobytes() == before
    # NULL parameters are the defaults; a NULL info is allowed on both sides
    assert call(p=None, i=None) == 0
    want = _want(c, miss_depth=0.0, margin=None)
    assert out[:, :4].tolist() == want[0].tolist() and np.all(info == 9)
    m.close()


# ----------------------------------------------------------------------------------------------------------- the Python API --
def test_view_gain_and_view_gain_into():
    import torch
    c = gc.cases()["wall, miss depth"]
    m = _map(c["rec"])
    k, size = c["view"]
    vol = api.SeenVolume(c["seen"], c["lo"], gc.V)
    want = mapfile.gain_records(c["rec"].astype(RAW), gc.V, c["lo"], c["n"], c["seen"], c["view"], c["poses"], miss_depth=2.0)
    got = m.view_gain(vol, c["poses"], camera=k[:4], size=size, zrange=k[4:], miss_depth=2.0)
    assert isinstance(got, mapfile.GainRecords) and got.dtype == mapfile.GAIN_DTYPE and got.tobytes() == want.tobytes() and got.info == want.info
    one = m.view_gain(vol, c["poses"][1], camera=api.Camera(*k[:4], *size), zrange=k[4:], miss_depth=2.0)
    assert len(one) == 1 and one.tobytes() == want[1:2].tobytes()
    # the context's own camera: all-zero intrinsics
    s = cc.settings320()
    ctx = ((s.fx, s.fy, s.cx, s.cy, s.depth_min, s.depth_max), (s.width, s.height))
    far = mapfile.gain_records(c["rec"].astype(RAW), gc.V, c["lo"], c["n"], c["seen"], ctx, c["poses"][1:], radius=2, min_views=2)
    assert m.view_gain(vol, c["poses"][1:], radius=2, min_views=2).tobytes() == far.tobytes()
    d_out = torch.full((2, 8), 9, dtype=torch.int32, device="cuda")
    d_info = torch.full((8,), 9, dtype=torch.int64, device="cuda")
    d_seen = torch.from_numpy(np.ascontiguousarray(c["seen"])).cuda()
    d_poses = torch.from_numpy(np.ascontiguousarray(c["poses"].transpose(0, 2, 1))).cuda()
    m.view_gain_into(d_out, d_seen, c["lo"], d_poses, camera=k[:4], size=size, zrange=k[4:], miss_depth=2.0, d_info=d_info)
    assert d_out.cpu().numpy().tobytes() == want.tobytes() and d_info.cpu().numpy().tolist() == [want.info[x] for x in mapfile.GAIN_INFO_KEYS]
    with pytest.raises(ValueError):
        m.view_gain(vol, c["poses"], size=size)
    with pytest.raises(ValueError):
        m.view_gain(api.SeenVolume(c["seen"], c["lo"], 0.5), c["poses"])
    with pytest.raises(ValueError):
        m.view_gain_into(d_out[:1], d_seen, c["lo"], d_poses, camera=k[:4], size=size)
    with pytest.raises(_lib.RevoError):
        m.view_gain(vol, c["poses"], camera=k[:4], size=size, zrange=k[4:], miss_depth=9.0)
    m.close()


def test_next_view_on_the_device():
    w = gc.wall()
    rec = w["rec"].astype(RAW)
    m = _map(rec)
    vol = api.SeenVolume(w["seen"], w["lo"], gc.V)
    k, size = gc.VIEW
    kw = dict(headings=4, up=(0, 0, 1), stride=4, miss_depth=2.0)
    want = mapfile.next_view_records(rec, gc.V, w["lo"], w["n"], w["seen"], w["start"], gc.V, gc.VIEW, **kw)
    got = api.next_view(m, vol, w["start"], gc.V, camera=k[:4], size=size, zrange=k[4:], **kw)
    for name in ("pose", "cell", "scores", "poses", "cells"):
        assert np.array_equal(got[name], want[name]), name
    assert got["index"] == want["index"] and got["heading"] == want["heading"] and got["gain"].tobytes() == want["gain"].tobytes()
    assert got["record"].tobytes() == want["record"].tobytes() and got["cost"].cost.tobytes() == want["cost"].tobytes()
    assert got["path"][0].tolist() == want["path"][0].tolist() and got["path"][1:] == want["path"][1:]
    assert got["cell"][1] >= 12 and got["pose"][0, 2] > 0.99 and got["path"][0][-1].tolist() == list(w["start"])  # through the gap
    with pytest.raises(ValueError):
        api.next_view(m, vol, (20, 8, 8), gc.V, camera=k[:4], size=size, zrange=k[4:], **kw)  # a start in unseen space
    m.close()


def test_map_window_forwards():
    import torch
    c = gc.cases()["box 9x7x5"]
    cam = tr._scene()[1]
    win = api.MapWindow(cam, gc.V, window=2)
    win.map.merge_raw(c["rec"].astype(RAW))
    k, size = c["view"]
    vol = api.SeenVolume(c["seen"], c["lo"], gc.V)
    want = mapfile.gain_records(c["rec"].astype(RAW), gc.V, c["lo"], c["n"], c["seen"], c["view"], c["poses"], **c["params"])
    assert win.view_gain(vol, c["poses"], camera=k[:4], size=size, zrange=k[4:], **c["params"]).tobytes() == want.tobytes()
    d_out = torch.zeros((len(want), 8), dtype=torch.int32, device="cuda")
    win.view_gain_into(d_out, torch.from_numpy(np.ascontiguousarray(c["seen"])).cuda(), c["lo"],
                       torch.from_numpy(np.ascontiguousarray(c["poses"].transpose(0, 2, 1))).cuda(), camera=k[:4], size=size, zrange=k[4:], **c["params"])
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    win.close()


# ---------------------------------------------------------------------------------------------------------------- the scene --
@functools.lru_cache(maxsize=None)
def _scene64():
    """A 64^3 box of DESIGN 19's scene, seen from its first two views; the candidates are its four views' poses at a quarter of
    the resolution, and two of them nudged."""
    lo, n = sc.scene_box(64)
    views = cc.scene_views(False)
    seen = mapfile.observe_records(cc.VOXEL, lo, n, views[:2])[0]
    fx, fy, cx, cy, zmin, zmax = cc.intrinsics320()
    view = ((fx / 4, fy / 4, (cx + 0.5) / 4 - 0.5, (cy + 0.5) / 4 - 0.5, zmin, zmax), (80, 60))
    poses = np.stack([v[1] for v in views] + [gc.nudged(views[2][1], 1, 0.1), gc.nudged(views[3][1], 2, 0.2)])
    return lo, n, seen, view, poses


def test_the_scene_box():
    lo, n, seen, view, poses = _scene64()
    rec = cc.scene_records().astype(RAW)
    m = _map(rec, cc.VOXEL)
    c = dict(lo=lo, n=n, seen=seen, view=view, poses=poses, params={})
    for params in (dict(), dict(miss_depth=3.0, radius=2, min_views=2)):
        g = mapfile.gain_records(rec, cc.VOXEL, lo, n, seen, view, poses, **params)
        want = (np.stack([g[f] for f in FIELDS], 1), [g.info[k] for k in mapfile.GAIN_INFO_KEYS])
        for sides in ((0, 0, 0), (1, 1, 1)):
            _same(_gain(m, c, sides, **params), want, ("scene", params, sides))
        print("scene 64^3:", params, g.info, want[0].tolist())
        assert g.info["unknown_free"] > 0 and g.info["ray_hits"] > 0
    m.close()
