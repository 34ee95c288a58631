"""Views of the TSDF surface on the device (revo_map_tsdf_raycast, api.VoxelMap.surface_raycast / surface_raycast_into,
api.TsdfVolume.raycast, api.SurfaceVolume.raycast, api.MapWindow, run_tum --surface-views): depth, normals, colours, hits
and info bit for bit revo_amd.mapfile's restatement (which test_map_tsdf_ray_cpu.py pins to the per-sample loop) on the shared
cases, with the volumes and the outputs in host and in device memory, through the block mask and without it; optional outputs
left NULL; every argument error with sentinel-filled outputs; fuse -> ray cast on the device; the pyramid form and the window; the
64^3 scene box from its four poses; the command."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile  # noqa: E402
from revo_amd.settings import MapTsdfRayInfo, MapTsdfRayParams  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_seen_cases as sc  # noqa: E402
import map_tsdf_cases as tc  # noqa: E402
import map_tsdf_ray_cases as rc  # noqa: E402
import test_gpu_map_raycast as tr  # noqa: E402
import test_gpu_map_surface as ts  # noqa: E402
import test_gpu_map_tsdf as tt  # noqa: E402

F = np.float32
INVALID_ARG = -1
vp = C.c_void_p
SIDES = ((False, False), (True, False), (True, True), (False, True))  # (device volumes, device outputs)


def _call(m, cells, color, lo, views, step=None, min_weight=1, max_steps=4096, device_tsdf=False, device_out=False, normals=True, colors=True,
          hits=True, info=True, fill=0x2B, raw=None):
    """revo_map_tsdf_raycast with the volumes and the outputs on either side, every output filled with `fill` bytes first ->
    (return code, dict of depth, normals, bgr, hits, info as mapfile gives them; None where not asked for).  raw: a dict that
    replaces arguments of the call (box, prm, n, flags, pointers) for the argument errors."""
    import torch
    L = _lib.lib()
    raw = raw or {}
    colors = colors and color is not None
    box = tt._box(lo, cells.shape)
    v = tr._views(views)
    n = len(views)
    sizes = [(max(h, 1), max(w, 1)) for _, _, (w, h) in views]  # a refused size still gets an output to look at
    keep = []
    if device_tsdf:
        d_cells = tt._as_tensor(cells)
        d_col = ts._col_tensor(color) if color is not None else None
        keep += [d_cells, d_col]
        p_cells, p_col = vp(d_cells.data_ptr()), (vp(d_col.data_ptr()) if d_col is not None else None)
    else:
        h_cells = np.ascontiguousarray(cells)
        h_col = np.ascontiguousarray(color) if color is not None else None
        keep += [h_cells, h_col]
        p_cells, p_col = h_cells.ctypes.data_as(vp), (h_col.ctypes.data_as(vp) if h_col is not None else None)
    if device_out:
        byte = lambda shape, dt: torch.full(shape, fill, dtype=torch.uint8, device="cuda").view(dt)  # noqa: E731
        o_depth = [byte((h, w * 4), torch.float32) for h, w in sizes]
        o_nrm = [byte((h, w * 12), torch.float32) for h, w in sizes]
        o_bgr = [byte((h, w * 3), torch.uint8) for h, w in sizes]
        o_hits = byte((256,), torch.int32)[:n]
        o_info = byte((64,), torch.int64)
        torch.cuda.synchronize()
        ptr = lambda t: t.data_ptr()  # noqa: E731
        p_hits, p_info = vp(o_hits.data_ptr()), vp(o_info.data_ptr())
    else:
        o_depth = [np.full((h, w * 4), fill, np.uint8).view(F) for h, w in sizes]
        o_nrm = [np.full((h, w * 12), fill, np.uint8).view(F).reshape(h, w, 3) for h, w in sizes]
        o_bgr = [np.full((h, w, 3), fill, np.uint8) for h, w in sizes]
        o_hits = np.full(n, fill * 0x01010101, np.uint32)
        o_info = MapTsdfRayInfo(*([fill * 0x0101010101010101] * 8))
        ptr = lambda a: a.ctypes.data  # noqa: E731
        p_hits, p_info = o_hits.ctypes.data_as(vp), C.cast(C.byref(o_info), vp)
    arr = lambda xs: (vp * n)(*[ptr(x) for x in xs])  # noqa: E731
    prm = MapTsdfRayParams(0.0 if step is None else float(step), int(min_weight), int(max_steps), 0)
    a = dict(m=m._h, box=C.byref(box), tsdf=p_cells, color=p_col if (colors or raw.get("keep_color")) else None, device_tsdf=1 if device_tsdf else 0, n=n, views=v,
             prm=C.byref(prm), depth=arr(o_depth), normal=arr(o_nrm) if normals else None, bgr=arr(o_bgr) if colors else None,
             hits=p_hits if hits else None, device_out=1 if device_out else 0, info=p_info if info else None)
    a.update({k: x for k, x in raw.items() if k in a})
    rc_ = L.revo_map_tsdf_raycast(a["m"], a["box"], a["tsdf"], a["color"], a["device_tsdf"], a["n"], a["views"], a["prm"], a["depth"], a["normal"], a["bgr"],
                                  a["hits"], a["device_out"], a["info"])
    m.sync()
    if device_out:
        torch.cuda.synchronize()
        host = lambda t: t.cpu().numpy()  # noqa: E731
        depth = [host(t) for t in o_depth]
        nrm = [host(t).reshape(h, w, 3) for t, (h, w) in zip(o_nrm, sizes)]
        bgr = [host(t).reshape(h, w, 3) for t, (h, w) in zip(o_bgr, sizes)]
        hit = host(o_hits).view(np.uint32)
        inf = host(o_info).view(np.uint64).tolist()
    else:
        depth, nrm, bgr, hit = o_depth, o_nrm, o_bgr, o_hits
        inf = [int(getattr(o_info, k)) for k, _ in MapTsdfRayInfo._fields_]
    del keep
    return rc_, {"depth": depth, "normals": nrm, "bgr": bgr, "hits": [int(x) for x in hit], "info": dict(zip(mapfile.TSDF_RAY_INFO_KEYS, inf[:7])),
                 "reserved": inf[7]}


def _untouched(got, fill=0x2B):
    """Every output still holds the fill."""
    blank = lambda a: bool(np.all(np.ascontiguousarray(a).view(np.uint8) == fill))  # noqa: E731
    return all(blank(a) for key in ("depth", "normals", "bgr") for a in got[key]) and blank(np.array(got["hits"], np.uint32)) and \
        blank(np.array(list(got["info"].values()) + [got["reserved"]], np.uint64))


def _same(got, want, what, normals=True, colors=True, hits=True, info=True, fill=0x2B):
    """The outputs asked for are mapfile's, the others still hold the fill."""
    blank = lambda a: bool(np.all(np.ascontiguousarray(a).view(np.uint8) == fill))  # noqa: E731
    for i, d in enumerate(want["depth"]):
        assert got["depth"][i].tobytes() == d.tobytes(), (what, "depth", i, int(np.sum(got["depth"][i] != d)))
        if normals:
            assert got["normals"][i].tobytes() == want["normals"][i].tobytes(), (what, "normals", i)
        else:
            assert blank(got["normals"][i]), (what, "normals written", i)
        if colors and want["bgr"][i] is not None:
            assert got["bgr"][i].tobytes() == want["bgr"][i].tobytes(), (what, "bgr", i)
        else:
            assert blank(got["bgr"][i]), (what, "bgr written", i)
    if hits:
        assert got["hits"] == want["hits"], (what, got["hits"], want["hits"])
    else:
        assert blank(np.array(got["hits"], np.uint32)), what
    if info:
        assert got["info"] == want["info"] and got["reserved"] == 0, (what, got["info"], want["info"])
    else:
        assert blank(np.array(list(got["info"].values()), np.uint64)), what


@functools.lru_cache(maxsize=None)
def _want(name):
    c = rc.cases()[name]
    a, kw = rc.args(c)
    return mapfile.tsdf_raycast_records(*a, **kw)


# ---------------------------------------------------------------------------------------------------------------- the cases --
@pytest.mark.parametrize("name", list(rc.cases()))
def test_cases_bit_exact(name):
    c = rc.cases()[name]
    want = _want(name)
    m = tt._map(sc.records_at([(0, 0, 8), (-4, -3, 6)]))  # a map with voxels in the boxes: they play no part
    before = m.export_raw().tobytes()
    kw = dict(step=c["step"], min_weight=c["min_weight"], max_steps=c["max_steps"])
    for device_tsdf, device_out in SIDES:
        code, got = _call(m, c["cells"], c["color"], c["lo"], c["views"], device_tsdf=device_tsdf, device_out=device_out, **kw)
        assert code == 0, _lib.lib().revo_last_error()
        _same(got, want, (name, device_tsdf, device_out))
    print(name, want["info"])
    assert m.export_raw().tobytes() == before
    m.close()


@pytest.mark.parametrize("name", ("9x9x17 block border z", "17x9x9 block border x", "zero sums", "thin layer stepped over", "unknown cell between",
                                  "inside and outside the box", "sphere"))
def test_the_block_mask_does_not_show(name, monkeypatch):
    """REVO_MAP_TSDF_RAY_MASK=0 evaluates every sample: the same bytes, `samples` included."""
    c = rc.cases()[name]
    m = tt._map()
    monkeypatch.setenv("REVO_MAP_TSDF_RAY_MASK", "0")
    code, got = _call(m, c["cells"], c["color"], c["lo"], c["views"], step=c["step"], min_weight=c["min_weight"], max_steps=c["max_steps"], device_tsdf=True,
                      device_out=True)
    assert code == 0
    _same(got, _want(name), (name, "plain march"))
    m.close()


def test_optional_outputs_left_null():
    c = rc.cases()["inside and outside the box"]
    want = _want("inside and outside the box")
    m = tt._map()
    for device in (False, True):
        for normals, colors, hits, info in ((False, True, True, True), (True, False, True, True), (True, True, False, True), (True, True, True, False),
                                            (False, False, False, False)):
            code, got = _call(m, c["cells"], c["color"], c["lo"], c["views"], device_tsdf=device, device_out=device, normals=normals, colors=colors,
                              hits=hits, info=info)
            assert code == 0
            w = want if colors else dict(want, info=dict(want["info"], uncolored=0))  # without the colour volume no hit counts as uncoloured
            _same(got, w, (device, normals, colors, hits, info), normals, colors, hits, info)
    # the colour volume given, the colour images not: uncolored still counts
    code, got = _call(m, c["cells"], c["color"], c["lo"], c["views"], colors=False, raw=dict(keep_color=True))
    assert code == 0 and got["info"] == want["info"]
    m.close()


def test_argument_errors_write_nothing():
    import torch
    c = rc.cases()["3x5x7 lo < 0"]
    m = tt._map()
    T, k, size = c["views"][0]
    nanT = T.copy()
    nanT[1, 3] = np.inf

    def prm(step=0.0, mw=1, ms=4096, res=0):
        p = MapTsdfRayParams(step, mw, ms, res)
        return dict(prm=C.byref(p), _keep=p)

    def box(lo, n):
        b = tt._box(lo, n)
        return dict(box=C.byref(b), _keep=b)

    bad_views = [[(nanT, k, size)], [(T, k, (0, 12))], [(T, k, (16, 2049))], [(T, (0.0,) + tuple(k[1:]), size)], [(T, tuple(k[:4]) + (1.0, 1.0), size)],
                 [(T, tuple(k[:4]) + (-0.5, 1.0), size)], [(T, tuple(k[:5]) + (float("nan"),), size)]]
    raws = [dict(m=None), dict(box=None), dict(tsdf=None), dict(views=None), dict(depth=None), dict(n=0), dict(n=65), dict(n=-1),
            dict(device_tsdf=2), dict(device_out=-1), dict(color=None),  # bgr without color
            prm(step=-0.125), prm(step=float("nan")), prm(step=float("inf")), prm(ms=(1 << 20) + 1), prm(res=1),
            box(c["lo"], (0, 5, 7)), box(c["lo"], (3, 5, 1025)), box(((1 << 20) - 2, 0, 0), (3, 5, 7)), box((0, 0, 0), (1024, 1024, 256))]
    for device in (False, True):
        for raw in raws:
            code, got = _call(m, c["cells"], c["color"], c["lo"], c["views"], device_tsdf=device, device_out=device, raw=raw)
            assert code == INVALID_ARG, (device, {x: y for x, y in raw.items() if x != "_keep"})
            assert _untouched(got), (device, {x: y for x, y in raw.items() if x != "_keep"})
        for views in bad_views:
            code, got = _call(m, c["cells"], c["color"], c["lo"], views, device_tsdf=device, device_out=device)
            assert code == INVALID_ARG and _untouched(got), views
    # a NULL entry of a given array, and misaligned device pointers
    two = [c["views"][0], c["views"][0]]
    for which in ("depth", "normal", "bgr"):
        holes = (vp * 2)(None, None)
        assert _call(m, c["cells"], c["color"], c["lo"], two, raw={which: holes})[0] == INVALID_ARG
    d = torch.zeros(64 * 48 + 8, dtype=torch.float32, device="cuda")
    good = (vp * 1)(d.data_ptr())
    off = (vp * 1)(d.data_ptr() + 4)
    for raw in (dict(depth=off), dict(normal=off), dict(bgr=off), dict(hits=vp(d.data_ptr() + 4)), dict(info=vp(d.data_ptr() + 8))):
        assert _call(m, c["cells"], c["color"], c["lo"], c["views"], device_tsdf=True, device_out=True, raw=raw)[0] == INVALID_ARG, list(raw)
    assert _call(m, c["cells"], c["color"], c["lo"], c["views"], device_tsdf=True, device_out=True, raw=dict(tsdf=vp(d.data_ptr() + 8)))[0] == INVALID_ARG
    assert _call(m, c["cells"], c["color"], c["lo"], c["views"], device_tsdf=True, device_out=True, raw=dict(depth=good))[0] == 0
    # the API's own checks
    vol = api.TsdfVolume(c["cells"], c["lo"], rc.V, None)
    with pytest.raises(ValueError):
        m.surface_raycast(vol, T, colors=True)  # no colour volume
    with pytest.raises(ValueError):
        m.surface_raycast(vol, np.zeros((65, 4, 4), F), colors=False)
    with pytest.raises(ValueError):
        m.surface_raycast(api.TsdfVolume(c["cells"], c["lo"], 0.5, None), T, colors=False)  # another voxel edge
    with pytest.raises(api.RevoError):
        m.surface_raycast(vol, T, colors=False, step=-1.0)
    m.close()


# ------------------------------------------------------------------------------------------------------------------ the API --
def test_fuse_then_raycast_on_the_device():
    """api.SurfaceVolume: two views fused into the device volumes, ray-cast from there without a host copy; the call only enqueues."""
    import torch
    w = tc.wall()
    m = tt._map()
    surf = api.SurfaceVolume(m, w["lo"], w["n"])
    tilted = np.eye(4, dtype=F)
    tilted[0, 3] = 0.1
    rng = np.random.default_rng(28)
    views = [(w["views"][0][0], np.eye(4, dtype=F), sc.KC), (w["views"][0][0], tilted, sc.KC)]
    bgr = [rng.integers(0, 256, (12, 16, 3), dtype=np.uint8) for _ in views]
    for (d, T, k), im in zip(views, bgr):
        surf.integrate((torch.from_numpy(d).cuda(), T, k, torch.from_numpy(im).cuda()))
    poses = [np.eye(4, dtype=F), tilted, rc.at(np.eye(4, dtype=F), 0.0, 0.05, -0.1)]
    kw = dict(camera=sc.KC[:4], size=rc.SIZE, zrange=sc.KC[4:])
    dev = surf.raycast(poses, device=True, **kw)  # enqueued behind the two fuse calls; nothing has been waited for
    got = surf.raycast(poses, **kw)
    vol = surf.volume()
    want = mapfile.tsdf_raycast_records(vol.cells, vol.color, w["lo"], tc.V, [(T, sc.KC, rc.SIZE) for T in poses])
    assert vol.cells.tobytes() == mapfile.tsdf_records(tc.V, w["lo"], w["n"], views, bgr=bgr)[0].tobytes()
    assert want["info"]["hits"] > 35 and want["info"]["uncolored"] == 0  # the front view alone has 35
    for i in range(3):
        assert got["depth"][i].tobytes() == want["depth"][i].tobytes() and got["normals"][i].tobytes() == want["normals"][i].tobytes()
        assert got["bgr"][i].tobytes() == want["bgr"][i].tobytes()
        assert dev["depth"][i].cpu().numpy().tobytes() == want["depth"][i].tobytes() and dev["bgr"][i].cpu().numpy().tobytes() == want["bgr"][i].tobytes()
    assert got["hits"] == want["hits"] == dev["hits"].cpu().numpy().tolist() and got["info"] == want["info"]
    assert dev["info"].cpu().numpy().tolist()[:7] == [want["info"][k] for k in mapfile.TSDF_RAY_INFO_KEYS]
    one = surf.raycast(tilted, normals=False, colors=False, step=0.05, **kw)
    fine = mapfile.tsdf_raycast_records(vol.cells, None, w["lo"], tc.V, [(tilted, sc.KC, rc.SIZE)], step=0.05)
    assert one["depth"].tobytes() == fine["depth"][0].tobytes() and one["normals"] is None and one["bgr"] is None and one["hits"] == fine["hits"][0]
    # the downloaded volume ray-casts on its map, the same bytes
    again = vol.raycast(poses, **kw)
    assert all(again["depth"][i].tobytes() == want["depth"][i].tobytes() and again["bgr"][i].tobytes() == want["bgr"][i].tobytes() for i in range(3))
    plain = api.SurfaceVolume(m, w["lo"], w["n"], color=False)
    assert plain.raycast(tilted, **kw)["bgr"] is None
    m.close()


def test_the_pyramid_form_and_the_window():
    import torch
    _, cam, pyrs, _ = tr._scene()
    T = tr._kf_poses()
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    lo, n = (-58, -11, 171), (24, 20, 30)
    v = m.fuse([(pyrs[0], T[0]), (pyrs[1], T[1])], lo=lo, n=n, color=True)
    s = cc.settings320()
    half = (s.fx / 4, s.fy / 4, (s.cx + 0.5) / 4 - 0.5, (s.cy + 0.5) / 4 - 0.5)
    zr = (s.depth_min, s.depth_max)
    views = [(T[i], half + zr, (80, 60)) for i in (0, 1, 2)]
    want = mapfile.tsdf_raycast_records(v.cells, v.color, lo, cc.VOXEL, views)
    assert want["info"]["hits"] > 0
    got = v.raycast(T[:3], camera=half, size=(80, 60), zrange=zr)
    for i in range(3):
        assert got["depth"][i].tobytes() == want["depth"][i].tobytes() and got["normals"][i].tobytes() == want["normals"][i].tobytes()
        assert got["bgr"][i].tobytes() == want["bgr"][i].tobytes()
    assert got["hits"] == want["hits"] and got["info"] == want["info"]
    # the context's own camera, size and range by default
    full = v.raycast(T[0], normals=False)
    wf = mapfile.tsdf_raycast_records(v.cells, v.color, lo, cc.VOXEL, [(T[0], cc.intrinsics320(), (s.width, s.height))])
    assert full["depth"].shape == (s.height, s.width) and full["depth"].tobytes() == wf["depth"][0].tobytes() and full["bgr"].tobytes() == wf["bgr"][0].tobytes()
    # between device tensors
    d_t, d_c = tt._as_tensor(v.cells), ts._col_tensor(v.color)
    d_depth = torch.zeros((3, 60, 80), dtype=torch.float32, device="cuda")
    d_nrm = torch.zeros((3, 60, 80, 3), dtype=torch.float32, device="cuda")
    d_bgr = torch.zeros((3, 60, 80, 3), dtype=torch.uint8, device="cuda")
    d_hits, d_info = torch.zeros(4, dtype=torch.int32, device="cuda")[:3], torch.zeros(8, dtype=torch.int64, device="cuda")
    m.surface_raycast_into(d_depth, d_t, lo, T[:3], camera=half, size=(80, 60), zrange=zr, d_normals=d_nrm, d_bgr=d_bgr, d_color=d_c, d_hits=d_hits, d_info=d_info)
    assert d_depth.cpu().numpy().tobytes() == np.stack(want["depth"]).tobytes() and d_nrm.cpu().numpy().tobytes() == np.stack(want["normals"]).tobytes()
    assert d_bgr.cpu().numpy().tobytes() == np.stack(want["bgr"]).tobytes() and d_hits.cpu().numpy().tolist() == want["hits"]
    with pytest.raises(ValueError):
        m.surface_raycast_into(d_depth, d_t, lo, T[:3], camera=half, size=(80, 60), zrange=zr, d_bgr=d_bgr)  # d_bgr needs d_color
    with pytest.raises(ValueError):
        m.surface_raycast_into(d_depth[:2], d_t, lo, T[:3], camera=half, size=(80, 60), zrange=zr)
    # MapWindow forwards
    win = api.MapWindow(cam, cc.VOXEL, dense=True, window=2)
    ws = win.surface_raycast(v, T[:3], camera=half, size=(80, 60), zrange=zr)
    assert all(ws["depth"][i].tobytes() == want["depth"][i].tobytes() and ws["bgr"][i].tobytes() == want["bgr"][i].tobytes() for i in range(3))
    d_depth.zero_()
    win.surface_raycast_into(d_depth, d_t, lo, T[:3], camera=half, size=(80, 60), zrange=zr)
    assert d_depth.cpu().numpy().tobytes() == np.stack(want["depth"]).tobytes()
    win.close()
    m.close()


def test_the_scene_box():
    """The 64^3 box of DESIGN 19's scene, fused from its four views and seen from those four poses with the views' camera at a
    quarter of its resolution (the numpy restatement marches every ray of a view in step)."""
    lo, n, views = tc.scene64()
    vol = tt._scene64()[3][0]
    s = cc.settings320()
    poses = [v[1] for v in views]
    quarter = (s.fx / 4, s.fy / 4, (s.cx + 0.5) / 4 - 0.5, (s.cy + 0.5) / 4 - 0.5)
    zr = (s.depth_min, s.depth_max)
    want = mapfile.tsdf_raycast_records(vol, None, lo, cc.VOXEL, [(T, quarter + zr, (80, 60)) for T in poses])
    m = tt._map(voxel=cc.VOXEL)
    got = m.surface_raycast(api.TsdfVolume(vol, lo, cc.VOXEL, None), poses, camera=quarter, size=(80, 60), zrange=zr, colors=False)
    print("scene 64^3:", want["info"])
    assert want["info"]["hits"] > 500
    for i in range(4):
        assert got["depth"][i].tobytes() == want["depth"][i].tobytes(), (i, int(np.sum(got["depth"][i] != want["depth"][i])))
        assert got["normals"][i].tobytes() == want["normals"][i].tobytes(), i
    assert got["hits"] == want["hits"] and got["info"] == want["info"] and got["bgr"] is None
    m.close()


def test_run_tum_surface_views(tmp_path, monkeypatch, capsys):
    import os
    import re
    from lm_settings_cases import S160
    from revo_amd import run_tum, tum
    from test_gpu_vo_multi import _tum_yaml
    name = "rgbd_synth_s"
    tum.write_synthetic_dataset(str(tmp_path / "data" / name), ts._two_keyframes(S160)[:12])
    _tum_yaml(tmp_path, S160, [name])
    monkeypatch.chdir(tmp_path)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "0", "--map", "0.05"]
    surface = ["--surface", "surface.ply", "--surface-box", "-40", "-40", "0", "80", "80", "100", "--surface-trunc", "0.2"]
    assert run_tum.main(args + surface + ["--surface-views", "sviews"]) == 0
    out = capsys.readouterr().out
    keyframes = int(re.search(r"Keyframes Tracked: (\d+)", out).group(1))
    folder = str(tmp_path / "sviews")
    rows = tum.read_associate(os.path.join(folder, "associate.txt"))
    assert "Surface views: %d views (one per keyframe)" % keyframes in out and len(rows) == keyframes >= 1
    assert len(tum.read_poses(os.path.join(folder, "poses.txt"))) == keyframes
    for _, rf, _, df in rows:
        bgr, depth = tum.load_frame(folder, rf, df)
        assert bgr.shape == (S160.height, S160.width, 3) and depth.shape == (S160.height, S160.width) and depth.dtype == np.uint16
        assert (depth > 0).sum() > 1000 and bgr[depth > 0].any() and not bgr[depth == 0].any()  # a miss is black, and the surface is there
    assert run_tum.main(args + surface + ["--surface-views", "every", "--surface-views-every", "5"]) == 0
    assert len(tum.read_associate(str(tmp_path / "every" / "associate.txt"))) == 3  # frames 0, 5 and 10 of 12
    # usage errors
    assert run_tum.main(args + ["--surface-views", "x"]) == 2 and run_tum.main(args + surface + ["--surface-views-every", "2"]) == 2
    capsys.readouterr()
