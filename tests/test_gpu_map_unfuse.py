"""Views taken out of the TSDF surface again, on the device (revo_map_tsdf_unfuse, api.VoxelMap.unfuse / unfuse_into,
api.TsdfVolume.unfuse, api.SurfaceVolume.remove / repose, api.SurfaceWindow, vo.REVO(voxelMap=MapWindow, surface=SurfaceWindow);
DESIGN 32): both volumes, info and view_info byte for byte revo_amd.mapfile's restatement (which test_map_unfuse_cpu.py pins to the
per-cell specification) on every shared case, from host and device images out of host and device volumes, with guard cells behind
the volumes; the exact properties; the pyramid form; every refusal with its misfit count and every byte of both volumes compared
with a copy; every argument error; the window against fresh fuses; the running sequence."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile, synth  # noqa: E402
from revo_amd.settings import MapTsdfUnfuseInfo  # noqa: E402

import map_seen_cases as sc  # noqa: E402
import map_surface_cases as su  # noqa: E402
import map_tsdf_cases as tc  # noqa: E402
import map_unfuse_cases as uc  # noqa: E402
import test_gpu_map_surface as ts  # noqa: E402
import test_gpu_map_tsdf as tt  # noqa: E402

F = np.float32
CELL, COLOR = mapfile.TSDF_CELL_DTYPE, mapfile.TSDF_COLOR_DTYPE
INVALID_ARG = -1
GUARD = 4  # cells behind each volume that no call may write
vp = C.c_void_p


def _guarded(vol, sentinel):
    """The volume's cells, flat, with GUARD sentinel cells behind them."""
    out = np.full(vol.size + GUARD, sentinel, vol.dtype)
    out[:vol.size] = np.ascontiguousarray(vol).reshape(-1)
    return out


def _unfuse(m, lo, n, views, bgr, trunc, cells, color=None, device=False, device_in=False, with_info=True):
    """revo_map_tsdf_unfuse out of host or device volumes that hold `cells` (and `color`; None: no colour volume, no images)
    -> (rc, cells', color', info list of 8, per-view counts); info and view_info start as nines, the guard cells are checked."""
    import torch
    L = _lib.lib()
    with_color = color is not None
    if with_color:
        views = [tuple(v[:3]) + (im,) for v, im in zip(views, bgr)]
        if device_in:
            views = [(torch.from_numpy(np.ascontiguousarray(v[0], F)).cuda(), v[1], v[2], torch.from_numpy(np.ascontiguousarray(v[3])).cuda()) for v in views]
        cv, din, keep, ptrs, keep_c = m._color_views(views)
    else:
        if device_in:
            views = [(torch.from_numpy(np.ascontiguousarray(v[0], F)).cuda(),) + tuple(v[1:3]) for v in views]
        cv, din, keep = m._carve_views([tuple(v[:3]) for v in views])
        ptrs, keep_c = None, None
    nv = len(cv)
    shape = tuple(int(x) for x in n)
    box = tt._box(lo, n)
    g_cells = _guarded(np.ascontiguousarray(cells, CELL), tt.SENTINEL)
    g_col = _guarded(np.ascontiguousarray(color, COLOR), ts.SENTINEL) if with_color else None
    info = np.full(8, 9, np.uint64)
    tr_ = float(0.0 if trunc is None else trunc)
    if device:
        d = torch.from_numpy(g_cells.view(np.int32).copy()).cuda()
        dc = torch.from_numpy(g_col.view(np.int32).copy()).cuda() if with_color else None
        vi = torch.full((8 * nv,), 9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = L.revo_map_tsdf_unfuse(m._h, C.byref(box), nv, cv, C.cast(ptrs, vp) if with_color else None, din, tr_, vp(d.data_ptr()),
                                    vp(dc.data_ptr()) if with_color else None, 1, C.cast(info.ctypes.data, C.POINTER(MapTsdfUnfuseInfo)) if with_info else None,
                                    vp(vi.data_ptr()))
        m.sync()
        g_cells = d.cpu().numpy().view(CELL).reshape(-1)
        g_col = dc.cpu().numpy().view(COLOR).reshape(-1) if with_color else None
        vi = vi.cpu().numpy().view(np.uint32).reshape(nv, 8)
    else:
        vinfo = np.full((nv, 8), 9, np.uint32)
        rc = L.revo_map_tsdf_unfuse(m._h, C.byref(box), nv, cv, C.cast(ptrs, vp) if with_color else None, din, tr_, g_cells.ctypes.data_as(vp),
                                    g_col.ctypes.data_as(vp) if with_color else None, 0, C.cast(info.ctypes.data, C.POINTER(MapTsdfUnfuseInfo)) if with_info else None,
                                    vinfo.ctypes.data_as(vp))
        vi = vinfo
    del keep, keep_c
    size = int(np.prod(shape))
    assert g_cells[size:].tobytes() == np.full(GUARD, tt.SENTINEL, CELL).tobytes(), "a guard cell behind the TSDF volume was written"
    assert not with_color or g_col[size:].tobytes() == np.full(GUARD, ts.SENTINEL, COLOR).tobytes(), "a guard cell behind the colour volume was written"
    assert not vi[:, 6:].any()
    counts = [dict(zip(mapfile.CARVE_CLASSES, (int(x) for x in row[:6]))) for row in vi]
    return rc, g_cells[:size].reshape(shape).copy(), g_col[:size].reshape(shape).copy() if with_color else None, info.tolist(), counts


def _info(info):
    assert info[7] == 0
    return dict(zip(mapfile.TSDF_UNFUSE_INFO_KEYS, (int(x) for x in info[:7])))


# ------------------------------------------------------------------------------------------------------------ the cases --
@pytest.mark.parametrize("name", list(uc.cases()))
def test_unfuse_cases_bit_exact(name):
    c = uc.cases()[name]
    views, bgr = uc.pick(c, c["removed"])
    all_views, all_bgr = uc.pick(c, range(len(c["views"])))
    full = mapfile.tsdf_records(uc.V, c["lo"], c["n"], all_views, c["trunc"], bgr=all_bgr)
    want = mapfile.tsdf_unfuse_records(full[0], full[3], c["lo"], uc.V, views, c["trunc"], bgr=bgr)
    plain = mapfile.tsdf_unfuse_records(full[0], None, c["lo"], uc.V, views, c["trunc"])
    m = tt._map()
    before = m.export_raw().tobytes()
    for device, device_in in tt.SIDES:
        rc, cells, col, info, counts = _unfuse(m, c["lo"], c["n"], views, bgr, c["trunc"], full[0], full[3], device, device_in)
        assert rc == 0, (name, device, device_in, _lib.lib().revo_last_error())
        assert cells.tobytes() == want[0].tobytes(), (name, device, device_in, int(np.sum(cells != want[0])))
        assert col.tobytes() == want[1].tobytes(), (name, device, device_in, int(np.sum(col != want[1])))
        assert _info(info) == want[2] and counts == want[3], (name, device, device_in, _info(info), want[2])
    for device in (False, True):  # without a colour volume: the TSDF bytes are the same, no colour counter moves
        rc, cells, col, info, counts = _unfuse(m, c["lo"], c["n"], views, None, c["trunc"], full[0], None, device, device)
        assert rc == 0 and col is None and cells.tobytes() == want[0].tobytes() and _info(info) == plain[2] and counts == want[3], (name, device)
    print(name, want[2])
    if not c["kept"]:
        assert not want[0].view(np.uint8).any() and not want[1].view(np.uint8).any()  # everything out: all-zero volumes
    else:  # what is left is the fuse of the kept views alone
        kv, kb = uc.pick(c, c["kept"])
        kept = mapfile.tsdf_records(uc.V, c["lo"], c["n"], kv, c["trunc"], bgr=kb)
        assert want[0].tobytes() == kept[0].tobytes() and want[1].tobytes() == kept[3].tobytes()
    assert m.export_raw().tobytes() == before
    m.close()


def test_the_exact_properties():
    c = su.fuse_cases()["64 views"]
    lo, n, views, bgr = c["lo"], c["n"], c["views"][:8], c["bgr"][:8]
    A, B = [0, 2, 5], [1, 3, 4, 6, 7]
    sub = lambda idx: ([views[i] for i in idx], [bgr[i] for i in idx])  # noqa: E731
    want = mapfile.tsdf_records(tc.V, lo, n, *sub(A)[:1], bgr=sub(A)[1])
    m = tt._map(sc.records_at([(0, 0, 8), (-4, -3, 6)]))  # a map with voxels in the box: they play no part
    before = m.export_raw().tobytes()
    results = []
    for device in (False, True):
        kw = dict(device=device, device_in=device)
        # A and B fused in any order and any split into accumulating calls ...
        for order, cut in ((A + B, 8), (B + A, 3), ([7, 0, 6, 1, 5, 2, 4, 3], 5)):
            ov, ob = sub(order)
            f = ts._fuse(m, lo, n, ov[:cut], ob[:cut], device=device)
            if cut < 8:
                f = ts._fuse(m, lo, n, ov[cut:], ob[cut:], before=(f[0], f[3]), device=device)
            # ... then B taken out in any split
            for parts in ([B], [B[::-1]], [B[:2], B[2:]], [[b] for b in B]):
                cells, col = f[0], f[3]
                infos = []
                for part in parts:
                    rc, cells, col, info, counts = _unfuse(m, lo, n, *sub(part), None, cells, col, **kw)
                    assert rc == 0
                    infos.append(_info(info))
                    # view_info is the fuse's for the same views
                    assert counts == ts._fuse(m, lo, n, *sub(part), device=device)[2]
                assert cells.tobytes() == want[0].tobytes() and col.tobytes() == want[3].tobytes(), (device, order, parts)
                assert sum(i["updates"] for i in infos) == int(f[0]["weight"].sum()) - int(want[0]["weight"].sum())
                assert infos[-1]["cells_weighted"] == want[1]["cells_weighted"] and infos[-1]["cells_colored"] == want[4]["cells_colored"]
                results.append((cells.tobytes(), col.tobytes()))
        # everything out: zeros
        f = ts._fuse(m, lo, n, views, bgr, device=device)
        rc, cells, col, info, _ = _unfuse(m, lo, n, views, bgr, None, f[0], f[3], **kw)
        assert rc == 0 and not cells.view(np.uint8).any() and not col.view(np.uint8).any()
        assert _info(info) == {"cells": cells.size, "updates": f[1]["updates"], "cells_weighted": 0, "cells_inside": 0, "misfits": 0,
                               "color_updates": f[4]["color_updates"], "cells_colored": 0}
        # info may be NULL: the same bytes
        rc, c2, k2, info, _ = _unfuse(m, lo, n, *sub(B), None, f[0], f[3], with_info=False, **kw)
        assert rc == 0 and info == [9] * 8 and c2.tobytes() == want[0].tobytes() and k2.tobytes() == want[3].tobytes()
    assert len(set(results)) == 1  # a host volume and a device volume give the same bytes
    assert m.export_raw().tobytes() == before
    m.close()


def test_the_pyramid_form_is_the_raw_form():
    import torch
    from lm_settings_cases import S160
    frames = ts._two_keyframes(S160)[:2]
    cam = api.CameraPyr(S160)
    m = api.VoxelMap(cam, 0.05, dense=True)
    lo, n = (-40, -40, 0), (33, 30, 41)
    T = [np.eye(4, dtype=F), np.eye(4, dtype=F)]
    T[1][0, 3] = F(0.0625)
    pyrs = [api.ImgPyramidRGBD(S160, cam, f[0], f[1], f[2]) for f in frames]
    raw = [(p.returnDepth(0).copy(), T_, None, np.ascontiguousarray(f[0])) for p, T_, f in zip(pyrs, T, frames)]
    full = m.fuse([(p, T_) for p, T_ in zip(pyrs, T)], lo=lo, n=n, color=True)
    assert full.cells.tobytes() == m.fuse(raw, lo=lo, n=n, color=True).cells.tobytes() and full.info["cells_inside"] > 0
    a = m.unfuse(full, [(pyrs[1], T[1])])          # the pyramid brings its depth and colour planes
    b = m.unfuse(full, [raw[1]])                   # the raw view of its level-0 planes
    assert a.cells.tobytes() == b.cells.tobytes() and a.color.tobytes() == b.color.tobytes()
    assert a.info == b.info and a.view_info == b.view_info and a.info["updates"] > 0 and a.info["color_updates"] > 0 and a.info["misfits"] == 0
    one = m.fuse([(pyrs[0], T[0])], lo=lo, n=n, color=True)
    assert a.cells.tobytes() == one.cells.tobytes() and a.color.tobytes() == one.color.tobytes()
    assert full.unfuse([(pyrs[1], T[1])]).cells.tobytes() == one.cells.tobytes()  # TsdfVolume.unfuse on its map
    # between device tensors, pyramid and device raw views together; MapWindow forwards both calls
    d = tt._as_tensor(full.cells)
    dc = ts._col_tensor(full.color)
    win = api.MapWindow(cam, 0.05, dense=True, window=2)
    dv = [(pyrs[0], T[0]), (torch.from_numpy(raw[1][0]).cuda(), T[1], None, torch.from_numpy(raw[1][3]).cuda())]
    info = m.unfuse_into(d, dv, lo, d_color=dc)
    assert info["cells_weighted"] == 0 and not d.cpu().numpy().any() and not dc.cpu().numpy().any()
    assert win.unfuse(full, [raw[1]]).cells.tobytes() == one.cells.tobytes()
    with pytest.raises(api.RevoError) as e:  # nothing is left to take
        win.unfuse_into(d, dv[:1], lo, d_color=dc)
    assert e.value.code == INVALID_ARG and e.value.misfits == e.value.info["misfits"] > 0 and not d.cpu().numpy().any()
    win.close()
    m.close()


# --------------------------------------------------------------------------------------------------------- the refusals --
@pytest.mark.parametrize("name", list(uc.refusals()))
def test_refusals_change_no_byte(name):
    r = uc.refusals()[name]
    m = tt._map()
    tried = 0
    for color in (True, False):
        if (color and r.get("tsdf_only")) or (not color and r.get("color_only")):
            continue
        with pytest.raises(mapfile.TsdfUnfuseRefused) as e:
            mapfile.tsdf_unfuse_records(r["cells"], r["color"] if color else None, r["lo"], uc.V, r["views"], r["trunc"], bgr=r["bgr"] if color else None)
        assert e.value.misfits == r["misfits"]
        for device, device_in in tt.SIDES:
            rc, cells, col, info, counts = _unfuse(m, r["lo"], r["n"], r["views"], r["bgr"] if color else None, r["trunc"], r["cells"],
                                                   r["color"] if color else None, device, device_in)
            assert rc == INVALID_ARG and b"do not fit" in _lib.lib().revo_last_error(), (name, color, device, rc)
            assert _info(info) == e.value.info, (name, color, device, _info(info), e.value.info)
            assert cells.tobytes() == r["cells"].tobytes() and (not color or col.tobytes() == r["color"].tobytes()), (name, color, device)
            assert counts == mapfile.tsdf_records(uc.V, r["lo"], r["n"], r["views"], r["trunc"])[2]  # the classes are what they are
            tried += 1
    assert tried
    # the handle is as usable as before
    c = uc.cases()["3x3x5 / all"]
    full = mapfile.tsdf_records(uc.V, c["lo"], c["n"], c["views"], c["trunc"], bgr=c["bgr"])
    rc, cells, col, _, _ = _unfuse(m, c["lo"], c["n"], c["views"], c["bgr"], c["trunc"], full[0], full[3], True, True)
    assert rc == 0 and not cells.view(np.uint8).any() and not col.view(np.uint8).any()
    m.close()


# -------------------------------------------------------------------------------------------------------------- arguments --
def test_argument_errors_write_nothing():
    import torch
    L = _lib.lib()
    m = tt._map()
    lo, n = (-2, -1, 6), (4, 3, 5)
    good = tt._box(lo, n)
    t = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    base = t.data_ptr()
    dp = lambda off: vp(base + off)  # noqa: E731
    depth, img = np.full((12, 16), tc.WALL_DEPTH, F), su.wall_image()
    cv, _, keep = m._carve_views([(depth, sc.I4, sc.KC)])
    one = (C.c_void_p * 1)(img.ctypes.data)
    none = (C.c_void_p * 1)()
    vol, col = np.full(60, tt.SENTINEL, CELL), np.full(60, ts.SENTINEL, COLOR)
    info, vinfo = np.full(8, 9, np.uint64), np.full(8, 9, np.uint32)
    sp, cp, vip = (x.ctypes.data_as(vp) for x in (vol, col, vinfo))
    ip = C.cast(info.ctypes.data, C.POINTER(MapTsdfUnfuseInfo))

    def unfuse(box=good, nv=1, views=cv, bgr=one, din=0, trunc=0.25, s=sp, c=cp, dev=0, i=ip, vi=vip, mm=m):
        return L.revo_map_tsdf_unfuse(mm._h if mm is not None else None, C.byref(box) if box is not None else None, nv, views,
                                      C.cast(bgr, vp) if bgr is not None else None, din, trunc, s, c, dev, i, vi)

    pyr_like, _, k2 = m._carve_views([(depth, sc.I4, sc.KC)])
    pyr_like[0].depth, pyr_like[0].kf = None, 1 << 12  # a pyramid view (never followed: the bgr rule comes first)
    bad = [unfuse(mm=None), unfuse(box=None), unfuse(views=None), unfuse(s=None),           # NULLs
           unfuse(bgr=None), unfuse(c=None),                                                 # bgr without color, color without bgr
           unfuse(bgr=none), unfuse(views=pyr_like, bgr=one),                                # a bgr[i] that does not match its view's kind
           unfuse(nv=0), unfuse(nv=65), unfuse(nv=-1),
           unfuse(trunc=-0.25), unfuse(trunc=float("nan")), unfuse(trunc=float("inf")),
           unfuse(din=2), unfuse(dev=2), unfuse(dev=-1),                                     # a bad flag
           unfuse(box=tt._box((0, 0, 0), (0, 3, 5))),
           unfuse(s=dp(8), c=dp(2048), dev=1, vi=None), unfuse(s=dp(0), c=dp(2048 + 8), dev=1, vi=None),  # a misaligned device pointer
           unfuse(s=dp(0), c=dp(2048), dev=1, vi=dp(4096 + 8))]
    assert bad == [INVALID_ARG] * len(bad), bad
    assert L.revo_last_error()
    m.sync()
    assert vol.tobytes() == np.full(60, tt.SENTINEL, CELL).tobytes() and col.tobytes() == np.full(60, ts.SENTINEL, COLOR).tobytes()
    assert np.all(info == 9) and np.all(vinfo == 9) and not t.cpu().numpy().any()
    # the handle is as usable as before: fuse, then take it out again, info and view_info NULL or given, trunc 0 the default
    want = mapfile.tsdf_records(tc.V, lo, n, [(depth, sc.I4, sc.KC)], 0.25, bgr=[img])
    vol[:], col[:] = want[0].reshape(-1), want[3].reshape(-1)
    assert unfuse(i=None, vi=None) == 0 and not vol.view(np.uint8).any() and not col.view(np.uint8).any() and np.all(info == 9)
    vol[:] = want[0].reshape(-1)
    assert unfuse(bgr=None, c=None) == 0 and not vol.view(np.uint8).any()
    assert info.tolist() == [60, want[1]["updates"], 0, 0, 0, 0, 0, 0] and vinfo[:6].tolist() == [want[2][0][k] for k in mapfile.CARVE_CLASSES]
    dflt = mapfile.tsdf_records(tc.V, lo, n, [(depth, sc.I4, sc.KC)])
    vol[:] = dflt[0].reshape(-1)
    assert unfuse(bgr=None, c=None, trunc=0.0) == 0 and not vol.view(np.uint8).any()
    # the Python layer's own refusals
    plain = m.fuse([(depth, sc.I4, sc.KC)], lo=lo, n=n)
    full = m.fuse([(depth, sc.I4, sc.KC, img)], lo=lo, n=n, color=True)
    for wrong in (lambda: m.unfuse(full, [(depth, sc.I4, sc.KC)]), lambda: m.unfuse(full, [(depth, sc.I4, sc.KC, img[:, :-1])]),
                  lambda: m.unfuse(plain, []), lambda: tt._map(voxel=0.25).unfuse(plain, [(depth, sc.I4, sc.KC)])):
        with pytest.raises(ValueError):
            wrong()
    assert not m.unfuse(plain, [(depth, sc.I4, sc.KC, img)]).cells.view(np.uint8).any()  # a colour image more than needed is not looked at
    assert not m.unfuse(full, [(depth, sc.I4, sc.KC, img)]).color.view(np.uint8).any()
    del keep, k2
    m.close()


# ------------------------------------------------------------------------------------------------------------ the window --
def _scene_views():
    """tc.scene64() with a seeded colour image per view -> (lo, n, host views (depth, T, intrinsics, bgr))."""
    lo, n, views = tc.scene64()
    rng = np.random.default_rng(32)
    return lo, n, [tuple(v[:3]) + (rng.integers(0, 256, np.shape(v[0]) + (3,), dtype=np.uint8),) for v in views]


def _on_device(v):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(v[0], F)).cuda(), v[1], v[2], torch.from_numpy(np.ascontiguousarray(v[3])).cuda())


def _fresh(m, lo, n, views, color=True, counts=False):
    """A fresh SurfaceVolume fused from the host views -> its TsdfVolume (counts: its per-view counts instead).  integrate only
    enqueues: the device images stay alive until the volume has been read behind the map's sync."""
    s = api.SurfaceVolume(m, lo, n, color=color)
    dev = [_on_device(v) if color else _on_device(v)[:3] for v in views]
    for v in dev:
        s.integrate(v)
    out = s.view_counts() if counts else s.volume()
    del dev
    return out


def _same_volume(got, want, what):
    assert got.cells.tobytes() == want.cells.tobytes(), (what, "tsdf", int(np.sum(got.cells != want.cells)))
    assert (got.color is None and want.color is None) or got.color.tobytes() == want.color.tobytes(), (what, "colour")


def test_surface_window_holds_the_last_views():
    import map_carve_cases as cc
    lo, n, views = _scene_views()
    m = tt._map(voxel=cc.VOXEL)
    assert len(views) == 4
    for color in (True, False):
        w = api.SurfaceWindow(m, lo, n, window=2, color=color)
        dev = [_on_device(v) if color else _on_device(v)[:3] for v in views]
        for i, v in enumerate(dev):
            w.integrate(v)
            assert w.views == min(i + 1, 2) == len(w.held_views()) == len(w.view_counts())
            _same_volume(w.volume(), _fresh(m, lo, n, views[max(0, i - 1):i + 1], color), ("window", color, i))
        assert w.view_counts() == _fresh(m, lo, n, views[2:], color, counts=True)
        held = w.held_views()
        assert held[0][0] is not dev[2][0] and torch_equal(held[0][0], dev[2][0])  # its own device copies
        # repose: the other views plus the view at T_new
        T_new = np.array(views[2][1], F)
        T_new[0, 3] += F(0.05)
        info = w.repose(held[0], views[2][1], T_new)
        assert info["misfits"] == 0 and info["updates"] > 0 and w.views == 2
        moved = tuple(views[2][:1]) + (T_new,) + tuple(views[2][2:])
        _same_volume(w.volume(), _fresh(m, lo, n, [moved, views[3]], color), ("repose", color))
        assert w.view_counts() == _fresh(m, lo, n, [moved, views[3]], color, counts=True) and np.array_equal(w.held_views()[0][1], T_new)
        # a repose from a pose the view is not at is refused and fuses nothing
        before = w.volume()
        refused = w.repose(0, views[2][1], views[2][1])
        assert refused["misfits"] > 0 and refused["updates"] == 0 and w.views == 2
        _same_volume(w.volume(), before, ("refused repose", color))
        # remove: what is left is the other view alone; then nothing
        w.remove(w.held_views()[0])
        assert w.views == 1 == len(w.held_views())
        _same_volume(w.volume(), _fresh(m, lo, n, [views[3]], color), ("remove", color))
        w.remove(0)
        vol = w.volume()
        assert w.views == 0 and w.view_counts() == [] and not vol.cells.view(np.uint8).any() and (not color or not vol.color.view(np.uint8).any())
        with pytest.raises(ValueError):
            w.remove(0)
        w.integrate(dev[0])
        w.clear()
        assert w.views == 0 and w.held_views() == [] and not w.volume().cells.view(np.uint8).any()
    # a plain SurfaceVolume: remove and repose against fresh fuses
    s = api.SurfaceVolume(m, lo, n)
    dev = [_on_device(v) for v in views]
    for v in dev[:3]:
        s.integrate(v)
    s.remove(dev[1])
    assert s.views == 2 and len(s.view_counts()) == 2
    _same_volume(s.volume(), _fresh(m, lo, n, [views[0], views[2]]), "SurfaceVolume.remove")
    with pytest.raises(api.RevoError) as e:  # it is no longer in the volumes
        s.remove(dev[1])
    assert e.value.misfits > 0 and s.views == 2
    T_new = np.array(views[0][1], F)
    T_new[2, 3] -= F(0.03)
    assert s.repose(dev[0], views[0][1], T_new)["misfits"] == 0 and s.views == 2
    _same_volume(s.volume(), _fresh(m, lo, n, [views[2], tuple(views[0][:1]) + (T_new,) + tuple(views[0][2:])]), "SurfaceVolume.repose")
    with pytest.raises(ValueError):
        api.SurfaceWindow(m, lo, n, window=0)
    m.close()


def test_integrate_keeps_the_images_it_has_enqueued():
    """integrate only enqueues on the map's stream, which torch's allocator does not know: every device image is dropped right
    behind its call here, and the next view's upload may get its memory."""
    import map_carve_cases as cc
    lo, n, views = _scene_views()
    m = tt._map(voxel=cc.VOXEL)
    s = api.SurfaceVolume(m, lo, n)
    rounds = 3
    for v in views * rounds:
        s.integrate(_on_device(v))
    assert len(s._pending) == len(views) * rounds and all(len(p) == 2 for p in s._pending)
    got = s.volume()
    assert s._pending == []
    want = m.fuse(views * rounds, lo=lo, n=n, color=True)
    _same_volume(got, want, "temporaries")
    # past 64 enqueued raw views the surface waits for the stream itself and lets go of them
    t = api.SurfaceVolume(m, (0, 0, 40), (4, 4, 4), color=False)
    for _ in range(70):
        t.integrate(_on_device(views[0])[:3])
    assert len(t._pending) == 70 - 64 and t.views == 70
    m.close()


def test_remove_needs_its_row_and_a_refused_eviction_keeps_every_view():
    import map_carve_cases as cc
    import torch
    lo, n, views = _scene_views()
    m = tt._map(voxel=cc.VOXEL)
    dev = [_on_device(v) for v in views]
    s = api.SurfaceVolume(m, lo, n)
    s.integrate(dev[0])
    s.integrate(dev[1])
    m.sync()
    t = api.SurfaceVolume(m, lo, n)  # the same volumes, and no view integrated through it
    t.d_tsdf.copy_(s.d_tsdf)
    t.d_color.copy_(s.d_color)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError) as e:
        t.remove(dev[0])
    assert not isinstance(e.value, api.RevoError) and t.views == 0 and t.view_counts() == []
    _same_volume(t.volume(), _fresh(m, lo, n, views[1:2]), "the unfuse itself took place")
    with pytest.raises(RuntimeError):
        s.remove(dev[0], index=5)
    # a window whose oldest view sits in cells of full weight: the eviction is refused, the new view stays fused and held
    w = api.SurfaceWindow(m, lo, n, window=1)
    w.integrate(dev[0])
    m.sync()
    hit = w.d_tsdf[..., 1] > 0
    assert bool(hit.any())
    w.d_tsdf[..., 1][hit] = 1 << 20
    torch.cuda.synchronize()
    before = w.volume()
    with pytest.raises(api.RevoError) as e:
        w.integrate(dev[1])
    assert e.value.misfits > 0 and w.views == 2 == len(w.held_views()) == len(w.view_counts())
    after = w.volume()
    assert np.array_equal(after.cells["weight"][before.cells["weight"] == (1 << 20)], before.cells["weight"][before.cells["weight"] == (1 << 20)])
    assert int(after.cells["weight"].sum()) > int(before.cells["weight"].sum())  # the new view is in the volumes
    m.close()


def torch_equal(a, b):
    import torch
    return bool(torch.equal(a, b))


# ------------------------------------------------------------------------------------------------------------ the driver --
def test_the_running_sequence_keeps_a_window():
    from lm_settings_cases import S160
    from revo_amd import vo
    frames = synth.make_sequence(41, S160, 40, max_t=0.01, max_rot_deg=0.4, bias=[0, 0, 0, 0, np.deg2rad(1.5), 0])
    cam = api.CameraPyr(S160)
    lo, n = (-40, -40, 0), (80, 80, 100)
    by_ts = {float(f[2]): f[0] for f in frames}
    vm = api.VoxelMap(cam, 0.05, dense=True)
    for track in (None, True):  # surface_track=True tracks against the window's surface and fuses at the refined pose
        win = api.MapWindow(cam, 0.05, dense=True, window=2)
        surf = api.SurfaceWindow(win, lo, n, window=2)
        g = vo.REVO(S160, cameraPyr=cam, voxelMap=win, surface=surf, surface_track=track)
        kfs = []
        for f in frames:
            _, kf = g.push(f[0], f[1], f[2])
            if kf:
                pyr, T = g.keyframe()
                T = np.array(T if track is None else g.surface_tracks[-1][2], F)  # the pose it was fused at
                kfs.append((pyr.returnDepth(0).copy(), T, None, np.ascontiguousarray(by_ts[float(pyr.returnTimestamp())])))
            if len(kfs) == 4:
                break
        print("track", track, "keyframes", len(kfs), "frames", len(g.poses), [t[4] for t in g.surface_tracks])
        assert len(kfs) >= 3 and g.surface_skipped == 0, "the sequence gives at least three keyframes"
        assert surf.views == 2 == len(surf.held_views()) == len(win.keyframes)
        assert all(np.array_equal(h[1], k[1]) for h, k in zip(surf.held_views(), kfs[-2:]))  # the window's keyframes at their reported poses
        got = surf.volume()
        want = vm.fuse(kfs[-2:], lo=lo, n=n, color=True)
        _same_volume(got, want, ("the running window", track))
        assert want.color_info["cells_colored"] > 0 and got.trunc == want.trunc
        assert [c["confirmed"] for c in surf.view_counts()] == [c["confirmed"] for c in want.view_info]
        assert len(g._window_bgr) <= 2  # the frames' colour images are not kept beyond the keyframe decision
        if track:
            assert len(g.surface_tracks) == len(kfs)
        else:  # a plain SurfaceVolume with a MapWindow is still refused, word for word; nothing is kept for another surface
            with pytest.raises(ValueError) as e:
                vo.REVO(S160, cameraPyr=cam, voxelMap=win, surface=api.SurfaceVolume(win, lo, n))
            assert str(e.value) == "surface is not supported with a MapWindow: the volumes keep what the window evicts"
            assert vo.REVO(S160, cameraPyr=cam, voxelMap=vm, surface=api.SurfaceVolume(vm, lo, n))._window_bgr is None
        win.close()
    vm.close()


def test_run_tum_surface_window(tmp_path, monkeypatch, capsys):
    from lm_settings_cases import S160
    from revo_amd import run_tum, tum
    from test_gpu_vo_multi import _tum_yaml
    name = "rgbd_synth_w"
    frames = synth.make_sequence(41, S160, 24, max_t=0.01, max_rot_deg=0.4, bias=[0, 0, 0, 0, np.deg2rad(1.5), 0])
    tum.write_synthetic_dataset(str(tmp_path / "data" / name), frames)
    _tum_yaml(tmp_path, S160, [name])
    monkeypatch.chdir(tmp_path)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "0", "--map", "0.05"]
    box = ["--surface-box", "-40", "-40", "0", "80", "80", "100"]
    assert run_tum.main(args + ["--surface", "window.ply", "--surface-window", "2", "--map-window", "2"] + box) == 0
    mesh = mapfile.Mesh.load_ply(str(tmp_path / "window.ply"))
    out = capsys.readouterr().out
    assert len(mesh.triangles) > 0 and mesh.colors is not None and "from 2 keyframes" in out and "Map window: the last 2 of" in out
    # the window alone, without --map-window
    assert run_tum.main(args + ["--surface", "alone.ply", "--surface-window", "1"] + box) == 0
    assert "from 1 keyframes" in capsys.readouterr().out
    # usage errors, each with a message
    for bad in (["--surface-window", "2"], ["--surface", "s.ply", "--surface-window", "0"], ["--surface", "s.ply", "--surface-window", "x"],
                ["--surface", "s.ply", "--surface-window", "2", "--surface-follow"], ["--surface", "s.ply", "--surface-window", "2", "--streams", "2"],
                ["--surface", "s.ply", "--map-window", "2"]):
        assert run_tum.main(args + bad) == 2, bad
        assert capsys.readouterr().out.strip(), bad


def test_the_threaded_run_feeds_the_window():
    """REVO.run's default: submit on the producer thread, track_next on the caller's.  The colour images the driver keeps for the
    window are written by the one and read and pruned by the other; the result is the single-threaded run's, byte for byte."""
    from lm_settings_cases import S160
    from revo_amd import vo
    frames = synth.make_sequence(41, S160, 40, max_t=0.01, max_rot_deg=0.4, bias=[0, 0, 0, 0, np.deg2rad(1.5), 0])
    lo, n = (-40, -40, 0), (80, 80, 100)
    runs = []
    for threaded in (False, True):
        cam = api.CameraPyr(S160)
        win = api.MapWindow(cam, 0.05, dense=True, window=2)
        surf = api.SurfaceWindow(win, lo, n, window=2)
        g = vo.REVO(S160, cameraPyr=cam, voxelMap=win, surface=surf)
        if threaded:
            res = g.run([f[:3] for f in frames], io_thread=True, max_queue=4)
        else:
            res = [g.push(f[0], f[1], f[2]) for f in frames]
        vol = surf.volume()
        runs.append((len(res), sum(1 for _, kf in res if kf), [h[1].tobytes() for h in surf.held_views()], vol.cells.tobytes(), vol.color.tobytes(),
                     len(g._window_bgr)))
        win.close()
    print("frames", runs[0][0], "keyframes", runs[0][1])
    assert runs[0][0] == len(frames) and runs[0][1] >= 3 and runs[0][5] <= 2 and runs[1][5] <= 2 + 4  # at most the queue ahead
    assert runs[0][:5] == runs[1][:5]
    assert any(runs[0][3]) and any(runs[0][4])
