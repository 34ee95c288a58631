"""The TSDF volume and its mesh on the device (revo_map_tsdf_fuse / revo_map_tsdf_mesh, api.VoxelMap.fuse / fuse_into / mesh /
mesh_into, api.TsdfVolume): the volume's bytes, the info record and the per-view class counts bit for bit
revo_amd.mapfile's restatement (which test_map_tsdf_cpu.py pins to the per-cell specification) on every hand-made case, from host
and device images into host and device volumes; the exact properties; the mesh's vertices, triangles and counts bit for bit on
every hand-made volume, from host and device volumes into host and device outputs; caps one too small; fuse then mesh without a
host copy; every argument error; the Python API and MapWindow; the scene's 64^3 box."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile  # noqa: E402
from revo_amd.settings import MapCarveViewInfo, MapDfBox, MapMeshInfo, MapTsdfInfo, MapTsdfParams  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_seen_cases as sc  # noqa: E402
import map_tsdf_cases as tc  # noqa: E402
import test_gpu_map_raycast as tr  # noqa: E402

F = np.float32
RAW = mapfile.RAW_DTYPE
CELL = mapfile.TSDF_CELL_DTYPE
INVALID_ARG, CAPACITY = -1, -5
EMPTY = np.zeros(0, RAW)
CLASS_FIELDS = ("outside", "unknown", "free_space", "confirmed", "occluded", "edge")
SENTINEL = np.array([(0x2B2B2B2B, 0xABABABAB)], CELL)[0]


def _box(lo, n):
    return MapDfBox((C.c_int32 * 3)(*[int(x) for x in lo]), (C.c_int32 * 3)(*[int(x) for x in n]))


def _map(rec=EMPTY, voxel=tc.V):
    return tr._hand(np.asarray(rec).astype(RAW), voxel)


def _as_tensor(vol):
    import torch
    return torch.from_numpy(np.ascontiguousarray(vol).view(np.int32).reshape(vol.shape + (2,)).copy()).cuda()


def _from_tensor(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(CELL).reshape(tuple(t.shape[:3]))


def _fuse(m, lo, n, views, trunc=None, before=None, device=False, device_in=False, fill=SENTINEL):
    """revo_map_tsdf_fuse into a host or device volume that holds `before` (an accumulating call) or is filled with `fill`
    -> (cells, info dict, per-view class counts); the info and per-view records start as nines."""
    import torch
    L = _lib.lib()
    if device_in:
        views = [(torch.from_numpy(np.ascontiguousarray(v[0], F)).cuda(),) + tuple(v[1:]) for v in views]
    cv, din, keep = m._carve_views(views)
    nv = len(cv)
    shape = tuple(int(x) for x in n)
    prm = MapTsdfParams(float(mapfile.tsdf_trunc(m.voxel, trunc)), 0 if before is None else 1)
    start = np.full(shape, fill, CELL) if before is None else np.ascontiguousarray(before, CELL).copy()
    box = _box(lo, n)
    if device:
        d, i = _as_tensor(start), torch.full((8,), 9, dtype=torch.int64, device="cuda")
        vi = torch.full((8 * nv,), 9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.revo_map_tsdf_fuse(m._h, C.byref(box), nv, cv, din, C.byref(prm), C.c_void_p(d.data_ptr()), 1, C.c_void_p(i.data_ptr()),
                                        C.c_void_p(vi.data_ptr())))
        m.sync()
        cells, i, vi = _from_tensor(d), i.cpu().numpy().tolist(), vi.cpu().numpy().reshape(nv, 8)
    else:
        cells, info, vinfo = start, MapTsdfInfo(), (MapCarveViewInfo * nv)()
        _lib.check(L.revo_map_tsdf_fuse(m._h, C.byref(box), nv, cv, din, C.byref(prm), cells.ctypes.data_as(C.c_void_p), 0, C.byref(info),
                                        C.cast(vinfo, C.c_void_p)))
        i = [int(getattr(info, k)) for k in mapfile.TSDF_INFO_KEYS] + list(info.reserved)
        vi = np.array([[getattr(v, k) for k in CLASS_FIELDS] + list(v.reserved) for v in vinfo])
    del keep
    assert i[5:] == [0, 0, 0] and not vi[:, 6:].any()
    counts = [dict(zip(mapfile.CARVE_CLASSES, (int(x) for x in row[:6]))) for row in vi]
    return cells, dict(zip(mapfile.TSDF_INFO_KEYS, i[:5])), counts


def _same(got, want, what):
    assert got[0].dtype == CELL and got[0].shape == want[0].shape, what
    assert got[0].tobytes() == want[0].tobytes(), (what, int(np.sum(got[0] != want[0])))
    assert got[1] == want[1] and got[2] == want[2], (what, got[1], want[1])
    assert all(sum(v.values()) == got[1]["cells"] for v in got[2]), what


SIDES = ((False, False), (True, False), (True, True), (False, True))  # (device volume, device images)


# ---------------------------------------------------------------------------------------------------------------- fusion --
@pytest.mark.parametrize("name", list(tc.fuse_cases()))
def test_fuse_cases_bit_exact(name):
    c = tc.fuse_cases()[name]
    want = mapfile.tsdf_records(tc.V, c["lo"], c["n"], c["views"], c["trunc"])
    m = _map()
    before = m.export_raw().tobytes()
    for device, device_in in SIDES:
        _same(_fuse(m, c["lo"], c["n"], c["views"], c["trunc"], device=device, device_in=device_in), want, (name, device, device_in))
    print(name, want[1], want[2][0])
    if name == "9x7x5 trunc M":  # the loop itself, once
        assert want[0].tobytes() == tc.fuse_spec(name)[0].tobytes()
    assert m.export_raw().tobytes() == before
    m.close()


def test_the_exact_properties():
    c = tc.fuse_cases()["9x7x5 default trunc"]
    lo, n, views = c["lo"], c["n"], c["views"]
    want = mapfile.tsdf_records(tc.V, lo, n, views)
    m = _map(sc.records_at([(0, 0, 8), (-4, -3, 6)]))  # a map with voxels in the box: they play no part
    before = m.export_raw().tobytes()
    for device in (False, True):
        kw = dict(device=device)
        # repeated runs and permuted views: the same bytes
        for order in (views, views, views[::-1], views[3:] + views[:3]):
            assert _fuse(m, lo, n, order, **kw)[0].tobytes() == want[0].tobytes()
        back = _fuse(m, lo, n, views[::-1], **kw)
        assert back[1] == want[1] and back[2] == want[2][::-1]
        # A, then B accumulating, is A and B together
        a = _fuse(m, lo, n, views[:3], **kw)
        ab = _fuse(m, lo, n, views[3:], before=a[0], **kw)
        assert ab[0].tobytes() == want[0].tobytes() and a[1]["updates"] + ab[1]["updates"] == want[1]["updates"]
        assert ab[1]["cells_weighted"] == want[1]["cells_weighted"] and ab[1]["cells_inside"] == want[1]["cells_inside"]
        # a call that does not accumulate does not read the volume
        zero, ones = np.zeros(1, CELL)[0], np.array([(-1, 0xFFFFFFFF)], CELL)[0]
        assert _fuse(m, lo, n, views, fill=zero, **kw)[0].tobytes() == _fuse(m, lo, n, views, fill=ones, **kw)[0].tobytes() == want[0].tobytes()
        # saturation: one update under a full weight, two views
        near = tc.nearly_full(n)
        sat = mapfile.tsdf_records(tc.V, lo, n, views[:2], tsdf=near)
        _same(_fuse(m, lo, n, views[:2], before=near, **kw), sat, ("saturation", device))
        assert sat[1]["saturated"] > 0
        # the identity with observe: weight > 0 exactly where the byte is not 0, and the same per-view counts
        seen = m.observe(views, lo=lo, n=n, radius=0, margin=float(mapfile.tsdf_trunc(tc.V)), margin_rel=0.0)
        assert np.array_equal(want[0]["weight"] > 0, seen.seen != 0) and seen.view_info == want[2]
    assert m.export_raw().tobytes() == before
    m.close()


# ------------------------------------------------------------------------------------------------------------------ mesh --
def _mesh(m, cells, lo, min_weight=1, device=False, device_out=False, cap=None, count_only=False):
    """revo_map_tsdf_mesh from a host or device volume into sentinel-filled host or device outputs -> (vertices, triangles, info
    dict), None when the call says REVO_ERR_CAPACITY (and has written nothing); cap: (vertices, triangles) to offer."""
    import torch
    L = _lib.lib()
    cells = np.ascontiguousarray(cells, CELL)
    box = _box(lo, cells.shape)
    t = _as_tensor(cells) if device else None
    vol = C.c_void_p(t.data_ptr()) if device else cells.ctypes.data_as(C.c_void_p)
    nv, nt, info = C.c_size_t(77), C.c_size_t(77), MapMeshInfo()
    torch.cuda.synchronize()
    _lib.check(L.revo_map_tsdf_mesh(m._h, C.byref(box), vol, int(device), min_weight, None, 0, None, 0, C.byref(nv), C.byref(nt), int(device_out),
                                    C.byref(info)))
    idict = {k: int(getattr(info, k)) for k in mapfile.MESH_INFO_KEYS}
    assert info.reserved == 0 and idict["vertices"] == nv.value and idict["triangles"] == nt.value
    if count_only:
        return idict
    cv, ct = (nv.value, nt.value) if cap is None else cap
    if device_out:
        dv = torch.full((max(cv, 1), 3), -7.0, dtype=torch.float32, device="cuda")
        dt = torch.full((max(ct, 1), 3), 0x55, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = L.revo_map_tsdf_mesh(m._h, C.byref(box), vol, int(device), min_weight, C.c_void_p(dv.data_ptr()), cv, C.c_void_p(dt.data_ptr()), ct,
                                  C.byref(nv), C.byref(nt), 1, C.byref(info))
        v, tri = dv.cpu().numpy(), dt.cpu().numpy().view(np.uint32)
    else:
        v, tri = np.full((max(cv, 1), 3), -7.0, F), np.full((max(ct, 1), 3), 0x55, np.uint32)
        rc = L.revo_map_tsdf_mesh(m._h, C.byref(box), vol, int(device), min_weight, v.ctypes.data_as(C.c_void_p), cv, tri.ctypes.data_as(C.c_void_p), ct,
                                  C.byref(nv), C.byref(nt), 0, C.byref(info))
    if rc == CAPACITY:
        assert np.all(v == F(-7.0)) and np.all(tri == 0x55) and (nv.value > cv or nt.value > ct)  # nothing written, and the counts it needs
        return None
    _lib.check(rc)
    assert np.all(v[nv.value:] == F(-7.0)) and np.all(tri[nt.value:] == 0x55)
    return v[:nv.value], tri[:nt.value], {k: int(getattr(info, k)) for k in mapfile.MESH_INFO_KEYS}


MESH_SIDES = ((False, False), (True, False), (True, True), (False, True))  # (device volume, device outputs)


@pytest.mark.parametrize("name", list(tc.mesh_cases()))
def test_mesh_cases_bit_exact(name):
    c = tc.mesh_cases()[name]
    want = mapfile.mesh_records(c["cells"], c["lo"], tc.V, c["min_weight"])
    m = _map()
    before = m.export_raw().tobytes()
    for device, device_out in MESH_SIDES:
        v, t, info = _mesh(m, c["cells"], c["lo"], c["min_weight"], device, device_out)
        assert v.tobytes() == want.vertices.tobytes() and t.tobytes() == want.triangles.tobytes() and info == want.info, (name, device, device_out)
    print(name, want.info)
    assert _mesh(m, c["cells"], c["lo"], c["min_weight"], count_only=True) == want.info
    nv, nt = want.info["vertices"], want.info["triangles"]
    if nt:  # caps one too small: nothing is written
        for device_out in (False, True):
            assert _mesh(m, c["cells"], c["lo"], c["min_weight"], device_out=device_out, cap=(nv - 1, nt)) is None
            assert _mesh(m, c["cells"], c["lo"], c["min_weight"], device_out=device_out, cap=(nv, nt - 1)) is None
            assert len(_mesh(m, c["cells"], c["lo"], c["min_weight"], device_out=device_out, cap=(nv + 2, nt + 3))[1]) == nt
    if name == "sphere":
        assert tc.closed_mesh_numbers(v, t)[3] and v.tobytes() == tc.mesh_spec(name)[0].tobytes()
    assert m.export_raw().tobytes() == before
    m.close()


def test_fuse_then_mesh_on_the_device_and_the_wall():
    import torch
    w = tc.wall()
    lo, n, views = w["lo"], w["n"], w["views"]
    cells = mapfile.tsdf_records(tc.V, lo, n, views)[0]
    want = mapfile.mesh_records(cells, lo, tc.V)
    m = _map()
    d = torch.full(tuple(n) + (2,), 0x2B, dtype=torch.int32, device="cuda")
    dviews = [(torch.from_numpy(views[0][0]).cuda(),) + tuple(views[0][1:])]
    m.fuse_into(d, dviews, lo, wait=False)  # only enqueued; the mesh runs behind it on the same stream
    counts = m.mesh_into(None, None, d, lo)
    assert counts[:2] == (want.info["vertices"], want.info["triangles"]) and counts[2] == want.info
    dv = torch.zeros((counts[0], 3), dtype=torch.float32, device="cuda")
    dt = torch.zeros((counts[1], 3), dtype=torch.int32, device="cuda")
    assert m.mesh_into(dv, dt, d, lo)[:2] == counts[:2]
    assert _from_tensor(d).tobytes() == cells.tobytes()
    assert dv.cpu().numpy().tobytes() == want.vertices.tobytes() and dt.cpu().numpy().view(np.uint32).tobytes() == want.triangles.tobytes()
    # every vertex lies within trunc / 512 of the wall (test_map_tsdf_cpu.py test_the_wall derives the bound)
    err = np.abs(dv.cpu().numpy()[:, 2].astype(np.float64) - float(tc.WALL_DEPTH))
    assert len(err) > 0 and err.max() <= float(mapfile.tsdf_trunc(tc.V)) / 512
    with pytest.raises(_lib.RevoError):
        m.mesh_into(dv[:-1], dt, d, lo)
    with pytest.raises(ValueError):
        m.mesh_into(dv, dt.to(torch.int64), d, lo)
    m.close()


# -------------------------------------------------------------------------------------------------------------- arguments --
def test_argument_errors_write_nothing():
    import torch
    L = _lib.lib()
    m = _map(sc.records_at([(1, 1, 1), (2, 3, 1)]).astype(RAW))
    before = m.export_raw().tobytes()
    lo, n = (-2, -1, 6), (4, 3, 5)  # in front of the plane's camera; a wall between the planes iz = 2 and iz = 3
    good = _box(lo, n)
    t = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    base = t.data_ptr()
    dp = lambda off: C.c_void_p(base + off)  # noqa: E731
    depth = np.full((12, 16), tc.WALL_DEPTH, F)
    cv, _, keep = m._carve_views([(depth, sc.I4, sc.KC)])
    prm = MapTsdfParams(0.25, 0)
    vol = np.full(60, SENTINEL, CELL)
    info, vinfo = np.full(8, 9, np.uint64), np.full(8, 9, np.uint32)
    sp, ip, vp_ = (x.ctypes.data_as(C.c_void_p) for x in (vol, info, vinfo))
    R = 1 << 20
    bad_boxes = [_box((0, 0, 0), (0, 3, 5)), _box((0, 0, 0), (4, -1, 5)), _box((0, 0, 0), (4, 3, 1025)), _box((0, 0, 0), (1024, 1024, 129)),
                 _box((-R - 1, 0, 0), (4, 3, 5)), _box((0, 0, R - 5), (4, 3, 6))]

    def fuse(box=good, nv=1, views=cv, din=0, p=prm, s=sp, dev=0, i=ip, vi=vp_, mm=m):
        return L.revo_map_tsdf_fuse(mm._h if mm is not None else None, C.byref(box) if box is not None else None, nv, views, din,
                                    C.byref(p) if p is not None else None, s, dev, i, vi)

    def view(**kw):
        v, _, k = m._carve_views([(depth, sc.I4, sc.KC)])
        keep.append(k)
        for name, x in kw.items():
            if name == "T":
                v[0].T_w_c[:] = x
            else:
                setattr(v[0], name, x)
        return v

    skew = np.eye(4, dtype=F)
    skew[0, 1] = 0.01
    bad_views = [view(depth=None), view(kf=1 << 12), view(width=0), view(height=2049), view(fx=0.0), view(fy=-1.0), view(cx=float("nan")),
                 view(zmin=-0.5), view(zmin=6.0), view(T=skew.T.reshape(16).tolist()), view(T=[float("nan")] * 16)]
    bad_params = [MapTsdfParams(0.0, 0), MapTsdfParams(-0.1, 0), MapTsdfParams(float("nan"), 0), MapTsdfParams(float("inf"), 0),
                  MapTsdfParams(0.25, 2), MapTsdfParams(0.25, 0, (C.c_uint32 * 2)(1, 0)), MapTsdfParams(0.25, 0, (C.c_uint32 * 2)(0, 9))]
    for j, b in enumerate(bad_boxes):
        assert fuse(b) == INVALID_ARG and L.revo_last_error(), j
    for j, v in enumerate(bad_views):
        assert fuse(views=v) == INVALID_ARG, j
    for j, p in enumerate(bad_params):
        assert fuse(p=p) == INVALID_ARG, j
    assert [fuse(mm=None), fuse(box=None), fuse(views=None), fuse(s=None), fuse(nv=0), fuse(nv=65), fuse(nv=-1), fuse(din=2), fuse(dev=2), fuse(dev=-1),
            fuse(s=dp(8), dev=1, i=None, vi=None), fuse(s=dp(0), dev=1, i=dp(1024 + 8), vi=None), fuse(s=dp(0), dev=1, i=None, vi=dp(2048 + 4)),
            fuse(views=view(depth=base + 4096 + 2), din=1)] == [INVALID_ARG] * 14
    # revo_map_tsdf_mesh
    verts, tris = np.full(3 * 400, -7.0, F), np.full(3 * 800, 0x55, np.uint32)
    vpt, tpt = verts.ctypes.data_as(C.c_void_p), tris.ctypes.data_as(C.c_void_p)
    nv, nt = C.c_size_t(77), C.c_size_t(77)
    minfo = np.full(8, 9, np.uint64)
    mip = minfo.ctypes.data_as(C.c_void_p)

    def mesh(box=good, s=sp, ds=0, v=vpt, tr_=tpt, pv=nv, pt=nt, do=0, i=mip, mm=m):
        return L.revo_map_tsdf_mesh(mm._h if mm is not None else None, C.byref(box) if box is not None else None, s, ds, 1, v, 400, tr_, 800,
                                    C.byref(pv) if pv is not None else None, C.byref(pt) if pt is not None else None, do, i)

    for j, b in enumerate(bad_boxes):
        assert mesh(b) == INVALID_ARG, j
    assert [mesh(mm=None), mesh(box=None), mesh(s=None), mesh(pv=None), mesh(pt=None), mesh(ds=2), mesh(do=-1), mesh(s=dp(8), ds=1),
            mesh(v=dp(4), tr_=dp(4096), do=1), mesh(v=dp(0), tr_=dp(4096 + 8), do=1)] == [INVALID_ARG] * 10
    m.sync()
    assert vol.tobytes() == np.full(60, SENTINEL, CELL).tobytes() and np.all(info == 9) and np.all(vinfo == 9)
    assert np.all(verts == F(-7.0)) and np.all(tris == 0x55) and np.all(minfo == 9) and (nv.value, nt.value) == (77, 77)
    assert not t.cpu().numpy().any() and m.export_raw().tobytes() == before
    # the handle is as usable as before (a fault would make info() fail); info and view_info may be NULL
    assert m.info()["voxels"] == 2
    assert fuse() == 0 and fuse(i=None, vi=None) == 0
    want = mapfile.tsdf_records(tc.V, lo, n, [(depth, sc.I4, sc.KC)], 0.25)
    assert vol.reshape(n).tobytes() == want[0].tobytes() and info.tolist()[:5] == [want[1][x] for x in mapfile.TSDF_INFO_KEYS]
    assert mesh() == 0 and mesh(i=None) == 0
    wm = mapfile.mesh_records(want[0], lo, tc.V)
    assert (nv.value, nt.value) == (len(wm.vertices), len(wm.triangles)) and 0 < nv.value <= 400 and 0 < nt.value <= 800 and minfo.tolist()[:7] == [wm.info[k] for k in mapfile.MESH_INFO_KEYS]
    assert verts[:3 * nv.value].tobytes() == wm.vertices.tobytes() and tris[:3 * nt.value].tobytes() == wm.triangles.tobytes()
    del keep
    m.close()


# ------------------------------------------------------------------------------------------------- the API and the scene --
def test_the_api_the_pyramid_form_and_the_window(tmp_path):
    import torch
    _, cam, pyrs, _ = tr._scene()
    T = tr._kf_poses()
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    m.integrate(pyrs[0], T[0])
    lo, n = (-58, -11, 171), (24, 20, 30)  # around the scene's back wall, where the second view sees less than the first
    plane = pyrs[0].returnDepth(0)
    raw_views = [(plane, T[0], cc.intrinsics320()), (cc.scene_frames()[0][1][1], T[1], cc.intrinsics320())]
    want = mapfile.tsdf_records(cc.VOXEL, lo, n, raw_views)
    # a pyramid against the same plane passed raw (no intrinsics: the context's)
    v = m.fuse([(pyrs[0], T[0]), (raw_views[1][0], T[1])], lo=lo, n=n)
    w = m.fuse([(plane, T[0]), (raw_views[1][0], T[1])], lo=lo, n=n)
    assert v.cells.tobytes() == w.cells.tobytes() == want[0].tobytes() and v.info == w.info == want[1] and v.view_info == want[2]
    assert v.lo.tolist() == list(lo) and v.n.tolist() == list(n) and v.voxel == m.voxel and v.trunc == float(F(4) * F(m.voxel))
    assert want[1]["cells_inside"] > 0 and np.array_equal(v.sdf(), mapfile.tsdf_sdf(want[0], v.trunc), equal_nan=True)
    # into=: a volume accumulates; its box and trunc are the call's, and it is not changed
    a = m.fuse(raw_views[:1], lo=lo, n=n)
    b = m.fuse(raw_views[1:], into=a)
    assert b.cells.tobytes() == want[0].tobytes() and a.cells.tobytes() == mapfile.tsdf_records(cc.VOXEL, lo, n, raw_views[:1])[0].tobytes()
    with pytest.raises(ValueError):
        m.fuse(raw_views, lo=lo, n=n, into=a)
    with pytest.raises(ValueError):
        m.fuse(raw_views, trunc=0.3, into=a)
    # the default box: the map's bounds grown by pad; another trunc
    blo, bhi, _ = m.bounds()
    d = m.fuse([(pyrs[0], T[0])], pad=1, trunc=0.05)
    assert d.lo.tolist() == (blo - 1).tolist() and d.n.tolist() == (bhi - blo + 3).tolist() and d.trunc == float(F(0.05))
    # the mesh, through the volume and through the map; save and load
    mesh = v.mesh(2)
    wm = mapfile.mesh_records(want[0], lo, cc.VOXEL, 2)
    assert mesh.vertices.tobytes() == wm.vertices.tobytes() and mesh.triangles.tobytes() == wm.triangles.tobytes() and mesh.info == wm.info
    assert wm.info["triangles"] > 0 and m.mesh(v).info == mapfile.mesh_records(want[0], lo, cc.VOXEL).info
    back = api.TsdfVolume.load(v.save(str(tmp_path / "v.npz")))
    assert back.mesh(2, map=m).triangles.tobytes() == wm.triangles.tobytes() == back.mesh(2).triangles.tobytes()
    with pytest.raises(ValueError):
        m.mesh(api.TsdfVolume(v.cells, lo, 2 * m.voxel, None))
    assert mapfile.Mesh.load_ply(mesh.save_ply(str(tmp_path / "m.ply"))).vertices.tobytes() == wm.vertices.tobytes()
    # fuse_into: pyramids and device tensors only enqueue
    t = torch.full(tuple(n) + (2,), 0x2B, dtype=torch.int32, device="cuda")
    i = torch.zeros(8, dtype=torch.int64, device="cuda")
    dv = [(pyrs[0], T[0]), (torch.from_numpy(raw_views[1][0]).cuda(), T[1])]
    m.fuse_into(t, dv, lo, d_info=i, wait=False)
    m.sync()
    assert _from_tensor(t).tobytes() == want[0].tobytes() and i.cpu().numpy().tolist()[:5] == [want[1][k] for k in mapfile.TSDF_INFO_KEYS]
    m.fuse_into(t, dv[:1], lo, accumulate=True)
    assert _from_tensor(t).tobytes() == mapfile.tsdf_records(cc.VOXEL, lo, n, raw_views[:1], tsdf=want[0])[0].tobytes()
    with pytest.raises(ValueError):
        m.fuse_into(t.to(torch.int64), dv, lo)
    # MapWindow forwards
    win = api.MapWindow(cam, cc.VOXEL, dense=True, window=2)
    win.integrate(pyrs[0], T[0])
    ws = win.fuse([(pyrs[0], T[0]), (raw_views[1][0], T[1])], lo=lo, n=n)
    assert ws.cells.tobytes() == want[0].tobytes() and win.mesh(ws, 2).triangles.tobytes() == wm.triangles.tobytes()
    assert ws.mesh(2).vertices.tobytes() == wm.vertices.tobytes()
    t2 = torch.zeros(tuple(n) + (2,), dtype=torch.int32, device="cuda")
    win.fuse_into(t2, dv, lo)
    assert win.mesh_into(None, None, t2, lo)[2] == mapfile.mesh_records(want[0], lo, cc.VOXEL).info
    win.close()
    m.close()


@functools.lru_cache(maxsize=None)
def _scene64():
    """The 64^3 box of DESIGN 19's scene, its four views, mapfile's volume and its mesh: computed once."""
    lo, n, views = tc.scene64()
    vol = mapfile.tsdf_records(cc.VOXEL, lo, n, views)
    return lo, n, views, vol, mapfile.mesh_records(vol[0], lo, cc.VOXEL)


def test_the_scene_box():
    lo, n, views, want, wm = _scene64()
    m = _map(cc.scene_records().astype(RAW), cc.VOXEL)
    for device, device_in in ((False, False), (True, True)):
        _same(_fuse(m, lo, n, views, device=device, device_in=device_in), want, ("scene", device))
    print("scene 64^3:", want[1], want[2], wm.info)
    for device, device_out in ((False, False), (True, True)):
        v, t, info = _mesh(m, want[0], lo, 1, device, device_out)
        assert v.tobytes() == wm.vertices.tobytes() and t.tobytes() == wm.triangles.tobytes() and info == wm.info, device
    assert wm.info["triangles"] > 1000 and int(wm.triangles.max()) == len(wm.vertices) - 1
    m.close()
