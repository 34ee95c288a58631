"""Colour and normals on the TSDF surface, on the device (revo_map_tsdf_fuse_color / revo_map_tsdf_mesh_attr, api.VoxelMap.fuse(color=)
/ fuse_into(d_color=) / mesh(normals=, colors=) / mesh_into, api.SurfaceVolume, vo.REVO(surface=), run_tum --surface):
both volumes, all infos and the per-view counts bit for bit revo_amd.mapfile's restatement (which test_map_surface_cpu.py pins to
the per-cell and per-vertex specification) on the shared cases, from host and device images into host and device volumes and in the
pyramid form; the tsdf bytes are revo_map_tsdf_fuse's; the exact properties and the saturation tie; the vertices' attributes bit for
bit from host and device volumes into host and device outputs, vertices and triangles byte for byte revo_map_tsdf_mesh's, caps one
too small; the sign and colour properties without a tolerance; every argument error; the running sequence and the command."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile, synth  # noqa: E402
from revo_amd.settings import MapCarveViewInfo, MapMeshInfo, MapTsdfColorInfo, MapTsdfInfo, MapTsdfParams  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_seen_cases as sc  # noqa: E402
import map_surface_cases as su  # noqa: E402
import map_tsdf_cases as tc  # noqa: E402
import test_gpu_map_tsdf as tt  # noqa: E402

F = np.float32
CELL, COLOR = mapfile.TSDF_CELL_DTYPE, mapfile.TSDF_COLOR_DTYPE
INVALID_ARG, CAPACITY = -1, -5
SENTINEL = np.array([(0x2B2B2B2B, 0x3C3C3C3C, 0x4D4D4D4D, 0xABABABAB)], COLOR)[0]
vp = C.c_void_p


def _col_tensor(col):
    import torch
    return torch.from_numpy(np.ascontiguousarray(col).view(np.int32).reshape(col.shape + (4,)).copy()).cuda()


def _col_from(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(COLOR).reshape(tuple(t.shape[:3]))


def _fuse(m, lo, n, views, bgr, trunc=None, before=None, device=False, device_in=False, fill=(tt.SENTINEL, SENTINEL)):
    """revo_map_tsdf_fuse_color into host or device volumes that hold `before` (a pair: an accumulating call) or are filled with
    `fill` -> (cells, info, per-view counts, colour cells, colour info); every info record starts as nines."""
    import torch
    L = _lib.lib()
    views = [tuple(v[:3]) + (im,) for v, im in zip(views, bgr)]
    if device_in:
        views = [(torch.from_numpy(np.ascontiguousarray(v[0], F)).cuda(), v[1], v[2], torch.from_numpy(np.ascontiguousarray(v[3])).cuda()) for v in views]
    cv, din, keep, ptrs, keep_c = m._color_views(views)
    nv = len(cv)
    shape = tuple(int(x) for x in n)
    prm = MapTsdfParams(float(mapfile.tsdf_trunc(m.voxel, trunc)), 0 if before is None else 1)
    start = np.full(shape, fill[0], CELL) if before is None else np.ascontiguousarray(before[0], CELL).copy()
    cstart = np.full(shape, fill[1], COLOR) if before is None else np.ascontiguousarray(before[1], COLOR).copy()
    box = tt._box(lo, n)
    if device:
        d, dc = tt._as_tensor(start), _col_tensor(cstart)
        i, ci = torch.full((8,), 9, dtype=torch.int64, device="cuda"), torch.full((4,), 9, dtype=torch.int64, device="cuda")
        vi = torch.full((8 * nv,), 9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.revo_map_tsdf_fuse_color(m._h, C.byref(box), nv, cv, C.cast(ptrs, vp), din, C.byref(prm), vp(d.data_ptr()), vp(dc.data_ptr()), 1,
                                              vp(i.data_ptr()), vp(ci.data_ptr()), vp(vi.data_ptr())))
        m.sync()
        cells, col = tt._from_tensor(d), _col_from(dc)
        i, ci, vi = i.cpu().numpy().tolist(), ci.cpu().numpy().tolist(), vi.cpu().numpy().reshape(nv, 8)
    else:
        cells, col, info, cinfo, vinfo = start, cstart, MapTsdfInfo(), MapTsdfColorInfo(), (MapCarveViewInfo * nv)()
        _lib.check(L.revo_map_tsdf_fuse_color(m._h, C.byref(box), nv, cv, C.cast(ptrs, vp), din, C.byref(prm), cells.ctypes.data_as(vp),
                                              col.ctypes.data_as(vp), 0, C.byref(info), C.byref(cinfo), C.cast(vinfo, vp)))
        i = [int(getattr(info, k)) for k in mapfile.TSDF_INFO_KEYS] + list(info.reserved)
        ci = [int(cinfo.color_updates), int(cinfo.cells_colored)] + list(cinfo.reserved)
        vi = np.array([[getattr(v, k) for k in tt.CLASS_FIELDS] + list(v.reserved) for v in vinfo])
    del keep, keep_c
    assert i[5:] == [0, 0, 0] and ci[2:] == [0, 0] and not vi[:, 6:].any()
    counts = [dict(zip(mapfile.CARVE_CLASSES, (int(x) for x in row[:6]))) for row in vi]
    return cells, dict(zip(mapfile.TSDF_INFO_KEYS, i[:5])), counts, col, dict(zip(mapfile.TSDF_COLOR_INFO_KEYS, ci[:2]))


def _same(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), (what, "tsdf", int(np.sum(got[0] != want[0])))
    assert got[3].dtype == COLOR and got[3].tobytes() == want[3].tobytes(), (what, "colour", int(np.sum(got[3] != want[3])))
    assert got[1] == want[1] and got[2] == want[2] and got[4] == want[4], (what, got[1], want[1], got[4], want[4])


# ---------------------------------------------------------------------------------------------------------------- fusion --
@pytest.mark.parametrize("name", su.FUSE_NAMES)
def test_fuse_color_cases_bit_exact(name):
    c = su.fuse_cases()[name]
    want = mapfile.tsdf_records(tc.V, c["lo"], c["n"], c["views"], c["trunc"], bgr=c["bgr"])
    m = tt._map()
    before = m.export_raw().tobytes()
    for device, device_in in tt.SIDES:
        _same(_fuse(m, c["lo"], c["n"], c["views"], c["bgr"], c["trunc"], device=device, device_in=device_in), want, (name, device, device_in))
    print(name, want[1], want[4])
    # the tsdf bytes, info and view_info are revo_map_tsdf_fuse's on the same arguments
    plain = tt._fuse(m, c["lo"], c["n"], c["views"], c["trunc"], device=True)
    assert plain[0].tobytes() == want[0].tobytes() and plain[1] == want[1] and plain[2] == want[2]
    if name == "3x5x7 trunc M":  # the loop itself, once
        assert want[3].tobytes() == su.fuse_spec(name)[3].tobytes()
    assert m.export_raw().tobytes() == before
    m.close()


def test_the_exact_properties_and_the_saturation_tie():
    c = su.fuse_cases()["64 views"]
    lo, n, views, bgr = c["lo"], c["n"], c["views"][:8], c["bgr"][:8]
    want = mapfile.tsdf_records(tc.V, lo, n, views, bgr=bgr)
    m = tt._map(sc.records_at([(0, 0, 8), (-4, -3, 6)]))  # a map with voxels in the box: they play no part
    before = m.export_raw().tobytes()
    for device in (False, True):
        kw = dict(device=device)
        for order in (list(range(8)), list(range(8))[::-1], [3, 4, 5, 6, 7, 0, 1, 2]):
            got = _fuse(m, lo, n, [views[i] for i in order], [bgr[i] for i in order], **kw)
            assert got[0].tobytes() == want[0].tobytes() and got[3].tobytes() == want[3].tobytes() and got[4] == want[4]
        a = _fuse(m, lo, n, views[:3], bgr[:3], **kw)
        ab = _fuse(m, lo, n, views[3:], bgr[3:], before=(a[0], a[3]), **kw)
        assert ab[0].tobytes() == want[0].tobytes() and ab[3].tobytes() == want[3].tobytes()
        assert a[4]["color_updates"] + ab[4]["color_updates"] == want[4]["color_updates"] and ab[4]["cells_colored"] == want[4]["cells_colored"]
        # a call that does not accumulate reads neither volume
        zeros = (np.zeros(1, CELL)[0], np.zeros(1, COLOR)[0])
        ones = (np.array([(-1, 0xFFFFFFFF)], CELL)[0], np.array([(0xFFFFFFFF,) * 4], COLOR)[0])
        for fill in (zeros, ones):
            got = _fuse(m, lo, n, views, bgr, fill=fill, **kw)
            assert got[0].tobytes() == want[0].tobytes() and got[3].tobytes() == want[3].tobytes()
        # TSDF weight 2^20 - 1 under two CONFIRMED views: the second colour update is dropped with the TSDF update
        w = tc.wall()
        vol, col = su.nearly_full(w["n"])
        img = [su.wall_image((1, 2, 3)), su.wall_image((200, 100, 50))]
        sat = mapfile.tsdf_records(tc.V, w["lo"], w["n"], w["views"] * 2, bgr=img, tsdf=vol, color=col)
        _same(_fuse(m, w["lo"], w["n"], w["views"] * 2, img, before=(vol, col), **kw), sat, ("saturation", device))
        assert sat[1]["saturated"] == sat[4]["color_updates"] == vol.size and np.all(sat[3]["weight"] == 6) and np.all(sat[3]["sum_b"] == 101)
    assert np.all(want[3]["weight"][want[0]["sum"] < 0] > 0) and want[4]["color_updates"] > 0
    assert m.export_raw().tobytes() == before
    m.close()


# -------------------------------------------------------------------------------------------------------- the attributes --
def _mesh(m, cells, color, lo, min_weight=1, device=False, device_out=False, cap=None, normals=True, colors=True):
    """revo_map_tsdf_mesh_attr from host or device volumes into sentinel-filled host or device outputs -> (vertices, triangles,
    info, normals, colours), None when the call says REVO_ERR_CAPACITY (and has written nothing); cap: (vertices, triangles)."""
    import torch
    L = _lib.lib()
    cells = np.ascontiguousarray(cells, CELL)
    box = tt._box(lo, cells.shape)
    t, tc_ = (tt._as_tensor(cells), _col_tensor(color)) if device else (None, None)
    vol = vp(t.data_ptr()) if device else cells.ctypes.data_as(vp)
    color = np.ascontiguousarray(color, COLOR)
    cvol = vp(tc_.data_ptr()) if device else color.ctypes.data_as(vp)
    nv, nt, info = C.c_size_t(77), C.c_size_t(77), MapMeshInfo()
    torch.cuda.synchronize()
    head = (m._h, C.byref(box), vol, cvol, int(device), min_weight)
    _lib.check(L.revo_map_tsdf_mesh_attr(*head, None, None, None, 0, None, 0, C.byref(nv), C.byref(nt), int(device_out), C.byref(info)))
    assert info.vertices == nv.value and info.triangles == nt.value
    cv, ct = (nv.value, nt.value) if cap is None else cap
    if device_out:
        dv = torch.full((max(cv, 1), 3), -7.0, dtype=torch.float32, device="cuda")
        dn = torch.full((max(cv, 1), 3), -7.0, dtype=torch.float32, device="cuda")
        dc = torch.full((max(cv, 1), 4), 0x66, dtype=torch.uint8, device="cuda")
        dt = torch.full((max(ct, 1), 3), 0x55, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = L.revo_map_tsdf_mesh_attr(*head, vp(dv.data_ptr()), vp(dn.data_ptr()) if normals else None, vp(dc.data_ptr()) if colors else None, cv,
                                       vp(dt.data_ptr()), ct, C.byref(nv), C.byref(nt), 1, C.byref(info))
        m.sync()
        v, nrm, rgb, tri = dv.cpu().numpy(), dn.cpu().numpy(), dc.cpu().numpy(), dt.cpu().numpy().view(np.uint32)
    else:
        v, nrm, rgb = np.full((max(cv, 1), 3), -7.0, F), np.full((max(cv, 1), 3), -7.0, F), np.full((max(cv, 1), 4), 0x66, np.uint8)
        tri = np.full((max(ct, 1), 3), 0x55, np.uint32)
        rc = L.revo_map_tsdf_mesh_attr(*head, v.ctypes.data_as(vp), nrm.ctypes.data_as(vp) if normals else None, rgb.ctypes.data_as(vp) if colors else None,
                                       cv, tri.ctypes.data_as(vp), ct, C.byref(nv), C.byref(nt), 0, C.byref(info))
    if rc == CAPACITY:
        assert np.all(v == F(-7.0)) and np.all(nrm == F(-7.0)) and np.all(rgb == 0x66) and np.all(tri == 0x55) and (nv.value > cv or nt.value > ct)
        return None
    _lib.check(rc)
    k = nv.value
    assert np.all(v[k:] == F(-7.0)) and np.all(nrm[k if normals else 0:] == F(-7.0)) and np.all(rgb[k if colors else 0:] == 0x66) and np.all(tri[nt.value:] == 0x55)
    return v[:k], tri[:nt.value], {x: int(getattr(info, x)) for x in mapfile.MESH_INFO_KEYS}, nrm[:k], rgb[:k]


@pytest.mark.parametrize("name", list(su.mesh_cases()))
def test_mesh_attr_cases_bit_exact(name):
    c = su.mesh_cases()[name]
    want = mapfile.mesh_attr_records(c["cells"], c["color"], c["lo"], tc.V, c["min_weight"])
    m = tt._map()
    before = m.export_raw().tobytes()
    plain = tt._mesh(m, c["cells"], c["lo"], c["min_weight"], True, True)  # revo_map_tsdf_mesh itself
    assert plain[0].tobytes() == want.vertices.tobytes() and plain[1].tobytes() == want.triangles.tobytes()
    for device, device_out in tt.MESH_SIDES:
        v, t, info, nrm, rgb = _mesh(m, c["cells"], c["color"], c["lo"], c["min_weight"], device, device_out)
        assert v.tobytes() == plain[0].tobytes() and t.tobytes() == plain[1].tobytes() and info == want.info == plain[2], (name, device, device_out)
        assert nrm.tobytes() == want.normals.tobytes(), (name, device, device_out, int(np.sum(nrm.view(np.uint32) != want.normals.view(np.uint32))))
        assert rgb.tobytes() == want.colors.tobytes(), (name, device, device_out, int(np.sum(rgb != want.colors)))
    print(name, want.info, np.bincount(want.colors[:, 3], minlength=3).tolist() if len(want.colors) else [])
    nv, nt = want.info["vertices"], want.info["triangles"]
    if nt:
        for device_out in (False, True):  # caps one too small: nothing is written; one attribute alone
            assert _mesh(m, c["cells"], c["color"], c["lo"], c["min_weight"], device_out=device_out, cap=(nv - 1, nt)) is None
            assert _mesh(m, c["cells"], c["color"], c["lo"], c["min_weight"], device_out=device_out, cap=(nv, nt - 1)) is None
            got = _mesh(m, c["cells"], c["color"], c["lo"], c["min_weight"], device=device_out, device_out=device_out, cap=(nv + 2, nt + 3), colors=False)
            assert got[3].tobytes() == want.normals.tobytes()
            got = _mesh(m, c["cells"], c["color"], c["lo"], c["min_weight"], device=device_out, device_out=device_out, normals=False)
            assert got[4].tobytes() == want.colors.tobytes() and got[0].tobytes() == want.vertices.tobytes()
    if name == "256 patterns":
        assert set(np.unique(want.colors[:, 3]).tolist()) == {0, 1, 2} and want.normals.tobytes() == su.mesh_spec(name)[3].tobytes()
    assert m.export_raw().tobytes() == before
    m.close()


def test_signs_and_colours_without_a_tolerance():
    m = tt._map()
    # the sphere: every vertex normal has a positive dot product with the summed face normals of its triangles
    c = su.mesh_cases()["sphere"]
    v, t, _, nrm, _ = _mesh(m, c["cells"], c["color"], c["lo"], 1, True, True)
    p, ti = v.astype(np.float64), t.astype(np.int64)
    fn = np.cross(p[ti[:, 1]] - p[ti[:, 0]], p[ti[:, 2]] - p[ti[:, 0]])
    face = np.zeros((len(v), 3))
    for k in range(3):
        np.add.at(face, ti[:, k], fn)
    assert len(v) > 100 and np.all(np.einsum("ij,ij->i", face, nrm.astype(np.float64)) > 0)
    # the wall under one view with a constant-colour image: every vertex has exactly that colour
    w = tc.wall()
    colour = (17, 130, 251)
    vol = m.fuse([tuple(w["views"][0]) + (su.wall_image(colour),)], lo=w["lo"], n=w["n"], color=True)
    mesh = vol.mesh(normals=True, colors=True)
    assert len(mesh.vertices) and np.all(mesh.colors[:, :3] == np.array(colour, np.uint8)) and np.all(mesh.colors[:, 3] >= 1)
    assert np.all(mesh.normals[:, 2] < 0)  # the field grows towards the camera, which looks down +z
    # fused through fuse(color=True) only: no vertex has k = 0
    for name in ("64 views", "two views", "3x5x7 default trunc"):
        c = su.fuse_cases()[name]
        vol = m.fuse([tuple(v_) + (im,) for v_, im in zip(c["views"], c["bgr"])], lo=c["lo"], n=c["n"], trunc=c["trunc"], color=True)
        want = mapfile.tsdf_records(tc.V, c["lo"], c["n"], c["views"], c["trunc"], bgr=c["bgr"])
        assert vol.cells.tobytes() == want[0].tobytes() and vol.color.tobytes() == want[3].tobytes() and vol.color_info == want[4] and vol.info == want[1]
        mesh = vol.mesh(colors=True)
        assert mesh.normals is None and (not len(mesh.colors) or int(mesh.colors[:, 3].min()) >= 1)
        assert mesh.colors.tobytes() == mapfile.mesh_attr_records(want[0], want[3], c["lo"], tc.V).colors.tobytes()
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
    prm = MapTsdfParams(0.25, 0)
    vol, col = np.full(60, tt.SENTINEL, CELL), np.full(60, SENTINEL, COLOR)
    info, cinfo, vinfo = np.full(8, 9, np.uint64), np.full(4, 9, np.uint64), np.full(8, 9, np.uint32)
    sp, cp, ip, cip, vip = (x.ctypes.data_as(vp) for x in (vol, col, info, cinfo, vinfo))

    def fuse(box=good, nv=1, views=cv, bgr=one, din=0, p=prm, s=sp, c=cp, dev=0, i=ip, ci=cip, vi=vip, mm=m):
        return L.revo_map_tsdf_fuse_color(mm._h if mm is not None else None, C.byref(box) if box is not None else None, nv, views,
                                          C.cast(bgr, vp) if bgr is not None else None, din, C.byref(p) if p is not None else None, s, c, dev, i, ci, vi)

    pyr_like, _, k2 = m._carve_views([(depth, sc.I4, sc.KC)])
    pyr_like[0].depth, pyr_like[0].kf = None, 1 << 12  # a pyramid view (never followed: the bgr rule comes first)
    assert [fuse(mm=None), fuse(box=None), fuse(views=None), fuse(bgr=None), fuse(s=None), fuse(c=None), fuse(bgr=none), fuse(views=pyr_like, bgr=one),
            fuse(nv=0), fuse(nv=65), fuse(din=2), fuse(dev=2), fuse(box=tt._box((0, 0, 0), (0, 3, 5))), fuse(p=MapTsdfParams(0.0, 0)),
            fuse(p=MapTsdfParams(0.25, 2)), fuse(s=dp(0), c=dp(2048 + 8), dev=1, i=None, ci=None, vi=None),
            fuse(s=dp(0), c=dp(2048), dev=1, i=None, ci=dp(4096 + 8), vi=None), fuse(s=dp(8), c=dp(2048), dev=1, i=None, ci=None, vi=None)] == [INVALID_ARG] * 18
    assert L.revo_last_error()
    # revo_map_tsdf_mesh_attr
    verts, nrm, rgb, tris = np.full(3 * 400, -7.0, F), np.full(3 * 400, -7.0, F), np.full(4 * 400, 0x66, np.uint8), np.full(3 * 800, 0x55, np.uint32)
    vpt, npt, cpt, tpt = (x.ctypes.data_as(vp) for x in (verts, nrm, rgb, tris))
    nv, nt = C.c_size_t(77), C.c_size_t(77)
    minfo = np.full(8, 9, np.uint64)

    def mesh(box=good, s=sp, c=cp, ds=0, v=vpt, nr=npt, cl=cpt, tr_=tpt, pv=nv, pt=nt, do=0, mm=m):
        return L.revo_map_tsdf_mesh_attr(mm._h if mm is not None else None, C.byref(box) if box is not None else None, s, c, ds, 1, v, nr, cl, 400, tr_, 800,
                                         C.byref(pv) if pv is not None else None, C.byref(pt) if pt is not None else None, do, minfo.ctypes.data_as(vp))

    assert [mesh(mm=None), mesh(box=None), mesh(s=None), mesh(c=None), mesh(pv=None), mesh(pt=None), mesh(ds=2), mesh(do=-1),
            mesh(box=tt._box((0, 0, 0), (4, -1, 5))), mesh(s=dp(0), c=dp(2048 + 8), ds=1), mesh(s=dp(8), c=dp(2048), ds=1),
            mesh(v=dp(0), nr=dp(1024 + 4), cl=dp(2048), tr_=dp(4096), do=1), mesh(v=dp(0), nr=dp(1024), cl=dp(2048 + 4), tr_=dp(4096), do=1)] == [INVALID_ARG] * 13
    m.sync()
    assert vol.tobytes() == np.full(60, tt.SENTINEL, CELL).tobytes() and col.tobytes() == np.full(60, SENTINEL, COLOR).tobytes()
    assert np.all(info == 9) and np.all(cinfo == 9) and np.all(vinfo == 9) and np.all(minfo == 9) and (nv.value, nt.value) == (77, 77)
    assert np.all(verts == F(-7.0)) and np.all(nrm == F(-7.0)) and np.all(rgb == 0x66) and np.all(tris == 0x55) and not t.cpu().numpy().any()
    # the handle is as usable as before; the infos may be NULL; normals without a colour volume are fine
    assert fuse() == 0 and fuse(i=None, ci=None, vi=None) == 0
    want = mapfile.tsdf_records(tc.V, lo, n, [(depth, sc.I4, sc.KC)], 0.25, bgr=[img])
    assert vol.reshape(n).tobytes() == want[0].tobytes() and col.reshape(n).tobytes() == want[3].tobytes()
    assert cinfo.tolist() == [want[4]["color_updates"], want[4]["cells_colored"], 0, 0]
    assert mesh() == 0 and mesh(c=None, cl=None) == 0
    wm = mapfile.mesh_attr_records(want[0], want[3], lo, tc.V)
    k = nv.value
    assert 0 < k == len(wm.vertices) <= 400 and nrm[:3 * k].tobytes() == wm.normals.tobytes() and rgb[:4 * k].tobytes() == wm.colors.tobytes()
    # the Python layer's own refusals
    plain = m.fuse([(depth, sc.I4, sc.KC)], lo=lo, n=n)
    full = m.fuse([(depth, sc.I4, sc.KC, img)], lo=lo, n=n, color=True)
    for bad in (lambda: m.fuse([(depth, sc.I4, sc.KC, img)], into=plain, color=True), lambda: m.fuse([(depth, sc.I4, sc.KC)], into=full),
                lambda: m.fuse([(depth, sc.I4, sc.KC)], lo=lo, n=n, color=True), lambda: m.fuse([(depth, sc.I4, sc.KC, img[:, :-1])], lo=lo, n=n, color=True),
                lambda: plain.mesh(colors=True), lambda: m.mesh(plain, colors=True)):
        with pytest.raises(ValueError):
            bad()
    assert plain.color is None and plain.cells.tobytes() == full.cells.tobytes()
    both = m.fuse([(depth, sc.I4, sc.KC, img)], into=full, color=True)
    assert both.color.tobytes() == mapfile.tsdf_records(tc.V, lo, n, [(depth, sc.I4, sc.KC)], bgr=[img], tsdf=full.cells, color=full.color)[3].tobytes()
    del keep, k2
    m.close()


# ----------------------------------------------------------------------------------------------- the API and the sequence --
def test_the_pyramid_form_and_the_device_tensors():
    import torch
    _, cam, pyrs, _ = tt.tr._scene()
    T = tt.tr._kf_poses()
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    lo, n = (-58, -11, 171), (24, 20, 30)
    frames = cc.scene_frames()
    plane = pyrs[0].returnDepth(0)
    bgr0 = np.ascontiguousarray(frames[0][0][0])  # the first view's colour image, as its pyramid was built from it
    rng = np.random.default_rng(5)
    bgr1 = rng.integers(0, 256, plane.shape + (3,), dtype=np.uint8)
    raw = [(plane, T[0], cc.intrinsics320()), (frames[0][1][1], T[1], cc.intrinsics320())]
    want = mapfile.tsdf_records(cc.VOXEL, lo, n, raw, bgr=[bgr0, bgr1])
    v = m.fuse([(pyrs[0], T[0]), (raw[1][0], T[1], None, bgr1)], lo=lo, n=n, color=True)  # a pyramid brings its colour plane
    assert v.cells.tobytes() == want[0].tobytes() and v.color.tobytes() == want[3].tobytes() and v.color_info == want[4] and want[4]["cells_colored"] > 0
    # fuse_into / mesh_into: only enqueued, everything on the device
    t = torch.full(tuple(n) + (2,), 0x2B, dtype=torch.int32, device="cuda")
    tcol = torch.full(tuple(n) + (4,), 0x2B, dtype=torch.int32, device="cuda")
    ci = torch.zeros(4, dtype=torch.int64, device="cuda")
    dv = [(pyrs[0], T[0]), (torch.from_numpy(raw[1][0]).cuda(), T[1], None, torch.from_numpy(bgr1).cuda())]
    m.fuse_into(t, dv, lo, wait=False, d_color=tcol, d_color_info=ci)
    nv, nt, info = m.mesh_into(None, None, t, lo)
    wm = mapfile.mesh_attr_records(want[0], want[3], lo, cc.VOXEL)
    assert (nv, nt) == (len(wm.vertices), len(wm.triangles)) and nt > 0
    d_v, d_n = (torch.zeros((nv, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    d_t, d_c = torch.zeros((nt, 3), dtype=torch.int32, device="cuda"), torch.zeros((nv, 4), dtype=torch.uint8, device="cuda")
    assert m.mesh_into(d_v, d_t, t, lo, d_normals=d_n, d_colors=d_c, d_color=tcol)[:2] == (nv, nt)
    assert _col_from(tcol).tobytes() == want[3].tobytes() and ci.cpu().numpy().tolist()[:2] == [want[4][k] for k in mapfile.TSDF_COLOR_INFO_KEYS]
    assert d_v.cpu().numpy().tobytes() == wm.vertices.tobytes() and d_n.cpu().numpy().tobytes() == wm.normals.tobytes()
    assert d_c.cpu().numpy().tobytes() == wm.colors.tobytes()
    with pytest.raises(ValueError):
        m.mesh_into(d_v, d_t, t, lo, d_colors=d_c)
    with pytest.raises(ValueError):
        m.fuse_into(t, dv, lo, d_color=tcol[..., :2].contiguous())
    # MapWindow forwards the new arguments
    win = api.MapWindow(cam, cc.VOXEL, dense=True, window=2)
    ws = win.fuse([(pyrs[0], T[0]), (raw[1][0], T[1], None, bgr1)], lo=lo, n=n, color=True)
    assert ws.color.tobytes() == want[3].tobytes() and win.mesh(ws, 1, True, True).colors.tobytes() == wm.colors.tobytes()
    win.close()
    m.close()


def _two_keyframes(s, seed=41):
    """A short synthetic sequence with a steady pan: the frames, up to the one that gives the second keyframe."""
    from test_gpu_voxel_map import BIASES
    return synth.make_sequence(seed, s, 40, max_t=0.01, max_rot_deg=0.4, bias=BIASES[1])


def test_the_running_sequence_is_one_fuse_call():
    from lm_settings_cases import S160
    from revo_amd import vo
    frames = _two_keyframes(S160)
    cam = api.CameraPyr(S160)
    vm = api.VoxelMap(cam, 0.05, dense=True)
    lo, n = (-40, -40, 0), (80, 80, 100)
    surf = api.SurfaceVolume(vm, lo, n)
    g = vo.REVO(S160, cameraPyr=cam, voxelMap=vm, surface=surf)
    by_ts = {float(f[2]): f[0] for f in frames}
    views = []
    for f in frames:
        _, kf = g.push(f[0], f[1], f[2])
        if kf:
            pyr, T = g.keyframe()
            views.append((pyr.returnDepth(0).copy(), np.array(T, F), None, np.ascontiguousarray(by_ts[float(pyr.returnTimestamp())])))
        if len(views) == 2:
            break
    assert len(views) == 2 == surf.views and g.surface_skipped == 0, "the sequence gives two keyframes"
    got = surf.volume()
    want = vm.fuse(views, lo=lo, n=n, color=True)
    assert got.cells.tobytes() == want.cells.tobytes() and got.color.tobytes() == want.color.tobytes() and got.trunc == want.trunc
    assert want.color_info["cells_colored"] > 0 and [c["confirmed"] for c in surf.view_counts()] == [c["confirmed"] for c in want.view_info]
    mesh = surf.mesh()
    wm = mapfile.mesh_attr_records(want.cells, want.color, lo, vm.voxel)
    assert len(wm.triangles) > 0 and mesh.vertices.tobytes() == wm.vertices.tobytes() and mesh.triangles.tobytes() == wm.triangles.tobytes()
    assert mesh.normals.tobytes() == wm.normals.tobytes() and mesh.colors.tobytes() == wm.colors.tobytes() and int(mesh.colors[:, 3].min()) >= 1
    # off by default, and refused where it cannot work
    with pytest.raises(ValueError):
        vo.REVO(S160, cameraPyr=cam, surface=surf)
    with pytest.raises(ValueError):
        vo.REVO(S160, cameraPyr=cam, voxelMap=api.VoxelMap(cam, 0.05), surface=surf)
    with pytest.raises(ValueError):
        api.SurfaceVolume(vm, lo, n, color=False).mesh()
    vm.close()


def test_run_tum_surface(tmp_path, monkeypatch, capsys):
    from lm_settings_cases import S160
    from revo_amd import run_tum, tum
    from test_gpu_vo_multi import _tum_yaml
    name = "rgbd_synth_s"
    tum.write_synthetic_dataset(str(tmp_path / "data" / name), _two_keyframes(S160)[:12])
    _tum_yaml(tmp_path, S160, [name])
    monkeypatch.chdir(tmp_path)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "0", "--map", "0.05"]
    assert run_tum.main(args + ["--surface", "surface.ply", "--surface-box", "-40", "-40", "0", "80", "80", "100", "--surface-trunc", "0.2"]) == 0
    mesh = mapfile.Mesh.load_ply(str(tmp_path / "surface.ply"))
    assert len(mesh.triangles) > 0 and mesh.normals is not None and mesh.colors is not None and len(mesh.normals) == len(mesh.colors) == len(mesh.vertices)
    ln = np.linalg.norm(mesh.normals.astype(np.float64), axis=1)
    assert np.all(np.abs(ln - 1) < 1e-6)  # unit vectors in float32: six operations of 2^-24 each
    assert "Surface:" in capsys.readouterr().out
    # usage errors
    assert run_tum.main(args[:4] + ["--surface", "s.ply"]) == 2 and run_tum.main(args + ["--surface-trunc", "0.2"]) == 2
    assert run_tum.main(args + ["--surface", "s.ply", "--map-window", "2"]) == 2 and run_tum.main(args + ["--surface", "s.ply", "--streams", "2"]) == 2
    assert run_tum.main(args + ["--surface", "s.ply", "--surface-box", "0", "0", "0", "0", "4", "4"]) == 2
    capsys.readouterr()
