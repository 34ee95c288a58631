"""A box that follows the camera, on the device (revo_map_tsdf_shift / revo_map_tsdf_refill, api.VoxelMap.shift_into / refill_into /
surface_shift / surface_refill, api.SurfaceVolume.shift / refill, api.FollowingSurface, vo.REVO(surface=FollowingSurface),
run_tum --surface-follow): both destination volumes, the records and every info bit for bit revo_amd.mapfile's restatement
(which test_map_follow_cpu.py pins to the per-cell loops) on the shared cases, from host and device volumes into host and device
records, in the counting, the emitting and the dropping mode; caps one too small; the exact properties (a) and (b); every argument
error and every refill refusal with nothing written; the map untouched; a following surface against the sequence rule."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile  # noqa: E402
from revo_amd.settings import MapTsdfRefillInfo  # noqa: E402

import map_follow_cases as fc  # noqa: E402
import map_follow_ref as fr  # noqa: E402
import map_seen_cases as sc  # noqa: E402
import test_gpu_map_surface as ts  # noqa: E402
import test_gpu_map_tsdf as tt  # noqa: E402

F = np.float32
CELL, COLOR, RECORD = mapfile.TSDF_CELL_DTYPE, mapfile.TSDF_COLOR_DTYPE, mapfile.TSDF_RECORD_DTYPE
INVALID_ARG, CAPACITY = -1, -5
SENT_T, SENT_C = tt.SENTINEL, ts.SENTINEL
SENT_R = np.array([(0x1111111111111111, 0x22222222, 0x33333333, 0x44444444, 0x55555555, 0x66666666, 0x77777777)], RECORD)[0]
vp = C.c_void_p


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and a.tobytes() == b.tobytes())


def _rec_tensor(rec):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).copy()).cuda()


def _rec_from(t, n):
    return np.ascontiguousarray(t.cpu().numpy()).view(RECORD)[:n]


def _shift(m, cells, color, lo, delta, mode, device, device_out=False, cap=None):
    """One raw revo_map_tsdf_shift call.  mode: "emit", "count" or "drop"; the destination volumes start as sentinels, the records as
    sentinels (cap of them; default: as many as there are, at least one), the info as nines.
    -> (rc, dst, dst colour, records [cap], n or None, info list of 8)."""
    import torch
    L = _lib.lib()
    want = mapfile.tsdf_shift_records(cells, color, lo, delta)
    cap = max(len(want[2]), 1) if cap is None else cap
    box = tt._box(lo, cells.shape)
    dl = (C.c_int32 * 3)(*[int(x) for x in delta])
    dst, cdst = np.full(cells.shape, SENT_T, CELL), (None if color is None else np.full(cells.shape, SENT_C, COLOR))
    rec = np.full(max(cap, 1), SENT_R, RECORD)
    n = C.c_size_t(77)
    info = np.full(8, 9, np.uint64)
    pn = None if mode == "drop" else C.byref(n)
    keep = []
    if device:
        ds, dd = tt._as_tensor(cells), tt._as_tensor(dst)
        dcs, dcd = (None, None) if color is None else (ts._col_tensor(color), ts._col_tensor(cdst))
        keep += [ds, dd, dcs, dcd]
        vols = [vp(ds.data_ptr()), None if color is None else vp(dcs.data_ptr()), vp(dd.data_ptr()), None if color is None else vp(dcd.data_ptr())]
    else:
        src, csrc = np.ascontiguousarray(cells), (None if color is None else np.ascontiguousarray(color))
        keep += [src, csrc]
        vols = [src.ctypes.data_as(vp), None if color is None else csrc.ctypes.data_as(vp), dst.ctypes.data_as(vp),
                None if color is None else cdst.ctypes.data_as(vp)]
    d_rec = _rec_tensor(rec) if device_out else None
    rp = None if mode != "emit" else (vp(d_rec.data_ptr()) if device_out else rec.ctypes.data_as(vp))
    d_info = None
    if mode == "drop" and device:  # the one case that only enqueues: info lives on the device
        d_info = torch.full((8,), 9, dtype=torch.int64, device="cuda")
        ip = vp(d_info.data_ptr())
    else:
        ip = info.ctypes.data_as(vp)
    torch.cuda.synchronize()
    rc = L.revo_map_tsdf_shift(m._h, C.byref(box), dl, vols[0], vols[1], vols[2], vols[3], 1 if device else 0, rp, cap if mode == "emit" else 0, pn,
                               1 if device_out else 0, ip)
    m.sync()
    if device:
        dst, cdst = tt._from_tensor(dd), (None if color is None else ts._col_from(dcd))
    if device_out:
        rec = _rec_from(d_rec, len(rec))
    if d_info is not None:
        info = d_info.cpu().numpy().view(np.uint64)
    del keep
    return rc, dst, cdst, rec, (None if mode == "drop" else n.value), [int(x) for x in info]


def _info_list(info, dropped=0):
    return [info["cells"], info["staying"], info["leaving"], info["records"], dropped, 0, 0, 0]


def _check_all_modes(m, c, device, device_out):
    cells, color, lo, delta = c["cells"], c["color"], c["lo"], c["delta"]
    want = mapfile.tsdf_shift_records(cells, color, lo, delta)
    nrec = len(want[2])
    sent_t, sent_c = np.full(cells.shape, SENT_T, CELL), (None if color is None else np.full(cells.shape, SENT_C, COLOR))
    # move and emit
    rc, dst, cdst, rec, n, info = _shift(m, cells, color, lo, delta, "emit", device, device_out)
    assert rc == 0 and same(dst, want[0]) and same(cdst, want[1]) and n == nrec and same(rec[:nrec], want[2]) and info == _info_list(want[3])
    assert np.all(rec[nrec:] == SENT_R), "nothing is written behind the last record"
    # count only: a sentinel-filled destination stays as it is
    rc, dst, cdst, rec, n, info = _shift(m, cells, color, lo, delta, "count", device, device_out)
    assert rc == 0 and same(dst, sent_t) and same(cdst, sent_c) and n == nrec and info == _info_list(want[3]) and np.all(rec == SENT_R)
    # a cap one too small
    if nrec:
        rc, dst, cdst, rec, n, info = _shift(m, cells, color, lo, delta, "emit", device, device_out, cap=nrec - 1)
        assert rc == CAPACITY and same(dst, sent_t) and same(cdst, sent_c) and np.all(rec == SENT_R) and n == nrec and info == _info_list(want[3])
    # move and drop
    rc, dst, cdst, rec, n, info = _shift(m, cells, color, lo, delta, "drop", device, device_out)
    assert rc == 0 and same(dst, want[0]) and same(cdst, want[1]) and n is None and info == _info_list(want[3], dropped=nrec) and np.all(rec == SENT_R)
    return want


@pytest.mark.parametrize("name", list(fc.shift_cases()))
def test_shift_cases_bit_exact(name):
    import torch
    c = fc.shift_cases()[name]
    m = tt._map(sc.records_at([(1, 1, 1), (2, 3, 1)]).astype(tt.RAW))
    before = m.export_raw().tobytes()
    for device, device_out in ((False, False), (True, True), (False, True), (True, False)):
        want = _check_all_modes(m, c, device, device_out)
    print(name, want[3])
    # the api's forms
    got = m.surface_shift(c["cells"], c["lo"], c["delta"], c["color"])
    assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2], want[2]) and got[3] == want[3]
    got = m.surface_shift(c["cells"], c["lo"], c["delta"], c["color"], records=False)
    assert same(got[0], want[0]) and same(got[1], want[1]) and got[2] is None and got[3] == dict(want[3], dropped=want[3]["records"])
    # the refill of the records into the emptied source box, on the host and on the device, is mapfile's
    zero, czero = np.zeros_like(c["cells"]), (None if c["color"] is None else np.zeros_like(c["color"]))
    ref = mapfile.tsdf_refill_records(zero, czero, c["lo"], want[2])
    got = m.surface_refill(zero, c["lo"], want[2], czero)
    assert same(got[0], ref[0]) and same(got[1], ref[1]) and got[2] == ref[2]
    d_t, d_c = tt._as_tensor(zero), (None if czero is None else ts._col_tensor(czero))
    d_r = _rec_tensor(want[2]) if len(want[2]) else None
    assert m.refill_into(d_t, c["lo"], d_r, d_color=d_c) == ref[2]
    m.sync()
    assert same(tt._from_tensor(d_t), ref[0]) and (d_c is None or same(ts._col_from(d_c), ref[1]))
    torch.cuda.synchronize()
    assert m.export_raw().tobytes() == before
    m.close()


def test_the_large_box_leaving_entirely():
    """266 240 records: 1040 blocks of leaving cells, more than one pass of the scan's 1024 threads."""
    c = fc.big_case()
    m = tt._map()
    want = mapfile.tsdf_shift_records(c["cells"], c["color"], c["lo"], c["delta"])
    assert want[3]["records"] == 266240
    for device, device_out in ((True, True), (False, False)):
        rc, dst, cdst, rec, n, info = _shift(m, c["cells"], c["color"], c["lo"], c["delta"], "emit", device, device_out)
        assert rc == 0 and n == 266240 and same(rec, want[2]) and same(dst, want[0]) and same(cdst, want[1]) and info == _info_list(want[3])
    # a shift that keeps most of it: the records of one plane, and the refill of all records of the first shift elsewhere
    part = mapfile.tsdf_shift_records(c["cells"], c["color"], c["lo"], (1, -1, 4))
    rc, dst, cdst, rec, n, info = _shift(m, c["cells"], c["color"], c["lo"], (1, -1, 4), "emit", True, True)
    assert rc == 0 and n == len(part[2]) and same(rec, part[2]) and same(dst, part[0]) and same(cdst, part[1]) and info == _info_list(part[3])
    lo2 = (c["lo"][0] + 32, c["lo"][1], c["lo"][2])  # half of the records lie outside this box
    zero, czero = np.zeros_like(c["cells"]), np.zeros_like(c["color"])
    ref = mapfile.tsdf_refill_records(zero, czero, lo2, want[2])
    assert ref[2] == {"records": 266240, "applied": 133120, "outside": 133120}
    d_t, d_c = tt._as_tensor(zero), ts._col_tensor(czero)
    assert m.refill_into(d_t, lo2, _rec_tensor(want[2]), d_color=d_c) == ref[2]
    m.sync()
    assert same(tt._from_tensor(d_t), ref[0]) and same(ts._col_from(d_c), ref[1])
    m.close()


def test_the_exact_properties_on_the_device():
    import torch
    m = tt._map()
    # (a) there and back: shift(d), shift(-d), refill(the records) restores both volumes
    for name in ("3x5x7 by (1, -2, 3)", "3x3x33 by dz 5", "3x3x5 by dz -4", "2x2x75 by (0, 0, 37)", "3x5x7 by (3, 0, 0)", "3x3x4 by (1, -1, 1)"):
        c = fc.shift_cases()[name]
        color = c["color"] if c["color"] is not None else np.zeros(c["cells"].shape, COLOR)
        d = np.asarray(c["delta"])
        a_t, a_c = tt._as_tensor(c["cells"]), ts._col_tensor(color)
        b_t, b_c = torch.empty_like(a_t), torch.empty_like(a_c)
        n, info = m.shift_into(b_t, a_t, c["lo"], d, b_c, a_c, count_only=True)
        d_rec = torch.zeros(32 * max(n, 1), dtype=torch.uint8, device="cuda")
        assert m.shift_into(b_t, a_t, c["lo"], d, b_c, a_c, d_records=d_rec)[0] == n
        a_t.fill_(-1)
        a_c.fill_(-1)
        spare = torch.zeros(32, dtype=torch.uint8, device="cuda")
        n2, info2 = m.shift_into(a_t, b_t, np.asarray(c["lo"]) + d, -d, a_c, b_c, d_records=spare)
        assert n2 == 0 and info2["records"] == 0, "what entered was empty"
        r = m.refill_into(a_t, c["lo"], d_rec, n, d_color=a_c)
        m.sync()
        assert r == {"records": n, "applied": n, "outside": 0}
        assert same(tt._from_tensor(a_t), c["cells"]) and same(ts._col_from(a_c), color), name
    # (b) shifts with no opposite signs compose
    for seed, (lo, n3), d1, d2 in fc.composition_cases():
        cells, col = fc.random_volume(seed, n3)
        whole = mapfile.tsdf_shift_records(cells, col, lo, np.asarray(d1) + d2)
        a_t, a_c = tt._as_tensor(cells), ts._col_tensor(col)
        b_t, b_c, c_t, c_c = torch.empty_like(a_t), torch.empty_like(a_c), torch.empty_like(a_t), torch.empty_like(a_c)
        r1, r2 = torch.zeros(32 * cells.size, dtype=torch.uint8, device="cuda"), torch.zeros(32 * cells.size, dtype=torch.uint8, device="cuda")
        n1 = m.shift_into(b_t, a_t, lo, d1, b_c, a_c, d_records=r1)[0]
        n2 = m.shift_into(c_t, b_t, np.asarray(lo) + d1, d2, c_c, b_c, d_records=r2)[0]
        m.sync()
        assert same(tt._from_tensor(c_t), whole[0]) and same(ts._col_from(c_c), whole[1])
        both = np.concatenate([_rec_from(r1, n1), _rec_from(r2, n2)])
        assert same(both[np.argsort(both["key"], kind="stable")], whole[2])
    m.close()


def test_argument_errors_write_nothing():
    import torch
    L = _lib.lib()
    m = tt._map(sc.records_at([(1, 1, 1), (2, 3, 1)]).astype(tt.RAW))
    before = m.export_raw().tobytes()
    lo, n = (-2, -1, 6), (4, 3, 5)
    good = tt._box(lo, n)
    R = 1 << 20
    bad_boxes = [tt._box((0, 0, 0), (0, 3, 5)), tt._box((0, 0, 0), (4, -1, 5)), tt._box((0, 0, 0), (4, 3, 1025)), tt._box((0, 0, 0), (1024, 1024, 129)),
                 tt._box((-R - 1, 0, 0), (4, 3, 5)), tt._box((0, 0, R - 5), (4, 3, 6))]
    t = torch.zeros(16384, dtype=torch.uint8, device="cuda")
    base = t.data_ptr()
    dp = lambda off: vp(base + off)  # noqa: E731
    src, csrc = np.full(n, SENT_T, CELL), np.full(n, SENT_C, COLOR)
    dst, cdst = np.full(n, SENT_T, CELL), np.full(n, SENT_C, COLOR)
    both = np.full((2,) + n, SENT_T, CELL)  # overlapping host ranges
    rec = np.full(64, SENT_R, RECORD)
    info = np.full(8, 9, np.uint64)
    nrec = C.c_size_t(77)
    hp = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    d0 = (C.c_int32 * 3)(1, 0, -1)

    def shift(box=good, delta=d0, s=hp(src), cs=hp(csrc), d=hp(dst), cd=hp(cdst), dev=0, r=hp(rec), cap=64, pn=nrec, do=0, i=hp(info), mm=m):
        return L.revo_map_tsdf_shift(mm._h if mm is not None else None, C.byref(box) if box is not None else None, delta, s, cs, d, cd, dev, r, cap,
                                     C.byref(pn) if pn is not None else None, do, i)

    for j, b in enumerate(bad_boxes):
        assert shift(b) == INVALID_ARG and L.revo_last_error(), j
    vol = 8 * 60  # the bytes of a TSDF volume of the box; a colour volume has twice as many
    got = [shift(mm=None), shift(box=None), shift(delta=None), shift(s=None), shift(d=None), shift(cs=None), shift(cd=None), shift(pn=None),
           shift(dev=2), shift(dev=-1), shift(do=2), shift(do=-1),
           shift(box=tt._box((R - 4, 0, 0), (4, 3, 5)), delta=(C.c_int32 * 3)(1, 0, 0)),      # the destination box passes the rim
           shift(box=tt._box((0, -R, 0), (4, 3, 5)), delta=(C.c_int32 * 3)(0, -1, 0)),
           shift(delta=(C.c_int32 * 3)(0, 0, 2 ** 31 - 1)),
           shift(d=hp(src)), shift(s=hp(both), d=vp(both.ctypes.data + vol - 8)), shift(cd=hp(csrc)), shift(d=hp(csrc), cs=hp(csrc)),   # overlap
           shift(s=dp(0), cs=dp(1024), d=dp(0), cd=dp(4096), dev=1), shift(s=dp(0), cs=dp(1024), d=dp(vol - 16), cd=dp(4096), dev=1),
           shift(s=dp(8), cs=dp(1024), d=dp(2048), cd=dp(4096), dev=1), shift(s=dp(0), cs=dp(1024 + 8), d=dp(2048), cd=dp(4096), dev=1),  # misaligned
           shift(s=dp(0), cs=dp(1024), d=dp(2048 + 4), cd=dp(4096), dev=1), shift(s=dp(0), cs=dp(1024), d=dp(2048), cd=dp(4096 + 8), dev=1),
           shift(r=dp(8192 + 8), do=1),
           shift(s=dp(0), cs=dp(1024), d=dp(2048), cd=dp(4096), dev=1, r=None, pn=None, i=dp(8192 + 8))]
    assert got == [INVALID_ARG] * len(got), got
    # revo_map_tsdf_refill
    good_rec = np.zeros(2, RECORD)
    good_rec["key"] = [fr.key(*lo), fr.key(lo[0], lo[1], lo[2] + 1)]
    good_rec["weight"] = 1
    rinfo = np.full(4, 9, np.uint64)

    def refill(box=good, v=hp(dst), cv=hp(cdst), dev=0, k=2, r=hp(good_rec), di=0, mm=m):
        return L.revo_map_tsdf_refill(mm._h if mm is not None else None, C.byref(box) if box is not None else None, v, cv, dev, k, r, di,
                                      C.cast(hp(rinfo), C.POINTER(MapTsdfRefillInfo)))

    for j, b in enumerate(bad_boxes):
        assert refill(b) == INVALID_ARG, j
    got = [refill(mm=None), refill(box=None), refill(v=None), refill(r=None), refill(dev=2), refill(di=-1), refill(k=(1 << 30) + 1),
           refill(v=dp(8), cv=dp(1024), dev=1), refill(v=dp(0), cv=dp(1024 + 4), dev=1), refill(r=dp(8192 + 16 + 8), di=1)]
    assert got == [INVALID_ARG] * len(got), got
    m.sync()
    for a, s in ((src, SENT_T), (dst, SENT_T), (csrc, SENT_C), (cdst, SENT_C), (both, SENT_T), (rec, SENT_R)):
        assert np.all(a == s)
    assert np.all(info == 9) and np.all(rinfo == 9) and nrec.value == 77
    assert not t.cpu().numpy().any() and m.export_raw().tobytes() == before
    # the handle is as usable as before; info may be NULL, n = 0 is valid with NULL records, the TSDF volume alone is valid
    assert shift(i=None) == 0 and nrec.value == 60 - 3 * 3 * 4 and refill(k=0, r=None) == 0 and rinfo.tolist() == [0, 0, 0, 0]
    assert shift(cs=None, cd=None) == 0 and m.info()["voxels"] == 2
    m.close()


def test_a_refused_refill_changes_no_byte():
    m = tt._map()
    cells, col = fc.random_volume(3, (3, 5, 7))
    lo = (-1, -2, 5)
    _, _, rec, _ = mapfile.tsdf_shift_records(cells, col, lo, (1, 0, 2))
    one = np.zeros(1, RECORD)
    one["key"] = fr.key(lo[0] + 2, lo[1] + 4, lo[2] + 6)   # the last cell: every record before it would have been applied
    full, cfull = np.zeros_like(cells), np.zeros_like(col)
    full[2, 4, 6] = (1 << 30, 1 << 20)
    cfull[2, 4, 6] = (255 << 20, 255 << 20, 255 << 20, 1 << 20)
    rows = rec[rec["key"] < one["key"][0]]
    assert len(rows) >= 3
    bad = {"out of order": rows[::-1], "a duplicate key": np.concatenate([rows[:2], rows[1:]])}
    for field, step in (("sum", 1), ("weight", 1), ("sum_b", 1), ("sum_g", 1), ("sum_r", 1), ("color_weight", 1), ("weight", 0xFFF00000), ("sum_b", 0xFFFFFFFF)):
        r = one.copy()
        r[field] = step
        bad["%s + %d does not FIT" % (field, step)] = np.concatenate([rows, r])
    top = one.copy()
    top["key"] |= np.uint64(1 << 63)
    bad["bit 63"] = np.concatenate([rows, top])
    for why, r in bad.items():
        with pytest.raises(ValueError):
            mapfile.tsdf_refill_records(full, cfull, lo, r)
        with pytest.raises(api.RevoError) as e:  # host volumes: the api copies, so the raw call below checks the caller's bytes
            m.surface_refill(full, lo, r, cfull)
        assert e.value.code == INVALID_ARG, why
        d_t, d_c = tt._as_tensor(full), ts._col_tensor(cfull)
        with pytest.raises(api.RevoError) as e:
            m.refill_into(d_t, lo, _rec_tensor(r), d_color=d_c)
        m.sync()
        assert e.value.code == INVALID_ARG and same(tt._from_tensor(d_t), full) and same(ts._col_from(d_c), cfull), why
        h_t, h_c, h_r = full.copy(), cfull.copy(), np.ascontiguousarray(r)
        box = tt._box(lo, cells.shape)
        assert _lib.lib().revo_map_tsdf_refill(m._h, C.byref(box), h_t.ctypes.data_as(vp), h_c.ctypes.data_as(vp), 0, len(h_r), h_r.ctypes.data_as(vp), 0,
                                               None) == INVALID_ARG
        assert same(h_t, full) and same(h_c, cfull), why
    # colour words without a colour volume, also in a record outside the box
    coloured = rows[rows["color_weight"] > 0][:1].copy()
    far = coloured.copy()
    far["key"] = fr.key(1000, 1000, 1000)
    assert len(coloured) == 1
    for r in (coloured, far):
        d_t = tt._as_tensor(full)
        with pytest.raises(api.RevoError):
            m.refill_into(d_t, lo, _rec_tensor(r))
        m.sync()
        assert same(tt._from_tensor(d_t), full)
    # back from the limit, and a record outside the box that is only counted
    neg = one.copy()
    neg["sum"] = -1
    far["weight"] = 0xFFFFFFFF
    r = np.concatenate([neg, far])
    want = mapfile.tsdf_refill_records(full, cfull, lo, r)
    got = m.surface_refill(full, lo, r, cfull)
    assert same(got[0], want[0]) and same(got[1], want[1]) and got[2] == want[2] == {"records": 2, "applied": 1, "outside": 1}
    m.close()


def test_interleaved_with_the_calls_that_share_the_host_volumes_buffers():
    """A host source volume goes through the handle's tsdfvol and tsdfcol, which fuse, mesh, the surface ray cast and the tracker
    stage through too, and the calls' own scratch only grows: on one handle, in both sizes of map_shared_cases and in every order of
    two, each call gives what it gives alone (map_shared_cases' rule)."""
    import map_shared_cases as ms

    def shift(m, size):
        cells, col = ms.tsdf_volume(size)
        out = m.surface_shift(cells, ms.BOX[size][0], (1, -2, 3), col)
        back = m.surface_refill(np.zeros_like(cells), ms.BOX[size][0], out[2], np.zeros_like(col))
        return [out[0].tobytes(), out[1].tobytes(), out[2].tobytes(), repr(out[3]), back[0].tobytes(), back[1].tobytes(), repr(back[2])]

    others = {name: ms.FEATURES[name] for name in ("fuse", "mesh", "surface_raycast", "fuse_color", "mesh_attr")}
    alone = {}
    for size in ms.SIZES:
        for name, fn in list(others.items()) + [("shift", shift)]:
            m = tt._map(ms.base_records(), ms.VOXEL)
            alone[name, size] = fn(m, size)
            m.close()
        cells, col = ms.tsdf_volume(size)
        want = mapfile.tsdf_shift_records(cells, col, ms.BOX[size][0], (1, -2, 3))
        assert alone["shift", size][:3] == [want[0].tobytes(), want[1].tobytes(), want[2].tobytes()] and len(want[2]) > 0, size
    m = tt._map(ms.base_records(), ms.VOXEL)
    for big, small in (("large", "small"), ("small", "large")):
        for name, fn in others.items():
            assert fn(m, big) == alone[name, big], (name, big)
            assert shift(m, small) == alone["shift", small], (name, "then shift", small)
            assert shift(m, big) == alone["shift", big], (name, "then shift", big)
            assert fn(m, small) == alone[name, small], ("shift then", name, small)
    m.close()


# ------------------------------------------------------------------------------------------------------ a following surface --
def _device_view(v):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(v[0], F)).cuda(), v[1], v[2], torch.from_numpy(np.ascontiguousarray(v[3])).cuda())


def test_a_following_surface_is_the_sequence_rule():
    m = tt._map(voxel=fc.V)
    views = fc.follow_views()
    surf = api.FollowingSurface(m, fc.FOLLOW_N, trunc=0.5, step=fc.FOLLOW_STEP)
    assert surf.ahead == 0.5 and surf.lo.tolist() == [-6, -6, 0] and surf.shifts == 0 and len(surf.store) == 0
    boxes = []
    for v in views:
        surf.integrate(_device_view(v))
        boxes.append(surf.lo.astype(np.int64).copy())
        assert boxes[-1].tolist() == mapfile.follow_lo(v[1], fc.FOLLOW_N, fc.V, 0.5, fc.FOLLOW_STEP).tolist()
    print("boxes", [b.tolist() for b in boxes], "shifts", surf.shifts, "store", len(surf.store))
    assert surf.shifts >= 3 and surf.views == 6 and boxes[0].tolist() == boxes[-1].tolist()
    assert all(len({tuple(b)[k] for b in boxes}) > 1 for k in range(3)), "the box moves on every axis"
    assert surf.shift_info is not None and surf.shift_info["dropped"] == 0
    # assemble() is the sequence rule, byte for byte, in both volumes
    want = fr.sequence(fc.V, fc.FOLLOW_N, [v[:3] for v in views], [v[3] for v in views], boxes, 0.5)
    whole = surf.assemble()
    ref = fr.sequence_volume(want, whole.lo, whole.n)
    assert same(whole.cells, ref[0]) and same(whole.color, ref[1]) and int((whole.cells["weight"] > 0).sum()) > 0
    assert int(sum(1 for w in want.values())) == int(mapfile._tsdf_cells_nonempty(whole.cells, whole.color).sum())
    # the cells that lay in every one of the six boxes: one plain fuse over a fixed box
    a = np.max(boxes, axis=0)
    e = np.min(boxes, axis=0) + fc.FOLLOW_N
    assert np.all(e > a)
    plain = m.fuse([v for v in views], lo=boxes[-1], n=fc.FOLLOW_N, trunc=0.5, color=True)
    cur = surf.volume()
    sl = tuple(slice(int(a[k] - boxes[-1][k]), int(e[k] - boxes[-1][k])) for k in range(3))
    assert same(np.ascontiguousarray(cur.cells[sl]), np.ascontiguousarray(plain.cells[sl]))
    assert same(np.ascontiguousarray(cur.color[sl]), np.ascontiguousarray(plain.color[sl])) and int((plain.cells[sl]["weight"] > 0).sum()) > 0
    # track and raycast on the moved box: the same calls on a TsdfVolume of the same bytes and lo
    assert cur.lo.tolist() == surf.lo.tolist()
    T = views[-1][1]
    k4 = fc.KC[:4]
    r0 = surf.raycast(T, camera=k4, size=(16, 12), zrange=fc.KC[4:])
    r1 = cur.raycast(T, camera=k4, size=(16, 12), zrange=fc.KC[4:])
    assert r0["hits"] == r1["hits"] and r0["depth"].tobytes() == r1["depth"].tobytes() and r0["bgr"].tobytes() == r1["bgr"].tobytes()
    assert r0["normals"].tobytes() == r1["normals"].tobytes() and r0["info"] == r1["info"]
    frame = (views[-1][0], fc.KC[:4], fc.KC[4:])
    t0 = surf.track_eval(frame, np.stack([T]))
    t1 = cur.track_eval(frame, np.stack([T]))
    assert bytes(t0[0]) == bytes(t1[0]) and int(t0[0].considered) == 16 * 12
    start = T.copy()
    start[:3, 3] += F([0.01, -0.005, 0.008])  # a little off the view's pose, so that the loop has something to do
    for kw in ({}, {"max_dist": 0.5, "min_matched": 6}):
        g0, g1 = surf.track(frame, start, **kw), cur.track(frame, start, **kw)
        print("track", kw, "status", g0["status"], "iterations", g0["iterations"], "matched", int(g0["info"].matched))
        assert np.asarray(g0["T"]).tobytes() == np.asarray(g1["T"]).tobytes() and bytes(g0["info"]) == bytes(g1["info"])
        assert (g0["iterations"], g0["status"]) == (g1["iterations"], g1["status"])
    assert int(g0["info"].matched) > 0, "the frame meets the moved box's surface"
    # mesh() meshes the assembled volume
    mesh = surf.mesh()
    wm = mapfile.mesh_attr_records(whole.cells, whole.color, whole.lo, m.voxel)
    assert mesh.vertices.tobytes() == wm.vertices.tobytes() and mesh.triangles.tobytes() == wm.triangles.tobytes()
    # SurfaceVolume.shift(spill=False) drops, and refill puts records back
    plainv = api.SurfaceVolume(m, boxes[-1], fc.FOLLOW_N, trunc=0.5)
    for v in views[:2]:
        plainv.integrate(_device_view(v))
    v0 = plainv.volume()
    rec = plainv.shift((2, 0, -2))
    wsh = mapfile.tsdf_shift_records(v0.cells, v0.color, v0.lo, (2, 0, -2))
    v1 = plainv.volume()
    assert same(rec, wsh[2]) and same(v1.cells, wsh[0]) and same(v1.color, wsh[1]) and v1.lo.tolist() == (v0.lo + (2, 0, -2)).tolist()
    assert plainv.shift((-2, 0, 2), spill=False) is None and plainv.shift_info is None
    assert plainv.refill(rec) == {"records": len(rec), "applied": len(rec), "outside": 0}
    v2 = plainv.volume()
    assert same(v2.cells, v0.cells) and same(v2.color, v0.color) and v2.lo.tolist() == v0.lo.tolist()
    # the kept record buffer: a shift with fewer records than it holds emits straight into it, one with more grows it first
    sizes = []
    for d in ((1, 0, 0), fc.FOLLOW_N):
        held, cap = plainv.volume(), plainv._spill.numel() // 32
        rec = plainv.shift(d)
        wsh2 = mapfile.tsdf_shift_records(held.cells, held.color, held.lo, d)
        now = plainv.volume()
        assert same(rec, wsh2[2]) and same(now.cells, wsh2[0]) and same(now.color, wsh2[1]) and plainv.shift_info == wsh2[3]
        sizes.append((cap, len(rec)))
    print("record buffer, records:", sizes)
    assert sizes[0][1] <= sizes[0][0] and sizes[1][1] > sizes[1][0]
    with pytest.raises(ValueError):
        plainv.shift(((1 << 20), 0, 0))
    # a store of the caller's: checked at creation, taken from at the first follow, and left whole by a refill that is refused
    with pytest.raises(ValueError):
        api.FollowingSurface(m, fc.FOLLOW_N, trunc=0.5, step=fc.FOLLOW_STEP, store=mapfile.SurfaceStore(voxel=0.25, trunc=0.5))
    with pytest.raises(ValueError):
        api.FollowingSurface(m, fc.FOLLOW_N, trunc=0.5, step=fc.FOLLOW_STEP, store=mapfile.SurfaceStore(voxel=fc.V, trunc=0.25))
    heavy = np.zeros(1, RECORD)
    heavy["key"], heavy["weight"], heavy["sum_b"], heavy["color_weight"] = fr.key(*boxes[0]), 1 << 20, 7, 1
    grey = api.FollowingSurface(m, fc.FOLLOW_N, trunc=0.5, color=False, step=fc.FOLLOW_STEP, store=mapfile.SurfaceStore(heavy, fc.V, 0.5))
    with pytest.raises(ValueError):
        grey.follow(views[0][1])  # colour words and no colour volume
    assert same(grey.store.records, heavy)
    mine = api.FollowingSurface(m, fc.FOLLOW_N, trunc=0.5, step=fc.FOLLOW_STEP, store=mapfile.SurfaceStore(heavy, fc.V, 0.5))
    assert mine.follow(views[0][1]) is False and len(mine.store) == 0 and mine.volume().cells[0, 0, 0]["weight"] == 1 << 20
    mine.store.add(heavy)
    with pytest.raises(api.RevoError):
        mine._take_back()  # the cell would pass 2^20
    assert same(mine.store.records, heavy) and mine.volume().cells[0, 0, 0]["weight"] == 1 << 20
    # the window forwards
    win = api.MapWindow(tt.tr._scene()[1], fc.V, dense=True, window=2)
    got = win.surface_shift(v0.cells, v0.lo, (2, 0, -2), v0.color)
    assert same(got[2], wsh[2]) and win.surface_refill(wsh[0], v1.lo, rec[:0], wsh[1])[2]["records"] == 0
    win.close()
    m.close()


def test_the_running_sequence_follows():
    """vo.REVO(surface=FollowingSurface) up to the second keyframe of the synthetic sequence is the sequence rule over the reported
    keyframes; the voxel (5 cm) and the step (1 cell) are chosen so that the pan between two keyframes moves the box."""
    from lm_settings_cases import S160
    from revo_amd import vo
    frames = ts._two_keyframes(S160)
    cam = api.CameraPyr(S160)
    vm = api.VoxelMap(cam, 0.05, dense=True)
    n = (48, 48, 40)
    surf = api.FollowingSurface(vm, n, step=1, ahead=2.0)
    g = vo.REVO(S160, cameraPyr=cam, voxelMap=vm, surface=surf)
    by_ts = {float(f[2]): f[0] for f in frames}
    views, boxes = [], []
    for f in frames:
        _, kf = g.push(f[0], f[1], f[2])
        if kf:
            pyr, T = g.keyframe()
            views.append((pyr.returnDepth(0).copy(), np.array(T, F), None, np.ascontiguousarray(by_ts[float(pyr.returnTimestamp())])))
            boxes.append(surf.lo.astype(np.int64).copy())
        if len(views) == 2:
            break
    assert len(views) == 2 == surf.views and g.surface_skipped == 0, "the sequence gives two keyframes"
    print("boxes", [b.tolist() for b in boxes], "shifts", surf.shifts)
    assert [b.tolist() for b in boxes] == [mapfile.follow_lo(v[1], n, 0.05, 2.0, 1).tolist() for v in views]
    # the rule, through the library's own fuse of each keyframe over the box it was fused in (the per-cell loop over 160 x 120 pixel
    # views is pinned to it by the tests of DESIGN 27)
    store = mapfile.SurfaceStore(voxel=vm.voxel, trunc=surf.trunc)
    for v, lo in zip(views, boxes):
        one = vm.fuse([v], lo=lo, n=n, color=True)
        store.add(mapfile.tsdf_volume_records(one.cells, one.color, lo))
    whole = surf.assemble()
    ref = store.volume(whole.lo, whole.n)
    assert same(whole.cells, ref[0]) and same(whole.color, ref[1]) and int((whole.cells["weight"] > 0).sum()) > 0
    assert surf.shifts >= 1, "two keyframes of this pan move a box of 5 cm cells snapped to single cells"
    # with surface_track the box follows the keyframe's pose before it is tracked
    vm2 = api.VoxelMap(cam, 0.05, dense=True)
    surf2 = api.FollowingSurface(vm2, n, step=1, ahead=2.0)
    g3 = vo.REVO(S160, cameraPyr=cam, voxelMap=vm2, surface=surf2, surface_track=True)
    kfs = 0
    for f in frames:
        _, kf = g3.push(f[0], f[1], f[2])
        kfs += bool(kf)
        if kfs == 2:
            break
    assert len(g3.surface_tracks) == 2 and surf2.views == 2
    assert surf2.lo.tolist() == mapfile.follow_lo(g3.surface_tracks[-1][2], n, 0.05, 2.0, 1).tolist()
    vm.close()
    vm2.close()


def test_run_tum_surface_follow(tmp_path, monkeypatch, capsys):
    from lm_settings_cases import S160
    from revo_amd import run_tum, tum
    from test_gpu_vo_multi import _tum_yaml
    name = "rgbd_synth_f"
    tum.write_synthetic_dataset(str(tmp_path / "data" / name), ts._two_keyframes(S160)[:12])
    _tum_yaml(tmp_path, S160, [name])
    monkeypatch.chdir(tmp_path)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "0", "--map", "0.05"]
    follow = ["--surface", "surface.ply", "--surface-trunc", "0.2", "--surface-follow", "--surface-follow-size", "64", "64", "64", "--surface-follow-step", "4"]
    assert run_tum.main(args + follow + ["--surface-store", "store.npz"]) == 0
    out = capsys.readouterr().out
    assert "Surface:" in out and "Surface store:" in out
    mesh = mapfile.Mesh.load_ply(str(tmp_path / "surface.ply"))
    assert len(mesh.triangles) > 0 and mesh.normals is not None and mesh.colors is not None
    store = mapfile.SurfaceStore.load(str(tmp_path / "store.npz"))
    assert len(store) > 0 and store.voxel == float(F(0.05)) and store.trunc == float(F(0.2))
    # the store holds the whole surface: assembled, it meshes to the file's mesh
    assert mapfile.main(["surface-assemble", "store.npz", "-o", "tsdf.npz"]) == 0
    cells, lo, voxel, _, col = mapfile.read_tsdf("tsdf.npz", color=True)
    wm = mapfile.mesh_attr_records(cells, col, lo, voxel)
    assert len(wm.vertices) == len(mesh.vertices) and len(wm.triangles) == len(mesh.triangles)
    # usage errors, each with a message
    assert run_tum.main(args + follow + ["--surface-box", "-40", "-40", "0", "80", "80", "100"]) == 2
    assert run_tum.main(args + follow + ["--surface-views", "views"]) == 2
    assert run_tum.main(args + ["--surface-follow"]) == 2 and run_tum.main(args + ["--surface", "s.ply", "--surface-follow-step", "4"]) == 2
    assert run_tum.main(args + follow[:5] + ["--surface-follow-step", "0"]) == 2 and run_tum.main(args + follow[:5] + ["--surface-follow-size", "4", "4"]) == 2
    assert capsys.readouterr().out.count("--surface-follow") >= 6
