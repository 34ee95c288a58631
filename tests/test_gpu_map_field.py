"""The voxel map's distance field on the device (revo_map_distance_field / revo_map_bounds / revo_map_df_sample,
api.VoxelMap.distance_field / distance_field_into / bounds / df_sample / sample_into): field bytes and the info record
bit for bit revo_amd.mapfile's restatement (which test_map_field_cpu.py pins to the brute-force definition) on one hand-made
case per rule and kernel path, a random box and the 35 000-voxel scene; the same bytes whatever the order of the records, the
table size and the output side, and directly behind an integration; the map is never changed; bounds; samples from a host and
from a device field; every argument error; and run_tum --map-esdf against `mapfile esdf`."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile, synth  # noqa: E402
from revo_amd.settings import DF_NONE, MapDfBox, MapDfInfo  # noqa: E402

import map_field_cases as fc  # noqa: E402
import map_field_ref as fr  # noqa: E402
import test_gpu_map_raycast as tr  # noqa: E402

F = np.float32
RAW = mapfile.RAW_DTYPE
INVALID_ARG = -1
VOXEL = tr.VOXEL
V = fc.V
SENTINEL = 0x07070707


def _box(lo, n):
    return MapDfBox((C.c_int32 * 3)(*[int(x) for x in lo]), (C.c_int32 * 3)(*[int(x) for x in n]))


def _field(m, lo, n, min_count=1, clamp=0, device=False):
    """revo_map_distance_field into sentinel-filled host or device outputs -> (d2, info dict); the map's records are the same
    before and after."""
    from revo_amd import _lib
    before = m.export_raw().tobytes()
    box = _box(lo, n)
    shape = tuple(int(x) for x in n)
    if device:
        import torch
        dev = "cuda:%d" % m.cameraPyr.device
        d = torch.full(shape, SENTINEL, dtype=torch.int32, device=dev)
        i = torch.full((8,), 9, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        _lib.check(_lib.lib().revo_map_distance_field(m._h, C.byref(box), min_count, clamp, C.c_void_p(d.data_ptr()), 1, C.c_void_p(i.data_ptr())))
        m.sync()
        d2, i = d.cpu().numpy().view(np.uint32), i.cpu().numpy()
        assert not i[5:].any()
        info = dict(zip(mapfile.DF_INFO_KEYS, (int(x) for x in i[:5])))
    else:
        d2 = np.full(shape, SENTINEL, np.uint32)
        i = MapDfInfo()
        _lib.check(_lib.lib().revo_map_distance_field(m._h, C.byref(box), min_count, clamp, d2.ctypes.data_as(C.c_void_p), 0, C.byref(i)))
        assert not any(i.reserved)
        info = {k: int(getattr(i, k)) for k in mapfile.DF_INFO_KEYS}
    assert m.export_raw().tobytes() == before
    return d2, info


def _check(m, rec, lo, n, what, min_count=1, clamp=0, want=None):
    want = want or mapfile.distance_field_records(rec.astype(RAW), lo, n, min_count, clamp)
    for device in (False, True):
        got = _field(m, lo, n, min_count, clamp, device)
        print("%s (%s output): %s" % (what, "device" if device else "host", got[1]))
        assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape
        assert got[0].tobytes() == want[0].tobytes(), (what, device, int(np.sum(got[0] != want[0])))
        assert got[1] == want[1], (what, device, got[1], want[1])
    return want


@pytest.mark.parametrize("case", fc.cases(), ids=lambda c: c["name"])
def test_hand_made_cases_bit_exact(case):
    rec = fc.records(case["cells"]).astype(RAW)
    m = tr._hand(rec, V, initial_voxels=1)
    want = _check(m, rec, case["lo"], case["n"], case["name"], case["min_count"], case["clamp"])
    if not want[1]["solid"]:
        assert np.all(want[0] == DF_NONE) and want[1]["max_d2"] == 0 and want[1]["outside"] + want[1]["below"] == len(rec)
    if case["name"].startswith("long axis 0"):
        assert want[1]["max_d2"] == fc.LONG_MAX_FIRST
    if case["name"].startswith("random"):
        assert want[0].tobytes() == fr.brute_force(rec, case["lo"], case["n"])[0].tobytes()
    m.close()


def test_the_api_and_the_window():
    import torch
    api, cam = tr._scene()[:2]
    c = fc.random_case(seed=11, n=(20, 12, 9), voxels=40, counts=True)
    rec = fc.records(c["cells"]).astype(RAW)
    m = tr._hand(rec, V)
    lo, hi, n = mapfile.bounds_records(rec, 2)
    f = m.distance_field(pad=3, min_count=2, clamp=30)
    want, info = mapfile.distance_field_records(rec, lo - 3, hi - lo + 7, 2, 30)
    assert f.d2.tobytes() == want.tobytes() and f.lo.tolist() == (lo - 3).tolist() and f.n.tolist() == list(want.shape) and f.info == info
    assert f.voxel == m.voxel == V and m.last_distance_field_ms() > 0
    g = m.distance_field(lo=c["lo"], n=c["n"])
    assert g.d2.tobytes() == mapfile.distance_field_records(rec, c["lo"], c["n"])[0].tobytes()
    assert m.distance_field().n.tolist() == (mapfile.bounds_records(rec)[1] - mapfile.bounds_records(rec)[0] + 17).tolist()  # pad 8
    with pytest.raises(ValueError):
        m.distance_field(lo=(0, 0, 0))
    with pytest.raises(ValueError):
        m.distance_field(lo=(0, 0, 0), n=(1025, 1, 1))
    # into a device tensor, with and without the info record
    d = torch.full(tuple(c["n"]), 7, dtype=torch.int32, device="cuda")
    i = torch.zeros(8, dtype=torch.int64, device="cuda")
    m.distance_field_into(d, c["lo"], c["n"], d_info=i)
    assert d.cpu().numpy().view(np.uint32).tobytes() == g.d2.tobytes() and i.cpu().numpy().tolist()[:5] == [g.info[k] for k in mapfile.DF_INFO_KEYS]
    d.fill_(7)
    m.distance_field_into(d, c["lo"], c["n"], clamp=5, wait=False)
    m.sync()
    assert d.cpu().numpy().view(np.uint32).tobytes() == np.minimum(g.d2, 5).tobytes()
    with pytest.raises(ValueError):
        m.distance_field_into(d[:-1], c["lo"], c["n"])
    # a field's samples, on the device and -- the same bytes -- from a loaded field
    a, b = np.asarray(c["lo"]) * V, (np.asarray(c["lo"]) + c["n"]) * V
    pts = np.random.default_rng(2).uniform(a - 0.05, b + 0.05, (300, 3)).astype(F)
    s = g.sample(pts)
    assert s.tobytes() == mapfile.df_sample(g.d2, g.lo, V, pts).tobytes() and np.sum(s["dist"] >= 0) > 20
    # MapWindow forwards to its inner map
    w = api.MapWindow(cam, V, window=2)
    w.map.merge_raw(rec)
    assert w.distance_field(lo=c["lo"], n=c["n"]).d2.tobytes() == g.d2.tobytes() and w.bounds()[2] == len(rec)
    w.close()
    m.close()


def test_same_bytes_whatever_the_conditions():
    c = fc.random_case(seed=3, n=(33, 20, 41), voxels=300, counts=True)
    rec = fc.records(c["cells"]).astype(RAW)
    base = tr._hand(rec, V, initial_voxels=16)
    want = _check(base, rec, c["lo"], c["n"], "base", min_count=2)
    rng = np.random.default_rng(3)
    others = [tr._hand(rec[::-1].copy(), V, initial_voxels=16), tr._hand(rec[rng.permutation(len(rec))], V, initial_voxels=16),
              tr._hand(rec, V, initial_voxels=1 << 18)]
    assert base.info()["capacity"] == 1024 and others[2].info()["capacity"] >= 1 << 19
    two = tr._hand(rec[:100], V, initial_voxels=16)  # merged in two parts
    two.merge_raw(rec[100:])
    for o in others + [two]:
        _check(o, rec, c["lo"], c["n"], "another table", min_count=2, want=want)
        o.close()
    base.close()


@functools.lru_cache(maxsize=None)
def _scene_box():
    """A 96^3 box around the median voxel of the scene map: it holds well over 1000 voxels, counted from the records."""
    rec = tr._scene_records()
    k = mapfile.key_axes(rec["key"])
    lo = np.median(k, 0).astype(np.int64) - 48
    inside = int(np.all((k >= lo) & (k < lo + 96), 1).sum())
    assert inside >= 1000
    return tuple(int(x) for x in lo), (96, 96, 96), inside


@functools.lru_cache(maxsize=None)
def _scene_spec(n_kf=2):
    lo, n, _ = _scene_box()
    return mapfile.distance_field_records(tr._scene_records(n_kf), lo, n)


def test_the_scene_map_and_stream_order():
    api, cam, pyrs, _ = tr._scene()
    P = tr._kf_poses()
    lo, n, inside = _scene_box()
    m = api.VoxelMap(cam, VOXEL, dense=True)
    m.integrate(pyrs[0], P[0])
    first = _field_no_export(m, lo, n)  # no waiting call in between
    m.integrate(pyrs[1], P[1])
    both = _field_no_export(m, lo, n)
    want = _scene_spec()
    assert want[1]["solid"] == inside and want[1]["solid"] + want[1]["outside"] == len(tr._scene_records())
    assert both[0].tobytes() == want[0].tobytes() and both[1] == want[1]
    one = _scene_spec(1)
    assert first[0].tobytes() == one[0].tobytes() and first[1] == one[1] and first[1]["solid"] < both[1]["solid"]
    assert m.export_raw().tobytes() == tr._scene_records().tobytes()
    _check(m, tr._scene_records(), lo, n, "the scene map", want=want)
    print("scene 96^3: last call %.3f ms on the device" % m.last_distance_field_ms())
    # an empty map gives all NONE, before and after a clear
    m.clear()
    for e in (api.VoxelMap(cam, VOXEL), m):
        d2, info = _field(e, lo, (7, 5, 33))
        assert np.all(d2 == DF_NONE) and info == {"cells": 7 * 5 * 33, "solid": 0, "outside": 0, "below": 0, "max_d2": 0}
        b = e.bounds()
        assert b[0].tolist() == [0, 0, 0] and b[1].tolist() == [0, 0, 0] and b[2] == 0


def _field_no_export(m, lo, n):
    """The field call alone: nothing that waits for the map runs before it."""
    from revo_amd import _lib
    box = _box(lo, n)
    d2 = np.full(tuple(n), SENTINEL, np.uint32)
    i = MapDfInfo()
    _lib.check(_lib.lib().revo_map_distance_field(m._h, C.byref(box), 1, 0, d2.ctypes.data_as(C.c_void_p), 0, C.byref(i)))
    return d2, {k: int(getattr(i, k)) for k in mapfile.DF_INFO_KEYS}


def test_bounds():
    rec = fc.records([(1, 1, 1, 1), (-6, 2, 3, 2), (3, 5, -7, 3), (20, 0, 0, 3), (21, -9, 0, 1), (fc.LO_RIM, 4, fc.HI_RIM, 2)]).astype(RAW)
    m = tr._hand(rec, V, initial_voxels=1)
    for mc in (0, 1, 2, 3, 4):
        got, want = m.bounds(mc), mapfile.bounds_records(rec, mc)
        assert (got[0].tolist(), got[1].tolist(), got[2]) == (want[0].tolist(), want[1].tolist(), want[2]), mc
    assert m.bounds(4)[2] == 0 and m.bounds(2)[0].tolist() == [fc.LO_RIM, 0, -7]
    m.close()
    sc = tr._hand(tr._scene_records(), VOXEL)
    k = mapfile.key_axes(tr._scene_records()["key"])
    b = sc.bounds()
    assert (b[0].tolist(), b[1].tolist(), b[2]) == (k.min(0).tolist(), k.max(0).tolist(), len(k))
    sc.close()


def _scene_points(n=4096, seed=7):
    """Points spread over and around the scene box, with points on every face of the box and non-finite ones in between."""
    lo, nn, _ = _scene_box()
    rng = np.random.default_rng(seed)
    a, b = np.asarray(lo) * VOXEL, (np.asarray(lo) + nn) * VOXEL
    p = rng.uniform(a - 0.15 * (b - a), b + 0.15 * (b - a), (n, 3))
    for i in range(3):  # on and next to the lower and the upper face of every axis, the other two coordinates well inside
        for j, x in enumerate((a[i], b[i], a[i] + VOXEL, b[i] - VOXEL, np.nextafter(F(b[i]), F(-1e9)), np.nextafter(F(a[i]), F(-1e9)))):
            rows = 40 * i + 6 * np.arange(6) + j
            p[rows] = rng.uniform(a + 0.25 * (b - a), b - 0.25 * (b - a), (6, 3))
            p[rows, i] = x
    p = p.astype(F)
    odd = [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (3e38, 0, 0), (-3e38, 0, 0), (np.nan, np.nan, np.nan)]
    for j, o in enumerate(odd):
        p[200 + 17 * j] = o
    return p


def test_df_sample_bit_exact():
    import torch
    from revo_amd import _lib, api
    L = _lib.lib()
    lo, n, _ = _scene_box()
    d2 = _scene_spec()[0]
    m = tr._hand(tr._scene_records()[:10], VOXEL)  # the field is an argument: the map gives its voxel edge only
    pts = _scene_points()
    want = mapfile.df_sample(d2, lo, VOXEL, pts)
    inside = want["dist"] >= 0
    print("samples: %d inside, %d outside, largest |grad| %.3f" % (inside.sum(), (~inside).sum(), np.abs(want["grad"]).max()))
    assert 1500 < inside.sum() < 3500 and np.any(want["grad"][inside] != 0)
    field = api.DistanceField(d2, lo, VOXEL)
    assert m.df_sample(field, pts).tobytes() == want.tobytes()  # a host field, host points and output
    # a device field, device points and output; and a host field with device points and output (the field is uploaded)
    d_d2 = torch.from_numpy(d2.view(np.int32)).cuda()
    d_pts = torch.from_numpy(pts).cuda()
    d_out = torch.full((len(pts), 4), 5.0, device="cuda")
    m.sample_into(d_out, d_d2, lo, d_pts)
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    d_out.fill_(5.0)
    torch.cuda.synchronize()
    box = _box(lo, n)
    _lib.check(L.revo_map_df_sample(m._h, C.byref(box), d2.ctypes.data_as(C.c_void_p), 0, len(pts), C.c_void_p(d_pts.data_ptr()), 1, C.c_void_p(d_out.data_ptr()), 1))
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    # a device field into host memory, one point, and a field that is all NONE
    one = np.zeros(1, mapfile.DF_SAMPLE_DTYPE)
    p1 = np.ascontiguousarray(pts[inside][:1])
    _lib.check(L.revo_map_df_sample(m._h, C.byref(box), C.c_void_p(d_d2.data_ptr()), 1, 1, p1.ctypes.data_as(C.c_void_p), 0, one.ctypes.data_as(C.c_void_p), 0))
    assert one.tobytes() == want[inside][:1].tobytes()
    none = m.df_sample(api.DistanceField(np.full(n, DF_NONE, np.uint32), lo, VOXEL), pts)
    assert np.all(none["dist"][inside] == np.inf) and np.all(none["dist"][~inside] == -1) and not none["grad"].any()
    # hand-made fields: one cell, and the faces of a tiny box (test_map_field_cpu.py states their values by hand)
    import test_map_field_cpu as tc
    h = tr._hand(np.zeros(0, RAW), 0.5)
    small = (tc.ROOTS * tc.ROOTS).reshape(3, 1, 4)
    grid = np.stack(np.meshgrid(np.arange(-1.25, 1.5, 0.25), [0.99, 1.0, 1.25, 1.49, 1.5], np.arange(-0.25, 2.5, 0.25), indexing="ij"), -1).reshape(-1, 3)
    for f in (api.DistanceField(small, tc.LO, 0.5), api.DistanceField(np.array([[[9]]], np.uint32), (0, 0, 0), 0.5)):
        assert h.df_sample(f, grid).tobytes() == mapfile.df_sample(f.d2, f.lo, 0.5, grid).tobytes()
    h.close()
    m.close()


def test_argument_errors_write_nothing():
    import torch
    from revo_amd import _lib
    from revo_amd.settings import MapDfSample
    L = _lib.lib()
    rec = fc.records([(1, 1, 1), (2, 3, 1)]).astype(RAW)
    m = tr._hand(rec, V)
    out = np.full(4 * 3 * 5, SENTINEL, np.uint32)
    info = np.full(8, 9, np.uint64)
    op, ip = out.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)
    good = _box((0, 0, 0), (4, 3, 5))
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    base = t.data_ptr()

    def call(box=good, o=op, dev=0, i=ip, mm=m):
        return L.revo_map_distance_field(mm._h if mm is not None else None, C.byref(box) if box is not None else None, 1, 0, o, dev, i)

    R = 1 << 20
    bad_boxes = [_box((0, 0, 0), (0, 3, 5)), _box((0, 0, 0), (4, -1, 5)), _box((0, 0, 0), (4, 3, 1025)), _box((0, 0, 0), (1025, 1, 1)),
                 _box((0, 0, 0), (1024, 1024, 129)), _box((-R - 1, 0, 0), (4, 3, 5)), _box((0, R - 2, 0), (4, 3, 5)), _box((0, 0, R - 5), (4, 3, 6)),
                 _box((0, 0, R), (1, 1, 1)), _box((-(1 << 31), 0, 0), (4, 3, 5)), _box(((1 << 31) - 1, 0, 0), (4, 3, 5))]
    for j, b in enumerate(bad_boxes):
        assert call(b) == INVALID_ARG and L.revo_last_error(), j
    assert [call(mm=None), call(box=None), call(o=None), call(dev=2), call(dev=-1)] == [INVALID_ARG] * 5
    assert [call(o=C.c_void_p(base + 4), dev=1, i=None), call(o=C.c_void_p(base), dev=1, i=C.c_void_p(base + 1024 + 8)),
            call(bad_boxes[0], o=C.c_void_p(base), dev=1, i=None)] == [INVALID_ARG] * 3
    m.sync()
    assert not t.cpu().numpy().any() and np.all(out == SENTINEL) and np.all(info == 9)
    # revo_map_df_sample
    field = np.full(4 * 3 * 5, 4, np.uint32)
    pts = np.full((65, 3), 0.01, F)
    res = np.full(16 * 65, 7, np.uint8)
    fp, pp, rp = field.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)

    def scall(box=good, f=fp, df=0, n=65, p=pp, di=0, o=rp, do=0, mm=m):
        return L.revo_map_df_sample(mm._h if mm is not None else None, C.byref(box) if box is not None else None, f, df, n, p, di, o, do)

    dptr = C.c_void_p(base)
    assert [scall(mm=None), scall(box=None), scall(f=None), scall(p=None), scall(o=None), scall(n=0), scall(n=(1 << 24) + 1), scall(df=2), scall(di=2),
            scall(do=2), scall(df=-1), scall(f=C.c_void_p(base + 4), df=1), scall(p=C.c_void_p(base + 8), di=1), scall(o=C.c_void_p(base + 2048 + 4), do=1),
            scall(f=dptr, df=1, p=C.c_void_p(base + 1024), di=1, o=C.c_void_p(base + 2048 + 12), do=1)] == [INVALID_ARG] * 15
    for j, b in enumerate(bad_boxes):
        assert scall(b) == INVALID_ARG, j
    m.sync()
    assert np.all(res == 7) and not t.cpu().numpy().any()
    # the handle is as usable as before; info may be NULL; the time of a map that has built no field is an error
    ms = C.c_float()
    fresh = tr._hand(rec, V)
    assert L.revo_map_distance_field_last_ms(fresh._h, C.byref(ms)) == INVALID_ARG and L.revo_map_distance_field_last_ms(m._h, None) == INVALID_ARG
    assert L.revo_map_distance_field_last_ms(None, C.byref(ms)) == INVALID_ARG
    lo3, n1 = (C.c_int32 * 3)(), C.c_size_t()
    assert [L.revo_map_bounds(None, 1, lo3, lo3, C.byref(n1)), L.revo_map_bounds(m._h, 1, None, lo3, C.byref(n1)), L.revo_map_bounds(m._h, 1, lo3, None, C.byref(n1)),
            L.revo_map_bounds(m._h, 1, lo3, lo3, None)] == [INVALID_ARG] * 4
    assert call() == 0 and call(i=None) == 0
    want = mapfile.distance_field_records(rec, (0, 0, 0), (4, 3, 5))
    assert out.tobytes() == want[0].tobytes() and info.tolist() == [want[1][k] for k in mapfile.DF_INFO_KEYS] + [0, 0, 0]
    assert L.revo_map_distance_field_last_ms(m._h, C.byref(ms)) == 0 and ms.value > 0
    assert scall() == 0 and C.sizeof(MapDfSample) == 16
    assert res.view(mapfile.DF_SAMPLE_DTYPE).tobytes() == mapfile.df_sample(field.reshape(4, 3, 5), (0, 0, 0), V, pts).tobytes()
    fresh.close()
    m.close()


def test_run_tum_map_esdf(tmp_path, monkeypatch):
    from revo_amd import api, run_tum, tum
    from test_gpu_map_render import S320
    from test_gpu_vo_multi import _tum_yaml
    from test_gpu_voxel_map import BIASES
    name = "rgbd_synth_b"
    seq = synth.make_sequence(952, S320, 33, max_t=0.01, max_rot_deg=0.4, bias=BIASES[4])
    tum.write_synthetic_dataset(str(tmp_path / "data" / name), seq)
    _tum_yaml(tmp_path, S320, [name])
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "2", "--map", "0.02"]
    monkeypatch.chdir(tmp_path)
    assert run_tum.main(args + ["--map-save", "M.rvm", "--map-esdf", "F.npz"]) == 0
    assert run_tum.main(args[:4] + ["--map-esdf", "F2.npz"]) == 2 and run_tum.main(args + ["--map-esdf-pad", "3"]) == 2  # usage errors
    assert mapfile.main(["esdf", "M.rvm", "-o", "G.npz"]) == 0
    with np.load("F.npz") as a, np.load("G.npz") as b:
        assert sorted(a.files) == sorted(b.files) == ["d2", "lo", "n", "voxel"]
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        assert a["d2"].size > 100000 and int((a["d2"] == 0).sum()) == mapfile.read("M.rvm")[0]["voxels"]
    f = api.DistanceField.load("F.npz")
    assert f.voxel == float(F(0.02)) and f.metres().max() > 0.1
