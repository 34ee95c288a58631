"""Known space on the device (revo_map_observe / revo_map_known_field / revo_map_frontiers, api.VoxelMap.observe / observe_into /
distance_field(seen=) / frontiers, api.explore): the seen volume's bytes, the info record and the per-view class counts
bit for bit the per-cell specification tests/map_seen_ref.py on every hand-made case, from host and device images into host and
device volumes; z-lines of every length and alignment; the pyramid form; the three exact properties; the known field, its info
and the frontiers against revo_amd.mapfile's restatement (which test_map_seen_cpu.py pins to the specification); the scene;
every argument error; the route; MapWindow."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile  # noqa: E402
from revo_amd.settings import (DF_NONE, MapCarveViewInfo, MapDfBox, MapKnownInfo, MapObserveInfo, MapObserveParams, MapPlanInfo,  # noqa: E402
                               MapPlanSeed)

import map_carve_cases as cc  # noqa: E402
import map_seen_cases as sc  # noqa: E402
import map_seen_ref as sr  # noqa: E402
import test_gpu_map_raycast as tr  # noqa: E402

F = np.float32
RAW = mapfile.RAW_DTYPE
INVALID_ARG, CAPACITY = -1, -5
SENTINEL = 0xAB
EMPTY = np.zeros(0, RAW)
SEED = np.dtype([("cell", "<i4", (3,)), ("cost0", "<u4")])
CLASS_FIELDS = ("outside", "unknown", "free_space", "confirmed", "occluded", "edge")


def _box(lo, n):
    return MapDfBox((C.c_int32 * 3)(*[int(x) for x in lo]), (C.c_int32 * 3)(*[int(x) for x in n]))


def _map(rec=EMPTY, voxel=sc.V):
    return tr._hand(np.asarray(rec).astype(RAW), voxel)


def _observe(m, lo, n, views, radius=1, margin=None, margin_rel=0.0, before=None, device=False, device_in=False, fill=SENTINEL):
    """revo_map_observe into a host or device volume that holds `before` (an accumulating call) or is filled with `fill`
    -> (seen, info dict, per-view class counts); the info and per-view records start as nines."""
    import torch
    L = _lib.lib()
    if device_in:
        views = [(torch.from_numpy(np.ascontiguousarray(v[0], F)).cuda(),) + tuple(v[1:]) for v in views]
    cv, din, keep = m._carve_views(views)
    nv = len(cv)
    shape = tuple(int(x) for x in n)
    prm = MapObserveParams(int(radius), 0 if before is None else 1, float(m.voxel if margin is None else margin), float(margin_rel))
    start = np.full(shape, fill, np.uint8) if before is None else np.ascontiguousarray(before, np.uint8).copy()
    box = _box(lo, n)
    if device:
        d, i = torch.from_numpy(start).cuda(), torch.full((8,), 9, dtype=torch.int64, device="cuda")
        vi = torch.full((8 * nv,), 9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.revo_map_observe(m._h, C.byref(box), nv, cv, din, C.byref(prm), C.c_void_p(d.data_ptr()), 1, C.c_void_p(i.data_ptr()),
                                      C.c_void_p(vi.data_ptr())))
        m.sync()
        seen, i, vi = d.cpu().numpy(), i.cpu().numpy().tolist(), vi.cpu().numpy().reshape(nv, 8)
    else:
        seen, info, vinfo = start, MapObserveInfo(), (MapCarveViewInfo * nv)()
        _lib.check(L.revo_map_observe(m._h, C.byref(box), nv, cv, din, C.byref(prm), seen.ctypes.data_as(C.c_void_p), 0, C.byref(info),
                                      C.cast(vinfo, C.c_void_p)))
        i = [int(getattr(info, k)) for k in mapfile.SEEN_INFO_KEYS] + list(info.reserved)
        vi = np.array([[getattr(v, k) for k in CLASS_FIELDS] + list(v.reserved) for v in vinfo])
    del keep
    assert i[5:] == [0, 0, 0] and not vi[:, 6:].any()
    counts = [dict(zip(mapfile.CARVE_CLASSES, (int(x) for x in row[:6]))) for row in vi]
    return seen, dict(zip(mapfile.SEEN_INFO_KEYS, i[:5])), counts


def _same(got, want, what):
    assert got[0].dtype == np.uint8 and got[0].shape == want[0].shape, what
    assert got[0].tobytes() == want[0].tobytes(), (what, int(np.sum(got[0] != want[0])))
    assert got[1] == want[1] and got[2] == want[2], (what, got[1], want[1])
    assert all(sum(v.values()) == got[1]["cells"] for v in got[2]), what


SIDES = ((False, False), (True, False), (True, True), (False, True))  # (device volume, device images)


# ------------------------------------------------------------------------------------------------------------- observe --
@pytest.mark.parametrize("name", list(sc.cases()))
def test_hand_made_cases_bit_exact(name):
    c, want = sc.cases()[name], sc.spec(name)
    m = _map()
    before = m.export_raw().tobytes()
    for device, device_in in SIDES:
        got = _observe(m, c["lo"], c["n"], c["views"], c["radius"], c["margin"], c["margin_rel"], device=device, device_in=device_in)
        _same(got, want, (name, device, device_in))
    print(name, want[1], want[2][0])
    assert m.export_raw().tobytes() == before
    m.close()


@pytest.mark.parametrize("lo,n", sc.z_boxes(), ids=lambda x: "x".join(str(v) for v in x))
def test_z_lines_of_every_length_and_cell_counts_around_a_block(lo, n):
    views = sc.z_views()
    want = sr.observe(sc.V, lo, n, views, 1, sc.M)[:3]
    m = _map()
    for device in (False, True):
        _same(_observe(m, lo, n, views, 1, sc.M, device=device), want, (n, device))
        _same(_observe(m, lo, n, views, 1, sc.M, device=device, fill=0), want, (n, device, "zeros"))
        # in two calls: the second one accumulates
        first = _observe(m, lo, n, views[:1], 1, sc.M, device=device)
        second = _observe(m, lo, n, views[1:], 1, sc.M, before=first[0], device=device)
        assert second[0].tobytes() == want[0].tobytes() and first[1]["votes"] + second[1]["votes"] == want[1]["votes"]
        assert first[1]["newly_known"] + second[1]["newly_known"] == want[1]["newly_known"]
    m.close()


def test_the_three_exact_properties():
    c = sc.cases()["9x7x5 radius 1"]
    lo, n, views = c["lo"], c["n"], c["views"]
    want = sc.spec("9x7x5 radius 1")
    v64 = sc.cases()["64 views"]["views"]
    once = sc.spec("64 views")[0]
    m = _map(sc.records_at([(0, 0, 8), (-4, -3, 6)]))  # a map with voxels in the box: they play no part
    for device in (False, True):
        kw = dict(radius=1, margin=sc.M, device=device)
        # repeated runs and permuted views: the same bytes
        for order in (views, views, views[::-1], views[3:] + views[:3]):
            assert _observe(m, lo, n, order, **kw)[0].tobytes() == want[0].tobytes()
        back = _observe(m, lo, n, views[::-1], **kw)
        assert back[1] == want[1] and back[2] == want[2][::-1]
        # A, then B accumulating, is A and B together
        a = _observe(m, lo, n, views[:3], **kw)
        ab = _observe(m, lo, n, views[3:], before=a[0], **kw)
        assert ab[0].tobytes() == want[0].tobytes()
        # ... saturation included
        twice = _observe(m, lo, n, v64, before=once, **kw)
        thrice = _observe(m, lo, n, v64, before=twice[0], **kw)
        assert thrice[0].tobytes() == (np.minimum(127, 3 * (once & 0x7F).astype(int)).astype(np.uint8) | (once & 0x80)).tobytes()
        assert int((thrice[0] & 0x7F).max()) == 127
        near = np.full(tuple(n), 0x7D, np.uint8)
        full = _observe(m, lo, n, v64[:8], before=near, **kw)
        assert full[0].tobytes() == sr.observe(sc.V, lo, n, v64[:8], 1, sc.M, seen=near)[0].tobytes() and 0x7F in (full[0] & 0x7F)
        assert full[1]["newly_known"] == 0
        # a call that does not accumulate does not read the volume
        assert _observe(m, lo, n, views, fill=0, **kw)[0].tobytes() == _observe(m, lo, n, views, fill=0xFF, **kw)[0].tobytes() == want[0].tobytes()
    m.close()


def test_the_api_the_pyramid_form_and_the_window():
    import torch
    _, cam, pyrs, _ = tr._scene()
    T = tr._kf_poses()
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    m.integrate(pyrs[0], T[0])
    lo, n = (-12, -10, 60), (24, 20, 30)
    plane = pyrs[0].returnDepth(0)
    raw_views = [(plane, T[0], cc.intrinsics320()), (cc.scene_frames()[0][1][1], T[1], cc.intrinsics320())]
    want = mapfile.observe_records(cc.VOXEL, lo, n, raw_views)
    # a pyramid against the same plane passed raw (no intrinsics: the context's)
    v = m.observe([(pyrs[0], T[0]), (raw_views[1][0], T[1])], lo=lo, n=n)
    w = m.observe([(plane, T[0]), (raw_views[1][0], T[1])], lo=lo, n=n)
    assert v.seen.tobytes() == w.seen.tobytes() == want[0].tobytes() and v.info == w.info == want[1] and v.view_info == want[2]
    assert v.lo.tolist() == list(lo) and v.n.tolist() == list(n) and v.voxel == m.voxel and want[1]["cells_free"] > 0
    # into=: a volume accumulates; its box is the call's
    a = m.observe(raw_views[:1], lo=lo, n=n)
    b = m.observe(raw_views[1:], into=a)
    assert b.seen.tobytes() == want[0].tobytes() and a.seen.tobytes() == mapfile.observe_records(cc.VOXEL, lo, n, raw_views[:1])[0].tobytes()
    with pytest.raises(ValueError):
        m.observe(raw_views, lo=lo, n=n, into=a)
    # the default box: the map's bounds grown by pad
    blo, bhi, _ = m.bounds()
    d = m.observe([(pyrs[0], T[0])], pad=1, radius=0, margin=0.03)
    assert d.lo.tolist() == (blo - 1).tolist() and d.n.tolist() == (bhi - blo + 3).tolist()
    # observe_into: pyramids and device tensors only enqueue
    t = torch.full(tuple(n), SENTINEL, dtype=torch.uint8, device="cuda")
    i = torch.zeros(8, dtype=torch.int64, device="cuda")
    dv = [(pyrs[0], T[0]), (torch.from_numpy(raw_views[1][0]).cuda(), T[1])]
    m.observe_into(t, dv, lo, d_info=i, wait=False)
    m.sync()
    assert t.cpu().numpy().tobytes() == want[0].tobytes() and i.cpu().numpy().tolist()[:5] == [want[1][k] for k in mapfile.SEEN_INFO_KEYS]
    m.observe_into(t, dv[:1], lo, accumulate=True)
    assert t.cpu().numpy().tobytes() == mapfile.observe_records(cc.VOXEL, lo, n, raw_views[:1], seen=want[0])[0].tobytes()
    with pytest.raises(ValueError):
        m.observe_into(t.to(torch.int8), dv, lo)
    # the known field and the frontiers through the API, and the whole route's pieces
    rec = m.export_raw()
    f = m.distance_field(seen=v, clamp=90, min_views=2)
    kd2, kinfo = mapfile.known_field_records(rec, lo, n, v.seen, 1, 90, 2)
    assert f.d2.tobytes() == kd2.tobytes() and f.info == kinfo and f.known and f.min_views == 2 and f.clamp == 90
    assert not m.distance_field(lo=lo, n=n).known
    assert m.frontiers(v, 2).tolist() == mapfile.frontier_records(rec, lo, n, v.seen, 1, 2).tolist()
    with pytest.raises(ValueError):
        m.distance_field(lo=lo, n=n, seen=v)
    with pytest.raises(ValueError):
        m.frontiers(api.SeenVolume(v.seen, lo, 2 * m.voxel))
    # MapWindow forwards
    win = api.MapWindow(cam, cc.VOXEL, dense=True, window=2)
    win.integrate(pyrs[0], T[0])
    ws = win.observe([(pyrs[0], T[0]), (raw_views[1][0], T[1])], lo=lo, n=n)
    assert ws.seen.tobytes() == want[0].tobytes()
    assert win.distance_field(seen=ws, clamp=90, min_views=2).d2.tobytes() == kd2.tobytes()
    assert win.frontiers(ws, 2).tolist() == m.frontiers(v, 2).tolist()
    win.close()
    m.close()


@functools.lru_cache(maxsize=None)
def _scene64():
    """The 64^3 box of DESIGN 19's scene, its four views, and mapfile's volume: computed once."""
    lo, n = sc.scene_box(64)
    views = cc.scene_views(False)
    return lo, n, views, mapfile.observe_records(cc.VOXEL, lo, n, views)


def test_the_scene_box():
    lo, n, views, want = _scene64()
    rec = cc.scene_records().astype(RAW)
    m = _map(rec, cc.VOXEL)
    for device, device_in in ((False, False), (True, True)):
        _same(_observe(m, lo, n, views, device=device, device_in=device_in), want, ("scene", device))
    print("scene 64^3:", want[1], want[2])
    seen = want[0]
    kw = mapfile.known_field_records(rec, lo, n, seen)
    for device in (False, True):
        got = _known(m, lo, n, seen, device=device)
        assert got[0].tobytes() == kw[0].tobytes() and got[1] == kw[1], device
    fw = mapfile.frontier_records(rec, lo, n, seen)
    assert _frontiers(m, lo, n, seen).tolist() == fw.tolist() and len(fw) > 0
    dev = _frontiers(m, lo, n, seen, device=True)
    assert sorted(dev.tolist()) == fw.tolist()
    print("scene 64^3: known field", kw[1], "frontier cells", len(fw))
    m.close()


# ------------------------------------------------------------------------------------------------------- the known field --
def _known(m, lo, n, seen, min_count=1, clamp=0, min_views=1, device=False):
    """revo_map_known_field from a host or device volume into sentinel-filled host or device outputs -> (d2, info dict)."""
    import torch
    L = _lib.lib()
    before = m.export_raw().tobytes()
    box, shape = _box(lo, n), tuple(int(x) for x in n)
    seen = np.ascontiguousarray(seen, np.uint8)
    if device:
        s = torch.from_numpy(seen).cuda()
        d = torch.full(shape, 0x07070707, dtype=torch.int32, device="cuda")
        i = torch.full((8,), 9, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.revo_map_known_field(m._h, C.byref(box), min_count, clamp, C.c_void_p(s.data_ptr()), 1, min_views, C.c_void_p(d.data_ptr()), 1,
                                          C.c_void_p(i.data_ptr())))
        m.sync()
        d2, i = d.cpu().numpy().view(np.uint32), i.cpu().numpy().tolist()
    else:
        d2, info = np.full(shape, 0x07070707, np.uint32), MapKnownInfo()
        _lib.check(L.revo_map_known_field(m._h, C.byref(box), min_count, clamp, seen.ctypes.data_as(C.c_void_p), 0, min_views,
                                          d2.ctypes.data_as(C.c_void_p), 0, C.byref(info)))
        i = [int(getattr(info, k)) for k, _ in MapKnownInfo._fields_]
    assert i[7] == 0 and m.export_raw().tobytes() == before
    return d2, dict(zip(mapfile.KNOWN_INFO_KEYS, i[:7]))


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_known_field_bit_exact(seed):
    c = sc.random_volume(seed)
    rec = c["rec"].astype(RAW)
    m = _map(rec)
    for min_count, clamp, min_views in ((1, 0, 1), (2, 40, 2), (1, 0, 200), (1, 0, 0)):
        want = mapfile.known_field_records(rec, c["lo"], c["n"], c["seen"], min_count, clamp, min_views)
        for device in (False, True):
            got = _known(m, c["lo"], c["n"], c["seen"], min_count, clamp, min_views, device)
            assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], (min_count, clamp, min_views, device)
    if seed == 1:
        assert want[0].tobytes() == sr.known_field(c["rec"], c["lo"], c["n"], c["seen"], 1, 0, 0)[0].tobytes()
    m.close()


def test_degenerate_fields_and_the_plain_field():
    import torch
    lo, n = (-3, 2, 1), (6, 5, 33)
    rec = sc.records_at([(-2, 3, 2), (1, 5, 30), (40, 0, 0)]).astype(RAW)
    m = _map(rec)
    nothing, all_seen = np.zeros(n, np.uint8), np.full(n, 0x7F, np.uint8)
    for device in (False, True):
        d2, info = _known(m, lo, n, nothing, device=device)
        assert not d2.any() and info == mapfile.known_field_records(rec, lo, n, nothing)[1] and info["unknown"] == info["cells"] - 2
        d2, info = _known(m, lo, n, all_seen, clamp=7, device=device)
        plain = tr_field(m, lo, n, 7)
        assert d2.tobytes() == plain[0].tobytes() and [info[k] for k in mapfile.DF_INFO_KEYS] == plain[1] and info["unknown"] == 0
        assert info["known_free"] == info["cells"] - 2
    empty = _map()
    for device in (False, True):
        d2, info = _known(empty, lo, n, np.full(n, 0x80, np.uint8), device=device)
        assert np.all(d2 == DF_NONE) and info["unknown"] == 0 and info["known_free"] == info["cells"] and info["max_d2"] == 0
    # the field goes straight into plan_into on the device
    c = sc.random_volume(2)
    rec = c["rec"].astype(RAW)
    m2 = _map(rec)
    shape = tuple(int(x) for x in c["n"])
    s, d = torch.from_numpy(c["seen"]).cuda(), torch.zeros(shape, dtype=torch.int32, device="cuda")
    cost, pi = torch.zeros(shape, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
    m2.known_field_into(d, s, c["lo"], c["n"], wait=False)
    goals = mapfile.frontier_records(rec, c["lo"], c["n"], c["seen"])
    m2.plan_into(cost, d, c["lo"], c["n"], goals, 1, d_info=pi)
    want_d2 = mapfile.known_field_records(rec, c["lo"], c["n"], c["seen"])[0]
    want_cost, want_info = mapfile.plan_records(want_d2, c["lo"], c["n"], mapfile.plan_seeds(goals), 1)
    assert cost.cpu().numpy().view(np.uint32).tobytes() == want_cost.tobytes()
    assert pi.cpu().numpy().tolist()[:7] == [want_info[k] for k in mapfile.PLAN_INFO_KEYS] and want_info["seeds_used"] == len(goals) > 0
    for x in (m, empty, m2):
        x.close()


def tr_field(m, lo, n, clamp):
    """revo_map_distance_field's bytes and its five counters."""
    f = m.distance_field(lo=lo, n=n, clamp=clamp)
    return f.d2, [f.info[k] for k in mapfile.DF_INFO_KEYS]


# ------------------------------------------------------------------------------------------------------------ frontiers --
def _frontiers(m, lo, n, seen, min_count=1, min_views=1, device=False, cap=None, count_only=False):
    """revo_map_frontiers -> the cells [k, 3] (count_only: k); device: a device volume and device records."""
    import torch
    L = _lib.lib()
    box, k = _box(lo, n), C.c_size_t(77)
    seen = np.ascontiguousarray(seen, np.uint8)
    s = torch.from_numpy(seen).cuda() if device else None
    sp = C.c_void_p(s.data_ptr()) if device else seen.ctypes.data_as(C.c_void_p)
    torch.cuda.synchronize()
    _lib.check(L.revo_map_frontiers(m._h, C.byref(box), min_count, sp, int(device), min_views, None, 0, C.byref(k), int(device)))
    if count_only:
        return k.value
    cap = k.value if cap is None else cap
    if device:
        out = torch.full((max(cap, 1), 4), 0x55, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = L.revo_map_frontiers(m._h, C.byref(box), min_count, sp, 1, min_views, C.c_void_p(out.data_ptr()), cap, C.byref(k), 1)
        rec = out.cpu().numpy()
    else:
        rec = np.full((max(cap, 1), 4), 0x55, np.int32)
        rc = L.revo_map_frontiers(m._h, C.byref(box), min_count, sp, 0, min_views, rec.ctypes.data_as(C.c_void_p), cap, C.byref(k), 0)
    if rc == CAPACITY:
        assert np.all(rec == 0x55) and k.value > cap  # nothing written, and the count it needs
        return None
    _lib.check(rc)
    assert not rec[:k.value, 3].any() and np.all(rec[k.value:] == 0x55)
    return rec[:k.value, :3]


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_frontiers(seed):
    c = sc.random_volume(seed)
    rec = c["rec"].astype(RAW)
    m = _map(rec)
    for min_count, min_views in ((1, 1), (2, 2), (1, 200)):
        want = mapfile.frontier_records(rec, c["lo"], c["n"], c["seen"], min_count, min_views)
        args = (m, c["lo"], c["n"], c["seen"], min_count, min_views)
        host, dev = _frontiers(*args), _frontiers(*args, device=True)
        assert host.tolist() == want.tolist() and sorted(dev.tolist()) == want.tolist()
        assert _frontiers(*args, count_only=True) == _frontiers(*args, device=True, count_only=True) == len(want)
        if len(want):
            for device in (False, True):
                assert _frontiers(*args, device=device, cap=len(want) - 1) is None
                assert len(_frontiers(*args, device=device, cap=len(want) + 3)) == len(want)
    # the records are seeds as they are
    want = mapfile.frontier_records(rec, c["lo"], c["n"], c["seen"])
    seeds = np.zeros(len(want), SEED)
    seeds["cell"] = _frontiers(m, c["lo"], c["n"], c["seen"])
    assert seeds.itemsize == C.sizeof(MapPlanSeed)
    d2 = mapfile.known_field_records(rec, c["lo"], c["n"], c["seen"])[0]
    cost, info = np.empty(d2.shape, np.uint32), MapPlanInfo()
    box = _box(c["lo"], c["n"])
    _lib.check(_lib.lib().revo_map_plan(m._h, C.byref(box), d2.ctypes.data_as(C.c_void_p), 0, 1, len(seeds), seeds.ctypes.data_as(C.c_void_p), 0,
                                        cost.ctypes.data_as(C.c_void_p), 0, C.byref(info)))
    assert info.seeds_used == len(want) and info.seeds_blocked == 0
    assert cost.tobytes() == mapfile.plan_records(d2, c["lo"], c["n"], mapfile.plan_seeds(want), 1)[0].tobytes()
    m.close()


def test_frontier_rules_on_the_device():
    lo, n = (10, -2, 0), (4, 3, 3)
    m, solid = _map(), _map(sc.records_at([(11, -1, 1)]))
    seen = np.full(n, 1, np.uint8)
    assert _frontiers(m, lo, n, seen, count_only=True) == 0  # all free: the faces of the box are no frontier
    seen[1, 1, 1] = 0
    assert len(_frontiers(m, lo, n, seen)) == 6 and _frontiers(solid, lo, n, seen, count_only=True) == 0
    assert _frontiers(solid, lo, n, seen, min_count=2, count_only=True) == 6
    seen[1, 1, 1] = 0x80
    assert _frontiers(m, lo, n, seen, count_only=True) == 0  # a surface bit is known
    seen[0, 0, 0], seen[0, 0, 1], seen[2, 1, 1], seen[3, 1, 1] = 0, 2, 0x82, 0
    for mm in (m, solid):
        rec = mm.export_raw()
        assert _frontiers(mm, lo, n, seen).tolist() == mapfile.frontier_records(rec, lo, n, seen).tolist()
    m.close()
    solid.close()


# -------------------------------------------------------------------------------------------------------------- arguments --
def test_argument_errors_write_nothing():
    import torch
    L = _lib.lib()
    rec = sc.records_at([(1, 1, 1), (2, 3, 1)]).astype(RAW)
    m = _map(rec)
    before = m.export_raw().tobytes()
    lo, n = (0, 0, 0), (4, 3, 5)
    good = _box(lo, n)
    t = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    base = t.data_ptr()
    dp = lambda off: C.c_void_p(base + off)  # noqa: E731
    depth = np.full((12, 16), 2.0, F)
    cv, _, keep = m._carve_views([(depth, sc.I4, sc.KC)])
    prm = MapObserveParams(1, 0, 0.1, 0.0)
    seen = np.full(60, SENTINEL, np.uint8)
    info, vinfo = np.full(8, 9, np.uint64), np.full(8, 9, np.uint32)
    sp, ip, vp_ = (x.ctypes.data_as(C.c_void_p) for x in (seen, info, vinfo))
    R = 1 << 20
    bad_boxes = [_box((0, 0, 0), (0, 3, 5)), _box((0, 0, 0), (4, -1, 5)), _box((0, 0, 0), (4, 3, 1025)), _box((0, 0, 0), (1024, 1024, 129)),
                 _box((-R - 1, 0, 0), (4, 3, 5)), _box((0, 0, R - 5), (4, 3, 6))]

    def obs(box=good, nv=1, views=cv, din=0, p=prm, s=sp, dev=0, i=ip, vi=vp_, mm=m):
        return L.revo_map_observe(mm._h if mm is not None else None, C.byref(box) if box is not None else None, nv, views, din,
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
    bad_params = [MapObserveParams(4, 0, 0.1, 0.0), MapObserveParams(-1, 0, 0.1, 0.0), MapObserveParams(1, 2, 0.1, 0.0),
                  MapObserveParams(1, 0, -0.1, 0.0), MapObserveParams(1, 0, float("nan"), 0.0), MapObserveParams(1, 0, float("inf"), 0.0),
                  MapObserveParams(1, 0, 0.1, -1.0), MapObserveParams(1, 0, 0.1, float("inf"))]
    for j, b in enumerate(bad_boxes):
        assert obs(b) == INVALID_ARG and L.revo_last_error(), j
    for j, v in enumerate(bad_views):
        assert obs(views=v) == INVALID_ARG, j
    for j, p in enumerate(bad_params):
        assert obs(p=p) == INVALID_ARG, j
    assert [obs(mm=None), obs(box=None), obs(views=None), obs(s=None), obs(nv=0), obs(nv=65), obs(nv=-1), obs(din=2), obs(dev=2), obs(dev=-1),
            obs(s=dp(4), dev=1, i=None, vi=None), obs(s=dp(0), dev=1, i=dp(1024 + 8), vi=None), obs(s=dp(0), dev=1, i=None, vi=dp(2048 + 4)),
            obs(views=view(depth=base + 4096 + 2), din=1)] == [INVALID_ARG] * 14
    # revo_map_known_field
    d2 = np.full(60, 0x07070707, np.uint32)
    op = d2.ctypes.data_as(C.c_void_p)

    def known(box=good, s=sp, ds=0, o=op, do=0, i=ip, mm=m):
        return L.revo_map_known_field(mm._h if mm is not None else None, C.byref(box) if box is not None else None, 1, 0, s, ds, 1, o, do, i)

    for j, b in enumerate(bad_boxes):
        assert known(b) == INVALID_ARG, j
    assert [known(mm=None), known(box=None), known(s=None), known(o=None), known(ds=2), known(do=-1), known(s=dp(8), ds=1),
            known(o=dp(4), do=1, i=None), known(o=dp(0), do=1, i=dp(1024 + 8))] == [INVALID_ARG] * 9
    # revo_map_frontiers
    cells = np.full(4 * 60, 0x55, np.int32)
    cp, k = cells.ctypes.data_as(C.c_void_p), C.c_size_t(77)

    def fr(box=good, s=sp, ds=0, o=cp, cap=60, kk=k, do=0, mm=m):
        return L.revo_map_frontiers(mm._h if mm is not None else None, C.byref(box) if box is not None else None, 1, s, ds, 1, o, cap,
                                    C.byref(kk) if kk is not None else None, do)

    for j, b in enumerate(bad_boxes):
        assert fr(b) == INVALID_ARG, j
    assert [fr(mm=None), fr(box=None), fr(s=None), fr(kk=None), fr(ds=2), fr(do=2), fr(s=dp(8), ds=1), fr(o=dp(8), do=1)] == [INVALID_ARG] * 8
    m.sync()
    assert np.all(seen == SENTINEL) and np.all(info == 9) and np.all(vinfo == 9) and np.all(d2 == 0x07070707) and np.all(cells == 0x55) and k.value == 77
    assert not t.cpu().numpy().any() and m.export_raw().tobytes() == before
    # the handle is as usable as before (a fault would make info() fail); info and view_info may be NULL
    assert m.info()["voxels"] == 2
    assert obs() == 0 and obs(i=None, vi=None) == 0
    want = mapfile.observe_records(sc.V, lo, n, [(depth, sc.I4, sc.KC)], 1, 0.1)
    assert seen.reshape(n).tobytes() == want[0].tobytes() and info.tolist()[:5] == [want[1][x] for x in mapfile.SEEN_INFO_KEYS]
    assert known() == 0 and fr() == 0
    assert d2.reshape(n).tobytes() == mapfile.known_field_records(rec, lo, n, want[0])[0].tobytes()
    assert cells.reshape(-1, 4)[:k.value, :3].tolist() == mapfile.frontier_records(rec, lo, n, want[0]).tolist()
    del keep
    m.close()


# --------------------------------------------------------------------------------------------------------------- the route --
def test_the_route_on_the_device():
    w = sc.wall_scene()
    rec, lo, n = w["rec"].astype(RAW), w["lo"], w["n"]
    m = _map(rec)
    seen = m.observe(w["views"], lo=lo, n=n)
    want = mapfile.observe_records(sc.V, lo, n, w["views"])
    assert seen.seen.tobytes() == want[0].tobytes() and seen.info == want[1] and seen.view_info == want[2]
    # the plain field lets the goal behind the wall be reached; the known field blocks it
    plain = m.distance_field(lo=lo, n=n).plan([w["goal"]], clearance=sc.V)
    cells, status, _ = plain.path([w["start"]])[0]
    assert status == mapfile.PLAN_REACHED and cells[-1].tolist() == list(w["goal"]) and plain.info["seeds_used"] == 1
    known = m.distance_field(seen=seen)
    blocked = known.plan([w["goal"]], clearance=sc.V)
    assert blocked.info["seeds_blocked"] == 1 and blocked.info["reachable"] == 0
    # explore: the same bytes as the restatement, and a path to a frontier through known free cells
    r = api.explore(m, seen, w["start"], sc.V)
    d2, fr, cost, info, (wcells, wstatus, wcost) = mapfile.explore_records(rec, lo, n, sc.V, want[0], w["start"], sc.V)
    assert r["field"].d2.tobytes() == d2.tobytes() and r["frontiers"].tolist() == fr.tolist() and r["cost"].cost.tobytes() == cost.tobytes()
    cells, status, c0 = r["path"]
    assert cells.tolist() == wcells.tolist() and (status, c0) == (wstatus, wcost) == (mapfile.PLAN_REACHED, c0) and c0 > 0
    assert cells[-1].tolist() in fr.tolist()
    at = tuple((cells - np.asarray(lo)).T)
    assert seen.free()[at].all() and np.all(d2[at] >= 1)
    with pytest.raises(ValueError):
        api.explore(m, api.SeenVolume(np.full(n, 1, np.uint8), lo, sc.V), w["start"], sc.V)
    with pytest.raises(ValueError):
        api.explore(m, seen, w["start"], 3 * sc.V)  # a frontier cell has d2 = 1: none keeps three cells
    m.close()
