"""Free-space carving on the device (revo_map_carve_eval / revo_map_carve, api.VoxelMap.carve_eval / carve, vo.REVO's carve;
DESIGN 19): the carved records, the info record and the per-view class counts bit for bit the specification's -- the per-voxel
loop of tests/map_carve_ref.py on the hand-made voxels, its vectorised twin revo_amd.mapfile.carve_records (which
test_map_carve_cpu.py pins to the loop) on the 35 000-voxel scene -- from the host and from the device output, whatever the
table size, the integration order and the split of the views over calls; the map after a carve byte for byte and counter for
counter, and the way back; the pyramid form against the depth plane the pyramid holds; every argument error one device can
show; and the driver's carve replayed through the specification."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile, synth  # noqa: E402
from revo_amd._lib import RevoError  # noqa: E402
from revo_amd.settings import MapCarveInfo, MapCarveParams, MapCarveView, MapCarveViewInfo  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_carve_ref as mc  # noqa: E402
import map_records_ref as mrr  # noqa: E402
import voxel_map_ref as ref  # noqa: E402

F = np.float32
RAW = mapfile.RAW_DTYPE
INVALID_ARG, CAPACITY = -1, -5
I4 = cc.I4
VOXEL = cc.VOXEL
COUNTERS = ("voxels", "points_integrated", "points_dropped", "keyframes", "keyframes_rejected")
VIEW16 = (cc.depth16(), I4, cc.K16)
SCENE_KW = dict(radius=1, margin=0.02, margin_rel=0.0)


@functools.lru_cache(maxsize=None)
def _scene():
    """The context, the pyramids of views 0 and 1 of the scene as built, and their dense level-0 clouds."""
    from revo_amd import api
    s = cc.settings320()
    cam = api.CameraPyr(s)
    pyrs = [api.ImgPyramidRGBD(s, cam, *cc.scene_frames()[0][i]) for i in (0, 1)]
    clouds = [ref.points_from_pcl(p.generateColoredPcl(0, True)) for p in pyrs]
    return api, cam, pyrs, clouds


def _kf_poses():
    return [T.astype(F) for T in cc.poses()[:2]]


@functools.lru_cache(maxsize=None)
def _scene_records():
    r = ref.VoxelMapRef(VOXEL)
    for (xyz, rgb), T in zip(_scene()[3], _kf_poses()):
        r.integrate(xyz, rgb, T)
    return mrr.records_of(r).astype(RAW)


@functools.lru_cache(maxsize=None)
def _scene_spec(min_views=1):
    """The specification on the scene map with the four changed views, computed once."""
    return mapfile.carve_records(_scene_records(), VOXEL, cc.scene_views(True), min_views=min_views, **SCENE_KW)


def _build(order=(0, 1), **kw):
    api, cam, pyrs, _ = _scene()
    m = api.VoxelMap(cam, VOXEL, dense=True, **kw)
    for i in order:
        m.integrate(pyrs[i], _kf_poses()[i])
    return m


def _hand(rec, **kw):
    api, cam = _scene()[:2]
    m = api.VoxelMap(cam, VOXEL, **kw)
    m.merge_raw(rec.astype(RAW))
    return m


def _counters(m):
    i = m.info()
    return {k: i[k] for k in COUNTERS}


def _sorted(t):
    r = t.cpu().numpy().view(RAW)
    return r[np.argsort(r["key"])]


def _check_eval(m, rec, views, **kw):
    """carve_eval from the host and from the device against the specification's loop; the map stays as it was."""
    want, winfo, wcounts, _ = mc.carve_eval(rec, VOXEL, views, **kw)
    before = m.export_raw().tobytes(), m.info()
    got, ginfo, gcounts = m.carve_eval(views, **kw)
    dev, dinfo, dcounts = m.carve_eval(views, device=True, **kw)
    print("%d views, %s: %s %s" % (len(views), kw, winfo, wcounts))
    assert ginfo == winfo == dinfo and gcounts == wcounts == dcounts
    assert got.dtype == RAW and got.tobytes() == want.astype(RAW).tobytes()
    assert dev.numel() == 64 * len(want) and _sorted(dev).tobytes() == want.astype(RAW).tobytes()
    assert (m.export_raw().tobytes(), m.info()) == before
    return want, winfo


@pytest.mark.parametrize("initial_voxels", [1, 1 << 16], ids=["1024 slots", "default table"])
def test_carve_eval_hand_made_bit_exact(initial_voxels):
    rec = cc.filled_records()
    m = _hand(rec, initial_voxels=initial_voxels)
    if initial_voxels == 1:
        assert m.info()["capacity"] == 1024
        assert len(np.unique(cc.map_hash(rec["key"]) & np.uint64(1023))) < len(rec) - 50  # keys that share slots
    else:
        assert m.info()["capacity"] >= 1 << 17
    assert m.export_raw().tobytes() == rec.astype(RAW).tobytes()
    carved = [_check_eval(m, rec, [VIEW16], radius=r, margin=cc.M)[1]["voxels_carved"] for r in range(4)]
    assert carved[0] > carved[1] > carved[2] > carved[3] > 0
    views = cc.three_views() + [cc.random_case(5, 12, 16, cc.K16)[1]]
    for mv in (1, 2, 3):
        _check_eval(m, rec, views, margin=cc.M, min_views=mv)
    _check_eval(m, rec, views, margin=0.0, margin_rel=2.0 ** -5, min_count=2, max_count=4)
    _check_eval(m, rec, [VIEW16], margin=None)
    # the class cases alone, one voxel per rule
    crec, where, expect = cc.class_records()
    want, info = _check_eval(_hand(crec, initial_voxels=initial_voxels), crec, [VIEW16], margin=cc.M)
    assert want["key"].tolist() == sorted(int(crec["key"][i]) for n, i in where.items() if expect[n] == "free")
    # an 8 x 8 view, and an empty map
    rr, view = cc.random_case(0, 8, 8, cc.K8)
    _check_eval(_hand(rr, initial_voxels=initial_voxels), rr, [view], margin=0.05, margin_rel=0.01)
    api, cam = _scene()[:2]
    empty = api.VoxelMap(cam, VOXEL, initial_voxels=initial_voxels)
    got, info, counts = empty.carve_eval([VIEW16])
    assert len(got) == 0 and info == dict.fromkeys(mc.INFO_KEYS, 0) and counts == [dict.fromkeys(mc.CLASSES, 0)]
    assert empty.carve([VIEW16], device=True)[0].numel() == 0 and empty.info()["voxels"] == 0


@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["kf0 first", "kf1 first"])
def test_scene_bit_exact_and_in_parts(order):
    import torch
    sr = _scene_records()
    m = _build(order)
    assert m.export_raw().tobytes() == sr.tobytes()
    views = cc.scene_views(True)
    for mv in (1, 2):
        want, winfo, wcounts = _scene_spec(mv)
        got, ginfo, gcounts = m.carve_eval(views, min_views=mv, **SCENE_KW)
        assert got.tobytes() == want.tobytes() and ginfo == winfo and gcounts == wcounts
    want, winfo, wcounts = _scene_spec(1)
    ghost = cc.ghost_mask(sr)
    is_ghost = np.isin(want["key"], sr["key"][ghost])
    print("scene: %d voxels, %d ghost; carved %d ghost, %d others; %s" % (len(sr), ghost.sum(), is_ghost.sum(), (~is_ghost).sum(), wcounts))
    assert len(sr) > 30000 and (~is_ghost).sum() == 0 and is_ghost.sum() >= 0.9 * ghost.sum()
    # the same views as device tensors, the records on the device
    dviews = [(torch.from_numpy(np.ascontiguousarray(D)).cuda(), T, k) for D, T, k in views]
    dev, dinfo, dcounts = m.carve_eval(dviews, device=True, **SCENE_KW)
    assert _sorted(dev).tobytes() == want.tobytes() and dinfo == winfo and dcounts == wcounts
    assert m.export_raw().tobytes() == sr.tobytes()
    # one call of four views against two calls of two
    left = mapfile.subtract_records(sr, want)
    two = _build(order)
    ga, ia, _ = two.carve(views[:2], **SCENE_KW)
    gb, ib, _ = two.carve(views[2:], **SCENE_KW)
    assert len(ga) and len(gb) and two.export_raw().tobytes() == left.tobytes()
    assert mapfile.merge_records(ga, gb).tobytes() == want.tobytes()
    gone, info, counts = m.carve(views, **SCENE_KW)
    assert gone.tobytes() == want.tobytes() and info == winfo and counts == wcounts
    assert m.export_raw().tobytes() == left.tobytes() and _counters(m) == _counters(two)
    # the unchanged scene carves nothing
    assert m.carve(cc.scene_views(False), **SCENE_KW)[1]["voxels_carved"] == 0 and m.export_raw().tobytes() == left.tobytes()


def test_carve_changes_the_map_as_the_contract_says():
    api, cam = _scene()[:2]
    sr = _scene_records()
    views = cc.scene_views(True)
    want, winfo, _ = _scene_spec(1)
    m = _build()
    before = _counters(m)
    assert before["keyframes"] == 2
    gone, info, _ = m.carve(views, **SCENE_KW)
    left = mapfile.subtract_records(sr, want)
    assert gone.tobytes() == want.tobytes() and m.export_raw().tobytes() == left.tobytes() == mc.remaining(sr, want).tobytes()
    after = _counters(m)  # reading them also says the fault word is clear
    assert after == dict(mc.counters_after(before, winfo), keyframes_rejected=0)
    assert after["voxels"] == len(left) and after["points_integrated"] == int(left["count"].sum())
    assert (after["keyframes"], after["points_dropped"]) == (before["keyframes"], before["points_dropped"])
    # a second carve removes nothing
    again, info2, _ = m.carve(views, **SCENE_KW)
    assert len(again) == 0 and info2["voxels_carved"] == 0 and info2["voxels_considered"] == len(left)
    assert m.export_raw().tobytes() == left.tobytes() and _counters(m) == after
    # the map still renders and merges: the ghost is gone from the view, and a merge into a fresh map gives the same records
    depth, bgr, covered = m.render(cc.poses()[2].astype(F))
    full = _build()
    d0, _, c0 = full.render(cc.poses()[2].astype(F))
    assert covered > 0 and c0 > 0 and depth.shape == d0.shape and not np.array_equal(depth, d0)
    other = api.VoxelMap(cam, VOXEL, dense=True)
    other.merge(m)
    assert other.export_raw().tobytes() == left.tobytes()
    # merging the removed records restores the map byte for byte, counters included
    m.merge_raw(gone)
    assert m.export_raw().tobytes() == sr.tobytes() and _counters(m) == before
    # the device output of carve
    dev, dinfo, _ = m.carve(views, device=True, **SCENE_KW)
    assert _sorted(dev).tobytes() == want.tobytes() and dinfo == winfo and m.export_raw().tobytes() == left.tobytes()
    m.merge_raw(dev)
    assert m.export_raw().tobytes() == sr.tobytes() and _counters(m) == before


@pytest.mark.parametrize("n", [255, 256, 257])
def test_record_counts_around_the_block_size(n):
    rec = cc.free_grid(n)
    view = (cc.depth64(), I4, cc.K64)
    # the free voxels among voxels that stay: behind the image's surface
    stay = cc.free_grid(40, z=2.5)
    both = mapfile.merge_records(rec.astype(RAW), stay.astype(RAW))
    m = _hand(both, initial_voxels=1)
    want, winfo = _check_eval(m, both, [view], margin=cc.M)
    assert winfo["voxels_carved"] == n and winfo["voxels_considered"] == n + 40 and want.tobytes() == rec.astype(RAW).tobytes()
    gone, info, counts = m.carve([view], margin=cc.M)
    assert gone.tobytes() == rec.astype(RAW).tobytes() and counts == [dict(outside=0, unknown=0, free=n, confirmed=0, occluded=40, edge=0)]
    assert m.export_raw().tobytes() == stay.astype(RAW).tobytes() and m.info()["voxels"] == 40


def test_the_pyramid_form():
    api, cam = _scene()[:2]
    s = cc.settings320()
    sr = _scene_records()
    m = _build()
    for i in (2, 3):
        bgr, depth = cc.scene_frames()[1][i]
        pyr = api.ImgPyramidRGBD(s, cam, bgr, depth)
        pyr.makeKeyframe()
        T = cc.poses()[i].astype(F)
        plane = np.array(pyr.returnDepth(0), F).reshape(s.height, s.width)  # what the pyramid holds, read back
        want, winfo, wcounts = mapfile.carve_records(sr, VOXEL, [(plane, T, cc.intrinsics320())], **SCENE_KW)
        a = m.carve_eval([(pyr, T)], **SCENE_KW)
        b = m.carve_eval([(plane, T)], **SCENE_KW)                         # no intrinsics: the context's
        c = m.carve_eval([(plane, T, cc.intrinsics320())], **SCENE_KW)
        assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() == want.tobytes() and a[1] == b[1] == c[1] == winfo
        assert a[2] == b[2] == c[2] == wcounts and winfo["voxels_carved"] > 300
    # a pyramid and a raw image in one call
    both, info, counts = m.carve_eval([(pyr, T), (cc.scene_frames()[1][2][1], cc.poses()[2].astype(F))], **SCENE_KW)
    assert len(counts) == 2 and counts[:1] == wcounts and info["voxels_carved"] >= winfo["voxels_carved"]


def test_argument_errors():
    import torch
    from revo_amd import _lib
    api, cam = _scene()[:2]
    L = _lib.lib()
    s = cc.settings320()
    m = _build()
    sr = _scene_records()
    D = np.ascontiguousarray(cc.scene_frames()[1][2][1])
    T = cc.poses()[2].astype(F)
    pyr = _scene()[2][0]
    other_cam = api.CameraPyr(s)
    foreign = api.ImgPyramidRGBD(s, other_cam, *cc.scene_frames()[0][0])
    # a batch view of the map's own context: frame 0 of a one-pair batch
    from revo_amd.settings import TrackerSettings
    api.TrackerNew(TrackerSettings(), s, cam)
    f0, f1 = cc.scene_frames()[0][:2]
    d_bgr = torch.from_numpy(np.stack([f0[0], f1[0]])).cuda()
    d_dep = torch.from_numpy(np.stack([f0[1], f1[1]]).astype(F)).cuda()
    torch.cuda.synchronize()
    batch = api.BatchTracker(cam, 1)
    batch.build(d_bgr.data_ptr(), d_dep.data_ptr())
    batch.sync()
    batch_view = batch.frame(0, s)

    def view(depth=D, kf=None, w=s.width, h=s.height, k=(0.0,) * 6, pose=T):
        v = MapCarveView()
        v.kf = kf._h if kf is not None else None
        v.depth = depth.ctypes.data if depth is not None else None
        v.width, v.height = w, h
        v.fx, v.fy, v.cx, v.cy, v.zmin, v.zmax = k
        v.T_w_c[:] = np.ascontiguousarray(np.asarray(pose, F).T).reshape(16).tolist()
        return v

    def call(fn, views, prm=None, n=None, records=None, cap=0, n_out=True, device_in=0, device_out=0, m_=m):
        arr = (MapCarveView * max(1, len(views)))(*views)
        nr = C.c_size_t()
        return fn(m_._h if m_ is not None else None, len(views) if n is None else n, arr if views else None, device_in,
                  C.byref(prm) if prm is not None else None, records, cap, C.byref(nr) if n_out else None, device_out, None, None)

    own = list(cc.intrinsics320())
    skew, nan = np.eye(4, dtype=F), np.eye(4, dtype=F)
    skew[0, 1] = 0.01
    nan[1, 3] = np.nan
    bad_views = [view(kf=pyr), view(depth=None), view(kf=foreign, depth=None), view(kf=batch_view, depth=None), view(w=0), view(h=2049), view(w=-1),
                 view(k=[0.0] + own[1:]), view(k=own[:1] + [-1.0] + own[2:]), view(k=own[:2] + [np.inf] + own[3:]),
                 view(k=own[:4] + [-0.1, 5.0]), view(k=own[:4] + [3.0, 3.0]), view(k=own[:4] + [np.nan, 5.0]),
                 view(pose=skew), view(pose=nan), view(pose=np.diag(F([1, 1, -1, 1])))]
    good = view()
    P = MapCarveParams
    bad_params = [P(-1, 1, 1, 0, 0.02, 0.0), P(4, 1, 1, 0, 0.02, 0.0), P(1, 1, 1, 0, -0.02, 0.0), P(1, 1, 1, 0, float("nan"), 0.0),
                  P(1, 1, 1, 0, float("inf"), 0.0), P(1, 1, 1, 0, 0.02, -0.5), P(1, 1, 1, 0, 0.02, float("nan"))]
    buf = torch.full((64 * 4096,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = m.export_raw().tobytes(), m.info()
    for fn in (L.revo_map_carve_eval, L.revo_map_carve):
        for v in bad_views:
            assert call(fn, [v]) == INVALID_ARG
            assert call(fn, [good, v]) == INVALID_ARG
            assert call(fn, [view(kf=pyr, depth=None), v]) == INVALID_ARG  # behind a good pyramid view too
        assert (m.export_raw().tobytes(), m.info()) == before
        for p in bad_params:
            assert call(fn, [good], prm=p) == INVALID_ARG
        assert call(fn, [good], m_=None) == INVALID_ARG
        assert call(fn, []) == INVALID_ARG and call(fn, [good], n=0) == INVALID_ARG and call(fn, [good] * 65) == INVALID_ARG
        assert call(fn, [good], n_out=False) == INVALID_ARG
        assert call(fn, [good], device_in=2) == INVALID_ARG and call(fn, [good], device_out=2) == INVALID_ARG
        assert call(fn, [good], records=C.c_void_p(buf.data_ptr() + 8), cap=4095, device_out=1) == INVALID_ARG  # misaligned records
        dd = torch.from_numpy(D).cuda()
        dv = view()
        dv.depth = dd.data_ptr() + 2
        assert call(fn, [dv], device_in=1) == INVALID_ARG                                                     # misaligned image
        # outputs that are too small: nothing is written and nothing removed
        assert call(fn, [good], records=C.c_void_p(buf.data_ptr()), cap=10, device_out=1) == CAPACITY
        host = np.full(64 * 10, 0xAB, np.uint8)
        assert call(fn, [good], records=host.ctypes.data_as(C.c_void_p), cap=10) == CAPACITY
        m.sync()
        assert bool((buf == 0xAB).all()) and bool((host == 0xAB).all())
        assert (m.export_raw().tobytes(), m.info()) == before
    # 64 views are accepted, counting only
    nr, info = C.c_size_t(), MapCarveInfo()
    arr = (MapCarveView * 64)(*[good] * 64)
    vinfo = (MapCarveViewInfo * 64)()
    assert L.revo_map_carve_eval(m._h, 64, arr, 0, None, None, 0, C.byref(nr), 0, C.byref(info), vinfo) == 0
    w1 = mapfile.carve_records(sr, VOXEL, [(D, T, cc.intrinsics320())])  # NULL parameters: radius 1, the voxel edge
    assert nr.value == info.voxels_carved == w1[1]["voxels_carved"] and info.votes == 64 * w1[1]["votes"]
    assert all(v.free_space == w1[2][0]["free"] and v.unknown == w1[2][0]["unknown"] for v in vinfo)
    assert (m.export_raw().tobytes(), m.info()) == before
    with pytest.raises(ValueError):
        m.carve_eval([])
    with pytest.raises(RevoError) as e:
        m.carve_eval([(D, skew)])
    assert e.value.code == INVALID_ARG


def test_map_window_cannot_be_carved():
    api, cam = _scene()[:2]
    w = api.MapWindow(cam, VOXEL, dense=True, window=2)
    with pytest.raises(NotImplementedError):
        w.carve([VIEW16])
    from revo_amd import vo
    with pytest.raises(ValueError):
        vo.REVO(cc.settings320(), cameraPyr=cam, voxelMap=w, carve=True)
    with pytest.raises(ValueError):
        vo.REVO(cc.settings320(), cameraPyr=cam, carve=True)
    w.close()


def test_revo_carves_before_it_integrates():
    from revo_amd import api, ply, vo
    s = cc.settings320()
    frames = synth.make_sequence(951, s, 40, max_t=0.01, max_rot_deg=0.4, bias=[0, 0, 0, 0, np.deg2rad(1.5), 0])
    prm = dict(radius=0, margin=0.01)  # no window, a tight margin: mixed-depth points at occlusion edges get carved
    runs = []
    for carve in (None, prm):
        cam = api.CameraPyr(s)
        drawer = ply.ModelExporter()
        vm = api.VoxelMap(cam, VOXEL, dense=True)
        g = vo.REVO(s, cameraPyr=cam, mapDrawer=drawer, generate_dense_pcl=True, voxelMap=vm, carve=carve)
        planes = []
        for f in frames:
            _, kf = g.push(f[0], f[1], f[2])
            if kf:
                planes.append(np.array(g.keyframe()[0].returnDepth(0), F).reshape(s.height, s.width))
        runs.append((g, vm, drawer, planes))
    (g0, vm0, _, _), (g, vm, drawer, planes) = runs
    assert [t for t, _ in g.poses] == [t for t, _ in g0.poses]
    assert all(a.tobytes() == b.tobytes() for (_, a), (_, b) in zip(g.poses, g0.poses))  # the poses do not depend on the map
    assert g.nKeyFrames == g0.nKeyFrames == len(planes) == len(g.carves) >= 3 and g0.carves == []
    rec = np.zeros(0, RAW)
    carved = points = 0
    for plane, pcl, T, (ts, Tc, info) in zip(planes, drawer.pclKfHost, drawer.vpKfsF, g.carves):
        T = np.asarray(T, F)
        assert Tc.tobytes() == T.tobytes()
        assert (info is not None) == mapfile.pose_is_orthogonal(T[:3, :3])
        if info is not None and len(rec):
            gone, winfo, _ = mapfile.carve_records(rec, VOXEL, [(plane, T, cc.intrinsics320())], **prm)
            assert info == winfo
            rec = mapfile.subtract_records(rec, gone)
            carved += len(gone)
            points += winfo["points_carved"]
        xyz, rgb = ref.points_from_pcl(pcl)
        rec = mapfile.merge_records(rec, mrr.records_from_points(xyz, rgb, T, VOXEL).astype(RAW))
    print("%d keyframes, %d voxels carved (%d points); the map holds %d voxels, without carving %d"
          % (g.nKeyFrames, carved, points, len(rec), vm0.info()["voxels"]))
    assert carved > 0 and any(c[2] is not None for c in g.carves)
    assert g.carve_skipped == sum(c[2] is None for c in g.carves) and g0.carve_skipped == 0
    assert vm.export_raw().tobytes() == rec.tobytes()
    i, i0 = vm.info(), vm0.info()
    assert i["keyframes"] == i0["keyframes"] == g.nKeyFrames and i["points_dropped"] == i0["points_dropped"]
    assert i["points_integrated"] == i0["points_integrated"] - points == int(rec["count"].sum()) and i["voxels"] == len(rec)
    # records=False: the counters only
    view = [(planes[-1], np.asarray(drawer.vpKfsF[-1], F), cc.intrinsics320())]
    none, einfo, _ = vm.carve_eval(view, records=False, **prm)
    assert none is None and einfo == mapfile.carve_records(rec, VOXEL, view, **prm)[1]
    assert vm.carve(view, records=False, **prm)[:2] == (None, einfo) and vm.info()["voxels"] == len(rec) - einfo["voxels_carved"]
