"""Maps under a pose on the device (revo_map_pose_raw / revo_map_merge_posed / revo_map_subtract_posed, api.VoxelMap.pose_raw /
merge_posed / subtract_posed / repose, api.align_merge): the posed records bit for bit the specification's
(tests/map_posed_ref.py) from the host and from the device output, merges and subtractions byte for byte and counter for counter,
whatever the table sizes and orders; all or nothing; the source unchanged and the fault words clear; argument errors (maps on
different devices need two devices and are not exercised); and a registration followed by its merge, visible in the map."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile, synth  # noqa: E402
from revo_amd._lib import RevoError  # noqa: E402
from revo_amd.settings import ImgPyramidSettings, ALIGN_CONVERGED, MapPoseInfo  # noqa: E402

import map_posed_cases as pc  # noqa: E402
import map_posed_ref as mp  # noqa: E402
import map_records_ref as mrr  # noqa: E402
import voxel_map_ref as ref  # noqa: E402

F = np.float32
RAW = mapfile.RAW_DTYPE
INVALID_ARG, CAPACITY = -1, -5
S320 = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
SEEDS = [902, 903]
I4 = pc.I4
VOXEL = 0.02
KF_POSES = [synth.se3_exp(np.asarray(t, np.float64)).astype(F) for t in ([0, 0, 0, 0, 0, 0], [0.05, 0.01, 0.0, 0.0, 0.03, 0.0])]
D_SMALL = synth.se3_exp(np.array([0.006, -0.004, 0.005, 0.002, -0.001, 0.0015]))  # DESIGN 16's D
D_LADDER = synth.se3_exp(np.array([0.02, -0.015, 0.012, 0.006, -0.005, 0.004]))   # DESIGN 17's
POSES = {"D": D_SMALL.astype(F),
         "off": (synth.se3_exp(np.array([0.03, 0.0, 0.0, 0.0, 0.0, 0.0])) @ np.linalg.inv(D_SMALL)).astype(F)}  # a voxel and a half off
# The share of moved source voxels that land on a key the destination already held, dense scene (destination at KF_POSES,
# source at D_LADDER * pose, both 0.02 m), computed with the specification on the CPU (map_posed_ref.overlap_share): at the
# final pose of the specification's point-to-plane ladder (map_plane_ref.align_maps from identity) and at the identity.
S_ALIGNED, S_UNALIGNED = 0.99731, 0.38070
COUNTERS = ("voxels", "points_integrated", "points_dropped", "keyframes", "keyframes_rejected")


@functools.lru_cache(maxsize=None)
def _scene():
    from revo_amd import api
    cam = api.CameraPyr(S320)
    pyrs = [api.ImgPyramidRGBD(S320, cam, *synth.make_pair(sd, S320)["ref"]) for sd in SEEDS]
    clouds = {d: [ref.points_from_pcl(p.generateColoredPcl(0, d)) for p in pyrs] for d in (False, True)}
    return api, cam, pyrs, clouds


def _poses(D_key=None):
    D = {None: np.eye(4), "small": D_SMALL, "ladder": D_LADDER}[D_key]
    return [(D @ T.astype(np.float64)).astype(F) for T in KF_POSES]


@functools.lru_cache(maxsize=None)
def _records(dense, D_key=None, voxel=VOXEL):
    r = ref.VoxelMapRef(voxel)
    for (xyz, rgb), T in zip(_scene()[3][dense], _poses(D_key)):
        r.integrate(xyz, rgb, T)
    return mrr.records_of(r).astype(RAW)


def _build(dense, D_key=None, order=(0, 1), voxel=VOXEL, **kw):
    api, cam, pyrs, _ = _scene()
    m = api.VoxelMap(cam, voxel, dense=dense, **kw)
    Ts = _poses(D_key)
    for i in order:
        m.integrate(pyrs[i], Ts[i])
    return m


def _hand(rec, voxel, **kw):
    api, cam = _scene()[:2]
    m = api.VoxelMap(cam, voxel, **kw)
    m.merge_raw(rec.astype(RAW))
    return m


def _counters(m):
    i = m.info()
    return {k: i[k] for k in COUNTERS}


def _canonical_of(t):
    return mapfile.merge_records(t.cpu().numpy().view(RAW), np.zeros(0, RAW))


@pytest.mark.parametrize("voxel_dst", [0.02, 0.04])
@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("dense", [False, True], ids=["edges", "dense"])
def test_pose_raw_bit_exact(dense, min_count, voxel_dst):
    src, sr = _build(dense, "small"), _records(dense, "small")
    before = src.export_raw().tobytes(), src.info()
    assert before[0] == sr.tobytes()
    for name, T in POSES.items():
        want, winfo = mp.pose_raw(sr, T, voxel_dst, min_count)
        got, ginfo = src.pose_raw(T, voxel_dst, min_count)
        dev, dinfo = src.pose_raw(T, voxel_dst, min_count, device=True)
        print("%s, pose %s, edge %g, min_count %d: %s -> %d canonical records" % ("dense" if dense else "edges", name, voxel_dst, min_count, winfo, len(want)))
        assert ginfo == winfo == dinfo and dev.numel() == 64 * winfo["voxels_moved"]
        assert got.tobytes() == want.tobytes()
        assert _canonical_of(dev).tobytes() == want.tobytes()
        assert winfo["voxels_moved"] > 1000 and (min_count == 1 or winfo["voxels_skipped"] > 0) and len(want) < winfo["voxels_moved"]
    assert (src.export_raw().tobytes(), src.info()) == before


@pytest.mark.parametrize("voxel_dst", [0.02, 0.04])
def test_merge_posed_bytes_and_counters(voxel_dst):
    api, cam = _scene()[:2]
    T = POSES["D"]
    src, sr = _build(False, "small"), _records(False, "small")
    src_before = src.export_raw().tobytes(), src.info()
    posed, info = mp.pose_raw(sr, T, voxel_dst)
    # into an empty map: revo_map_pose_raw's canonical form
    empty = api.VoxelMap(cam, voxel_dst)
    assert empty.merge_posed(src, T) == info
    assert empty.export_raw().tobytes() == posed.tobytes() == src.pose_raw(T, voxel_dst)[0].tobytes()
    assert _counters(empty) == dict(voxels=len(posed), points_integrated=info["points_moved"], points_dropped=info["points_dropped"],
                                    keyframes=2, keyframes_rejected=0)
    # into a map that holds the destination scene, at every table size, integration order and merge order
    dr = _records(False, None, voxel_dst)
    want, _ = mp.merge_posed(dr, sr, T, voxel_dst)
    wc = mp.counters_after_merge(dict(points_integrated=int(dr["count"].sum()), points_dropped=0, keyframes=2),
                                 dict(points_dropped=0, keyframes=2), info)
    assert len(dr) < len(want) < len(dr) + len(posed)
    def check(dst, s2):
        assert dst.export_raw().tobytes() == dr.tobytes() and s2.export_raw().tobytes() == sr.tobytes()
        caps = dst.info()["capacity"], s2.info()["capacity"]  # before the merge, which may grow dst's table
        assert dst.merge_posed(s2, T) == info
        assert dst.export_raw().tobytes() == want.tobytes()
        assert _counters(dst) == dict(wc, voxels=len(want), keyframes_rejected=0)
        return caps

    # both integration orders of either map (an integration sizes the table by the frame, whatever initial_voxels says)
    for order, sorder in (((0, 1), (0, 1)), ((0, 1), (1, 0)), ((1, 0), (0, 1)), ((1, 0), (1, 0))):
        check(_build(False, None, order, voxel_dst), _build(False, "small", sorder))
    # every pairing of table sizes 1x and 8x or more: maps loaded from their records, whose table follows initial_voxels
    caps = set()
    for dinit in (1, 1 << 17):
        for sinit in (1, 1 << 17):
            dst, s2 = _hand(dr, voxel_dst, initial_voxels=dinit), _hand(sr, VOXEL, initial_voxels=sinit)
            for m in (dst, s2):  # the counters of the integrated maps ride on one record that goes again
                m.merge_raw(sr[:1], keyframes=2)
                m.subtract_raw(sr[:1])
            caps.add(check(dst, s2))
    assert len(caps) == 4
    for i in (0, 1):
        sizes = sorted({c[i] for c in caps})
        assert len(sizes) == 2 and sizes[1] >= 8 * sizes[0]
    # merge_posed(a) then merge_posed(b) against the reverse order
    other = _build(False, "ladder")
    Tb = POSES["off"]
    ab, ba = _build(False, None, voxel=voxel_dst), _build(False, None, voxel=voxel_dst)
    ab.merge_posed(src, T), ab.merge_posed(other, Tb)
    ba.merge_posed(other, Tb), ba.merge_posed(src, T)
    assert ab.export_raw().tobytes() == ba.export_raw().tobytes() == mp.merge_posed(want, _records(False, "ladder"), Tb, voxel_dst)[0].tobytes()
    assert _counters(ab) == _counters(ba)
    assert (src.export_raw().tobytes(), src.info()) == src_before  # the source is unchanged, its fault word clear


def test_hand_made_maps():
    api, cam = _scene()[:2]
    # identity, count 1: the same bytes as a plain merge
    rec = pc.singles()
    src = _hand(rec, 0.02)
    a, b = api.VoxelMap(cam, 0.02), api.VoxelMap(cam, 0.02)
    info = a.merge_posed(src, I4)
    b.merge(src)
    assert a.export_raw().tobytes() == b.export_raw().tobytes() == rec.astype(RAW).tobytes() and a.info() == b.info()
    assert info == dict(voxels_in=len(rec), voxels_moved=len(rec), voxels_dropped=0, voxels_skipped=0, points_moved=len(rec),
                        points_dropped=0, points_skipped=0)
    # a whole-voxel translation at edge 2^-6
    rec = pc.counted()
    src = _hand(rec, pc.V6)
    T = pc.translation(np.array(pc.SHIFT) * pc.V6)
    got, info = src.pose_raw(T)
    assert got.tobytes() == pc.shifted(rec).astype(RAW).tobytes() == mp.pose_raw(rec, T, pc.V6)[0].tobytes()
    # voxels pushed past 2048 m and past the key range are dropped and counted
    rec, T, vd = pc.edge_cases()
    src = _hand(rec, 2.0 ** -8)
    dst = api.VoxelMap(cam, vd)
    info = dst.merge_posed(src, T)
    want, winfo = mp.pose_raw(rec, T, vd)
    assert info == winfo and (info["voxels_moved"], info["voxels_dropped"], info["points_dropped"]) == (1, 2, 12)
    assert dst.export_raw().tobytes() == want.tobytes()
    assert _counters(dst) == dict(voxels=1, points_integrated=3, points_dropped=12, keyframes=0, keyframes_rejected=0)
    dst.subtract_posed(src, T)
    assert _counters(dst) == dict(voxels=0, points_integrated=0, points_dropped=0, keyframes=0, keyframes_rejected=0)
    # the last index
    rec, T = pc.last_index()
    src = _hand(rec, 2.0 ** -9)
    got, info = src.pose_raw(T)
    assert got.tobytes() == mp.pose_raw(rec, T, 2.0 ** -9)[0].tobytes() and (int(got["key"][0]) >> 42) == (1 << 21) - 1
    assert src.pose_raw(pc.translation([2.0 ** -8, 0, 0]))[1]["voxels_dropped"] == 1
    # an empty source: nothing happens
    none = api.VoxelMap(cam, 0.02)
    before = dst.export_raw().tobytes(), dst.info()
    assert dst.merge_posed(none, I4)["voxels_in"] == 0 and dst.subtract_posed(none, I4)["voxels_in"] == 0
    assert len(none.pose_raw(I4)[0]) == 0 and none.pose_raw(I4, device=True)[0].numel() == 0
    assert (dst.export_raw().tobytes(), dst.info()) == before
    # a subtracted voxel does not reappear
    rec = pc.singles()
    src = _hand(rec, 0.02)
    src.subtract_raw(rec[4:5].astype(RAW))
    got, info = src.pose_raw(I4)
    assert got.tobytes() == np.delete(rec, 4).astype(RAW).tobytes() and info["voxels_in"] == len(rec) - 1
    # a count of 2^32 is a bad record
    bad = rec[:3].copy()
    bad["count"][1] = 1 << 32
    src = _hand(bad, 0.02)
    with pytest.raises(RevoError) as e:
        src.pose_raw(I4)
    assert e.value.code == INVALID_ARG
    import torch
    buf = torch.full((64 * 4,), 0xAB, dtype=torch.uint8, device="cuda")  # room for every voxel: still nothing may be written
    torch.cuda.synchronize()
    n = C.c_size_t()
    from revo_amd import _lib
    t = np.ascontiguousarray(I4.T).reshape(16)
    assert _lib.lib().revo_map_pose_raw(src._h, t.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(0.02), 1, C.c_void_p(buf.data_ptr()), 4,
                                        C.byref(n), 1, None) == INVALID_ARG
    assert src.info()["voxels"] == 3 and bool((buf == 0xAB).all())
    with pytest.raises(RevoError):
        a.merge_posed(src, I4)
    assert a.export_raw().tobytes() == b.export_raw().tobytes() and a.info() == b.info()


def test_all_or_nothing_subtract_and_repose():
    api, cam = _scene()[:2]
    T, T2 = POSES["D"], POSES["off"]
    src, sr, dr = _build(False, "small"), _records(False, "small"), _records(False)
    want, info = mp.merge_posed(dr, sr, T, VOXEL)
    need = len(want)
    # one voxel short: refused, nothing changed but keyframes_rejected
    dst = _build(False, max_voxels=need - 1)
    before = _counters(dst)
    with pytest.raises(RevoError) as e:
        dst.merge_posed(src, T)
    assert e.value.code == CAPACITY
    assert dst.export_raw().tobytes() == dr.tobytes() and _counters(dst) == dict(before, keyframes_rejected=2)
    dst.merge_raw(dr[:1])  # still usable
    dst.subtract_raw(dr[:1])
    assert dst.export_raw().tobytes() == dr.tobytes()
    # exactly enough: accepted; subtract_posed restores the map byte for byte, counters included
    dst = _build(False, max_voxels=need)
    before = _counters(dst)
    assert dst.merge_posed(src, T) == info and dst.export_raw().tobytes() == want.tobytes() and dst.info()["voxels"] == need
    assert dst.subtract_posed(src, T) == info
    assert dst.export_raw().tobytes() == dr.tobytes() and _counters(dst) == before
    # a map that was never put there
    with pytest.raises(RevoError) as e:
        dst.subtract_posed(src, T)
    assert e.value.code == INVALID_ARG
    assert dst.export_raw().tobytes() == dr.tobytes() and _counters(dst) == before
    # repose: the submap follows its corrected pose
    fresh = _build(False)
    fresh.merge_posed(src, T2)
    dst.merge_posed(src, T)
    dst.repose(src, T, T2)
    assert dst.export_raw().tobytes() == fresh.export_raw().tobytes() == mp.merge_posed(dr, sr, T2, VOXEL)[0].tobytes()
    assert _counters(dst) == _counters(fresh)
    # the second half refused: src is merged back at the old pose
    need2 = len(mp.merge_posed(dr, sr, T2, VOXEL)[0])
    far = pc.translation([0.5, 0.5, 0.5])  # hardly a shared voxel: needs more than either
    assert len(mp.merge_posed(dr, sr, far, VOXEL)[0]) > max(need, need2)
    tight = _build(False, max_voxels=max(need, need2))
    tight.merge_posed(src, T)
    before = _counters(tight)
    with pytest.raises(RevoError) as e:
        tight.repose(src, T, far)
    assert e.value.code == CAPACITY
    assert tight.export_raw().tobytes() == want.tobytes() and _counters(tight) == dict(before, keyframes_rejected=2)
    assert src.export_raw().tobytes() == sr.tobytes() and src.info()["keyframes"] == 2


def test_argument_errors():
    import torch
    from revo_amd import _lib
    api, cam = _scene()[:2]
    L = _lib.lib()
    src, dst = _build(False, "small"), _build(False)
    sr = _records(False, "small")
    before = dst.export_raw().tobytes(), dst.info()
    fp = C.POINTER(C.c_float)

    def cm(T):
        return np.ascontiguousarray(np.asarray(T, F).T).reshape(16)

    good = cm(I4)
    skew, nan, mirror = I4.copy(), I4.copy(), np.diag(F([1, 1, -1, 1]))
    skew[0, 1] = 0.01
    nan[1, 3] = np.nan
    n, info = C.c_size_t(), MapPoseInfo()
    for T in (skew, nan, mirror):
        t = cm(T)
        assert L.revo_map_pose_raw(src._h, t.ctypes.data_as(fp), C.c_float(VOXEL), 1, None, 0, C.byref(n), 0, C.byref(info)) == INVALID_ARG
        assert L.revo_map_merge_posed(dst._h, src._h, t.ctypes.data_as(fp), 1, C.byref(info)) == INVALID_ARG
        assert L.revo_map_subtract_posed(dst._h, src._h, t.ctypes.data_as(fp), 1, C.byref(info)) == INVALID_ARG
    g = good.ctypes.data_as(fp)
    for v in (0.0, -0.02, float("inf"), float("nan")):
        assert L.revo_map_pose_raw(src._h, g, C.c_float(v), 1, None, 0, C.byref(n), 0, None) == INVALID_ARG
    assert L.revo_map_pose_raw(None, g, C.c_float(VOXEL), 1, None, 0, C.byref(n), 0, None) == INVALID_ARG
    assert L.revo_map_pose_raw(src._h, None, C.c_float(VOXEL), 1, None, 0, C.byref(n), 0, None) == INVALID_ARG
    assert L.revo_map_pose_raw(src._h, g, C.c_float(VOXEL), 1, None, 0, None, 0, None) == INVALID_ARG
    assert L.revo_map_pose_raw(src._h, g, C.c_float(VOXEL), 1, None, 0, C.byref(n), 2, None) == INVALID_ARG
    for fn in (L.revo_map_merge_posed, L.revo_map_subtract_posed):
        assert fn(None, src._h, g, 1, None) == INVALID_ARG and fn(dst._h, None, g, 1, None) == INVALID_ARG
        assert fn(dst._h, src._h, None, 1, None) == INVALID_ARG and fn(dst._h, dst._h, g, 1, None) == INVALID_ARG
    # counting only, a misaligned device buffer, and outputs that are too small: nothing is written
    assert L.revo_map_pose_raw(src._h, g, C.c_float(VOXEL), 1, None, 0, C.byref(n), 1, C.byref(info)) == 0
    moved = n.value
    assert moved == info.voxels_moved == len(sr)
    buf = torch.full((64 * moved + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert L.revo_map_pose_raw(src._h, g, C.c_float(VOXEL), 1, C.c_void_p(buf.data_ptr() + 8), moved, C.byref(n), 1, None) == INVALID_ARG
    assert L.revo_map_pose_raw(src._h, g, C.c_float(VOXEL), 1, C.c_void_p(buf.data_ptr()), moved - 1, C.byref(n), 1, None) == CAPACITY
    src.sync()
    assert n.value == moved and bool((buf == 0xAB).all())
    assert L.revo_map_pose_raw(src._h, g, C.c_float(VOXEL), 1, C.c_void_p(buf.data_ptr()), moved, C.byref(n), 1, None) == 0
    src.sync()
    assert _canonical_of(buf[:64 * moved]).tobytes() == mp.pose_raw(sr, I4, VOXEL)[0].tobytes() and bool((buf[64 * moved:] == 0xAB).all())
    assert L.revo_map_pose_raw(src._h, g, C.c_float(VOXEL), 1, None, 0, C.byref(n), 0, None) == 0
    host = np.full(n.value, 0xAB, np.uint8).repeat(64).view(RAW)
    assert L.revo_map_pose_raw(src._h, g, C.c_float(VOXEL), 1, host.ctypes.data_as(C.c_void_p), n.value - 1, C.byref(n), 0, None) == CAPACITY
    assert bool((host.view(np.uint8) == 0xAB).all())
    assert (dst.export_raw().tobytes(), dst.info()) == before and src.export_raw().tobytes() == sr.tobytes()


def test_align_merge_end_to_end():
    api = _scene()[0]
    src, dr = _build(True, "ladder"), _records(True)
    dst = _build(True)
    r = api.align_merge(dst, src)
    assert r["status"] == ALIGN_CONVERGED and r["pose_info"]["voxels_moved"] == src.info()["voxels"]
    again = _build(True)
    assert again.merge_posed(src, r["T"]) == r["pose_info"]
    assert dst.export_raw().tobytes() == again.export_raw().tobytes() and dst.info() == again.info()
    keys = src.pose_raw(r["T"], device=True)[0].cpu().numpy().view(RAW)["key"]
    s = float(np.isin(keys, dr["key"]).mean())
    s0 = float(np.isin(src.pose_raw(I4, device=True)[0].cpu().numpy().view(RAW)["key"], dr["key"]).mean())
    print("share of moved source voxels on a key the destination held: %.5f aligned (specification %.5f), %.5f at the identity "
          "(specification %.5f)" % (s, S_ALIGNED, s0, S_UNALIGNED))
    assert S_ALIGNED - S_UNALIGNED >= 0.1 and s > 0.5 * (S_ALIGNED + S_UNALIGNED)
    assert abs(s0 - S_UNALIGNED) < 5e-6  # the identity is the same pose on both sides: the same share to the figure's digits
    # refusals leave the destination unchanged
    before = again.export_raw().tobytes(), again.info()
    with pytest.raises(RuntimeError):
        api.align_merge(again, src, max_iters=1)  # every level stops at its iteration limit
    with pytest.raises(RuntimeError):
        api.align_merge(again, src, T_init=pc.translation([5.0, 5.0, 5.0]))  # nothing to match: lost
    assert (again.export_raw().tobytes(), again.info()) == before
    lim = api.align_merge(again, src, max_iters=1, accept_limit=True)
    assert lim["status"] == 1 and again.info()["keyframes"] == 6
