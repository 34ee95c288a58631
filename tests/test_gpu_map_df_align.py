"""Registration against the distance field on the device (revo_map_df_align_eval / revo_map_df_align, api.VoxelMap.df_align_eval /
df_align, api.DistanceField.align_eval / align, api.localize): records bit for bit the numpy specification's
(tests/map_df_align_ref.py) on one hand-made case per rule and kernel path; the same bytes whatever the side of field, points and
output, the order of the points and what was enqueued before; the map is never changed; every argument error; the loop follows
the specification's on the dense scene; and the measured basin."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile, synth  # noqa: E402
from revo_amd.settings import MapAlignOpts, MapAlignParams, MapDfAlignInfo, MapDfBox, ALIGN_CONVERGED, ALIGN_ITER_LIMIT, ALIGN_LOST  # noqa: E402

import map_align_ref as mar  # noqa: E402
import map_df_align_cases as dc  # noqa: E402
import map_df_align_ref as dfr  # noqa: E402
import map_records_ref as mrr  # noqa: E402
import test_gpu_map_plane as tgp  # noqa: E402
import voxel_map_ref as ref  # noqa: E402

F = np.float32
RAW = mapfile.RAW_DTYPE
INVALID_ARG = -1
V = dc.V
VOXEL = tgp.VOXEL
I4 = np.eye(4, dtype=F)
REC = 208
TWIST = np.array([0.02, -0.015, 0.012, 0.006, -0.005, 0.004])
MAX_DIST = 0.24  # 12 voxels: the field stage's gate on the scene; the box is the map's bounds grown by 14 cells
# Measured on the CPU with the specification: the field stage from the identity, then map_plane_ref.align_plane,
# against D_k; and map_plane_ref.align_maps(metric="plane") from the identity on the same maps.  Errors in (m, rad).
#   k   field stage (30 it., limit)   field + plane               the ladder alone
#   2   1.66e-3  5.93e-4              4.42e-5  2.41e-5  (3 it.)   4.42e-5  2.41e-5  (4 + 3 + 3)
#   4   1.65e-3  5.89e-4              3.32e-5  2.40e-5  (3 it.)   3.31e-5  2.40e-5  (9 + 5 + 3)
#   6   1.61e-3  5.73e-4              6.76e-5  2.48e-5  (3 it.)   6.75e-5  2.48e-5  (12 + 3 + 2)
#   8   1.65e-3  5.66e-4              5.70e-5  1.87e-5  (4 it.)   5.71e-5  1.87e-5  (16 + 3 + 3)
#  10   1.60e-3  5.65e-4              3.27e-5  3.17e-5  (3 it.)   3.27e-5  3.17e-5  (20 + 3 + 3)
# The ladder alone converges at every k of the list 2, 4, 6 and of its extension (8, 10), to the same pose: on this scene there
# is NO k <= 10 at which it fails, so the assertion that one exists is dropped (DESIGN 22 says so).  The ladder's first level
# needs more iterations with every k; with a half-metre gate and k = 16, 24 (about 22 and 34 voxels) it ends at its limit 0.38 m
# and 0.37 m off, where field + plane ends 2.80e-5 m / 2.66e-5 rad and 3.46e-5 m / 2.56e-5 rad off: test_the_basin_beyond_the_ladder.
SPEC_ERR = {2: (4.42e-5, 2.41e-5), 4: (3.32e-5, 2.40e-5), 6: (6.76e-5, 2.48e-5), 8: (5.70e-5, 1.87e-5), 10: (3.27e-5, 3.17e-5)}
SPEC_ERR_FAR = {16: (2.80e-5, 2.66e-5)}  # max_dist 0.5 m
FAR_MAX_DIST = 0.5


def _scene():
    return tgp._scene()


def _map(voxel=V):
    """A map that gives its voxel edge, context and stream: the field is an argument."""
    api, cam = _scene()[:2]
    return api.VoxelMap(cam, voxel)


def _spec(d2, lo, voxel, pts, poses, max_dist, centre):
    return [dfr.df_align_eval(d2, lo, voxel, pts, T, max_dist, centre) for T in poses]


def _check(m, d2, lo, pts, poses, max_dist, centre, what):
    """df_align_eval on the device (host field, points and output) against the specification, record by record."""
    before = m.export_raw().tobytes()
    got = m.df_align_eval(d2, lo, pts, poses, max_dist, centre)
    want = _spec(d2, lo, m.voxel, pts, poses, max_dist, centre)
    for i, (g, w) in enumerate(zip(got, want)):
        a, b = np.frombuffer(bytes(g), np.uint32), np.frombuffer(bytes(w), np.uint32)
        print("%s, pose %d: matched %d of %d (skipped %d), flags %d, words differing %d"
              % (what, i, w.matched, w.considered, w.skipped, w.flags, int(np.sum(a != b))))
        assert bytes(g) == bytes(w), (what, i)
    assert m.export_raw().tobytes() == before
    return want


def test_hand_made_fields_bit_exact():
    m = _map()
    C3 = (0.1, -0.05, 0.2)
    # a 2 x 2 x 2 box: a single interpolation cell; points in it, on its faces and around it
    d2 = np.array([[[0, 1], [4, 9]], [[2, 3], [5, 6]]], np.uint32)
    lo = (3, -2, 5)
    pts = np.concatenate([dc.random_points(lo, (2, 2, 2), 300, 1, margin=0.2), dc.cell_points(lo, dc.rim_cells((2, 2, 2))), dc.ODD_POINTS])
    w = _check(m, d2, lo, pts, [I4], 1.0, C3, "2x2x2")
    assert 50 < w[0].matched < w[0].considered and w[0].skipped > 50
    # lo negative; points at a = 0 and a = n - 2 and one cell further on each side of each axis; non-finite points
    d2, lo, n = dc.base()
    rim = dc.cell_points(lo, dc.rim_cells(n))
    r = dfr.interpolate(d2, lo, V, rim, I4)
    assert r["ok"].reshape(3, 10).tolist() == [[True] * 4 + [False] * 4 + [False, True]] * 3  # in, in, in, in, out x 4, just out, just in
    pts = np.concatenate([dc.random_points(lo, n, 1200, 1), rim, dc.ODD_POINTS])
    w = _check(m, d2, lo, pts, dc.poses(3, 2), 0.08, C3, "base")
    assert all(0 < x.matched < x.considered - x.skipped for x in w) and w[0].skipped >= 12 + 6
    only_rim = _check(m, d2, lo, rim, [I4], 10.0, C3, "rim")[0]
    assert (only_rim.matched, only_rim.skipped) == (15, 15)
    odd = _check(m, d2, lo, dc.ODD_POINTS, [I4], 10.0, C3, "non-finite points")[0]
    assert (odd.matched, odd.skipped, odd.considered) == (0, 6, 6) and not any(odd.S)
    # an axis of one cell, a field that is all NONE, a clamped field
    for flat in ((1, 7, 11), (9, 1, 11), (9, 7, 1)):
        w = _check(m, dc.field_of(flat, [(0, 0, 0)]), lo, pts, [I4], 10.0, C3, "one cell %s" % (flat,))[0]
        assert (w.matched, w.skipped) == (0, len(pts))
    w = _check(m, dc.field_of(n, []), lo, pts, [I4], 10.0, C3, "all NONE")[0]
    assert (w.matched, w.skipped) == (0, len(pts))
    part = d2.copy()
    part[:3] = dc.NONE  # NONE next to values: a cell with one NONE corner is skipped
    w = _check(m, part, lo, pts, [I4], 10.0, C3, "partly NONE")[0]
    assert 0 < w.matched and w.skipped > only_rim.skipped
    w = _check(m, np.minimum(d2, 3), lo, pts, dc.poses(2, 2), 1.0, C3, "clamped")
    assert w[0].matched == w[0].considered - w[0].skipped
    # e exactly max_dist (accepted), and one float above it (gated): points at the centres of cells that hold 4
    four = np.argwhere(d2 == 4)
    four = four[np.all(four <= np.asarray(n) - 2, 1)]
    assert len(four) >= 2
    p4 = dc.cell_points(lo, four)
    e = F(2) * F(V)
    assert np.all(dfr.interpolate(d2, lo, V, p4, I4)["e"] == e)
    w = _check(m, d2, lo, p4, [I4], e, C3, "e == max_dist")[0]
    assert w.matched == len(p4)
    w = _check(m, d2, lo, p4, [I4], np.nextafter(e, F(0)), C3, "e one float above max_dist")[0]
    assert (w.matched, w.skipped) == (0, 0)
    # another voxel edge: cell boundaries are not exact
    m2 = _map(0.02)
    _check(m2, d2, lo, dc.random_points(lo, n, 700, 3, 0.02), dc.poses(2, 2), 0.05, C3, "0.02 m")
    m2.close()
    m.close()


@pytest.mark.parametrize("npts", [1, 511, 513, 5 * 512 + 77])
def test_point_counts(npts):
    m = _map()
    d2, lo, n = dc.base()
    pts = dc.random_points(lo, n, npts, 10 + npts, margin=0.3)
    w = _check(m, d2, lo, pts, dc.poses(3, 6, 0.3), 0.2, (0, 0, 0), "%d points" % npts)
    assert w[0].considered == npts and (npts == 1 or w[0].matched > npts // 4)
    m.close()


def test_poses_in_one_call():
    m = _map()
    d2, lo, n = dc.base()
    pts = dc.random_points(lo, n, 1500, 4, margin=0.5)
    skew, nan, flip = dc.bad_poses()
    good = dc.poses(61, 8, 0.4)
    poses = good[:2] + [skew] + good[2:30] + [nan, flip] + good[30:]
    assert len(poses) == 64
    c = (0.02, 0.01, 0.2)
    w = _check(m, d2, lo, pts, poses, 0.1, c, "64 poses")
    flags = [x.flags for x in w]
    assert sum(flags) == 3 and [flags[2], flags[31], flags[32]] == [1, 1, 1]
    for x in (w[2], w[31], w[32]):  # bit0: the rest zero except pose, centre, max_dist
        assert x.matched == x.considered == x.skipped == 0 and not any(x.S) and x.reserved == 0
        assert tuple(x.centre) == tuple(F(c)) and x.max_dist == F(0.1)
    base = [bytes(x) for x in w]
    assert [bytes(x) for x in m.df_align_eval(d2, lo, pts, poses[:3], 0.1, c)] == base[:3]  # 3 poses
    assert [bytes(m.df_align_eval(d2, lo, pts, T, 0.1, c)) for T in poses[:4]] == base[:4]   # 1 pose a call
    m.close()


def test_same_bytes_whatever_the_sides_the_order_and_the_stream():
    import torch
    api, cam, pyrs, _ = _scene()
    m = api.VoxelMap(cam, V, dense=True)
    d2, lo, n = dc.base()
    pts = dc.random_points(lo, n, 3 * 512 + 100, 12, margin=0.4)
    poses = dc.poses(3, 5, 0.5)
    c = (0.0, 0.1, 0.2)
    base = b"".join(bytes(x) for x in _check(m, d2, lo, pts, poses, 0.1, c, "host"))
    d_d2 = torch.from_numpy(d2.view(np.int32)).cuda()
    d_pts = torch.from_numpy(pts).cuda()
    before = m.export_raw().tobytes()
    for field in (d2, d_d2):
        for p in (pts, d_pts):
            got = m.df_align_eval(field, lo, p, poses, 0.1, c)
            assert b"".join(bytes(x) for x in got) == base
            d_out = torch.full((REC * 3 + 16,), 7, dtype=torch.uint8, device="cuda")
            assert m.df_align_eval(field, lo, p, poses, 0.1, c, d_out=d_out) is None
            m.sync()
            out = d_out.cpu().numpy()
            assert out[:REC * 3].tobytes() == base and np.all(out[REC * 3:] == 7)
    # the sums are exact: the order of the points cannot show
    perm = np.random.default_rng(1).permutation(len(pts))
    assert b"".join(bytes(x) for x in m.df_align_eval(d2, lo, pts[perm], poses, 0.1, c)) == base
    assert m.export_raw().tobytes() == before
    # directly behind an integration and a field build on the same stream, nothing waiting in between
    box_n = (24, 20, 24)
    field_lo = (-12, -10, 40)  # holds a few dozen voxels of keyframe 0 at this edge
    d_f = torch.empty(box_n, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(REC * 3, dtype=torch.uint8, device="cuda")
    scene_pts = torch.from_numpy(dc.random_points(field_lo, box_n, 2000, 3, V, margin=0.2)).cuda()
    torch.cuda.synchronize()
    m.integrate(pyrs[0], tgp.KF_POSES[0])
    m.distance_field_into(d_f, field_lo, box_n, wait=False)
    assert m.df_align_eval(d_f, field_lo, scene_pts, poses, 0.3, c, d_out=d_out) is None
    m.sync()
    f_host = d_f.cpu().numpy().view(np.uint32)
    want = _spec(f_host, field_lo, V, scene_pts.cpu().numpy(), poses, 0.3, c)
    assert d_out.cpu().numpy().tobytes() == b"".join(bytes(x) for x in want)
    assert f_host.tobytes() == mapfile.distance_field_records(m.export_raw(), field_lo, box_n)[0].tobytes() and want[0].matched > 100
    # a DistanceField of a live map and a MapWindow forward to the same call
    f = api.DistanceField(d2, lo, V, map=m)
    assert b"".join(bytes(x) for x in f.align_eval(pts, poses, 0.1, c)) == base
    w = api.MapWindow(cam, V, window=2)
    assert b"".join(bytes(x) for x in w.df_align_eval(d2, lo, pts, poses, 0.1, c)) == base
    w.close()
    m.close()


def test_argument_errors_write_nothing():
    import torch
    from revo_amd import _lib
    L = _lib.lib()
    m = _map()
    d2, lo, n = dc.base()
    field = np.ascontiguousarray(d2)
    pts = dc.random_points(lo, n, 65, 1, margin=0.2)
    T = np.ascontiguousarray(np.concatenate([I4.T.reshape(16), I4.T.reshape(16)]))
    out = np.full(2 * REC, 7, np.uint8)
    t = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    base = t.data_ptr()
    good = MapDfBox((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*n))
    fp, pp, Tp, op = field.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.c_void_p)

    def prm(max_dist=0.1, centre=(0, 0, 0), mcd=0, mcs=0):
        p = MapAlignParams()
        p.max_dist, p.min_count_dst, p.min_count_src = max_dist, mcd, mcs
        p.centre[:] = centre
        return p

    def call(mm=m, box=good, f=fp, df=0, npts=65, p=pp, di=0, nposes=2, Tq=Tp, pr=prm(), o=op, do=0):
        return L.revo_map_df_align_eval(mm._h if mm is not None else None, C.byref(box) if box is not None else None, f, df, npts, p, di, nposes,
                                        Tq, C.byref(pr) if pr is not None else None, o, do)

    def box(lo_, n_):
        return MapDfBox((C.c_int32 * 3)(*lo_), (C.c_int32 * 3)(*n_))

    R = 1 << 20
    nan, inf = float("nan"), float("inf")
    bad = [call(mm=None), call(box=None), call(f=None), call(p=None), call(Tq=None), call(pr=None), call(o=None),
           call(npts=0), call(npts=(1 << 24) + 1), call(nposes=0), call(nposes=-1), call(nposes=65536),
           call(box=box((0, 0, 0), (0, 3, 5))), call(box=box((0, 0, 0), (4, 3, 1025))), call(box=box((0, 0, 0), (1024, 1024, 129))),
           call(box=box((-R - 1, 0, 0), (4, 3, 5))), call(box=box((0, 0, R - 5), (4, 3, 6))),
           call(df=2), call(di=2), call(do=2), call(df=-1),
           call(f=C.c_void_p(base + 4), df=1), call(p=C.c_void_p(base + 8), di=1), call(o=C.c_void_p(base + 4096 + 4), do=1),
           call(pr=prm(0.0)), call(pr=prm(-1.0)), call(pr=prm(nan)), call(pr=prm(inf)), call(pr=prm(centre=(0, nan, 0))), call(pr=prm(centre=(inf, 0, 0))),
           call(pr=prm(mcd=1)), call(pr=prm(mcs=1))]
    assert bad == [INVALID_ARG] * len(bad) and L.revo_last_error()
    # the loop: the same rules, a T_init that is not finite, max_iters < 1
    T1 = np.full(16, 7, F)
    info, it, st = MapDfAlignInfo(), C.c_int32(77), C.c_int32(77)
    Tnan = np.ascontiguousarray(I4.T.reshape(16)).copy()
    Tnan[13] = nan

    def loop(mm=m, box=good, f=fp, npts=65, p=pp, T0=Tp, pr=prm(), opt=None, To=T1.ctypes.data_as(C.POINTER(C.c_float)), stp=C.byref(st)):
        return L.revo_map_df_align(mm._h if mm is not None else None, C.byref(box) if box is not None else None, f, 0, npts, p, 0, T0,
                                   C.byref(pr) if pr is not None else None, C.byref(opt) if opt is not None else None, To, C.byref(info), C.byref(it), stp)

    badl = [loop(mm=None), loop(box=None), loop(f=None), loop(p=None), loop(T0=None), loop(pr=None), loop(To=None), loop(stp=None), loop(npts=0),
            loop(box=box((0, 0, 0), (0, 3, 5))), loop(pr=prm(0.0)), loop(pr=prm(mcd=2)), loop(T0=Tnan.ctypes.data_as(C.POINTER(C.c_float))),
            loop(opt=MapAlignOpts(0, 0, 1e-6, 1e-6, 12))]
    assert badl == [INVALID_ARG] * len(badl)
    m.sync()
    assert np.all(out == 7) and not t.cpu().numpy().any() and np.all(T1 == 7) and (it.value, st.value) == (77, 77) and not any(bytes(info))
    # the handle is as usable as before
    assert call() == 0 and loop() == 0
    want = _spec(d2, lo, V, pts, [I4, I4], 0.1, (0, 0, 0))
    assert out.tobytes() == b"".join(bytes(x) for x in want)
    m.close()


def test_the_loop_on_a_hand_made_surface():
    """A cloud sampled from the field's own solids: the loop recovers the twist exactly as the specification's does, from host
    and from device memory; a limited and a lost run."""
    import torch
    from revo_amd import api
    m = _map()
    d2, lo, n, solids = dc.blob()
    D = dc.se3((0.03, -0.02, 0.025, 0.02, -0.015, 0.01))
    Di = np.linalg.inv(D)
    p = (dc.cell_points(lo, solids).astype(np.float64) @ Di[:3, :3].T + Di[:3, 3]).astype(F)
    c = dfr.default_centre(p, I4)
    T, rec, it, st = dfr.df_align(d2, lo, V, p, I4, F(8 * V), c)
    got = m.df_align(d2, lo, p)
    assert got["T"].tobytes() == T.tobytes() and bytes(got["info"]) == bytes(rec) and (got["iterations"], got["status"]) == (it, st)
    assert st == ALIGN_CONVERGED and got["centre"].tobytes() == c.tobytes()
    dev = m.df_align(torch.from_numpy(d2.view(np.int32)).cuda(), lo, torch.from_numpy(p).cuda(), centre=c)
    assert dev["T"].tobytes() == T.tobytes() and bytes(dev["info"]) == bytes(rec)
    H, g = api.df_align_system(got["info"])
    assert np.array_equal(H, dfr.system(rec)[0]) and got["sigma2"] == float(rec.S[27]) / (rec.matched - 6)
    lim = m.df_align(d2, lo, p, max_iters=2)
    assert (lim["status"], lim["iterations"]) == (ALIGN_ITER_LIMIT, 2) and lim["T"].tobytes() == dfr.df_align(d2, lo, V, p, I4, F(8 * V), c, max_iters=2)[0].tobytes()
    away = I4.copy()
    away[:3, 3] = (7, -9, 11)
    lost = m.df_align(d2, lo, p, away)
    assert (lost["status"], lost["iterations"]) == (ALIGN_LOST, 0) and lost["T"].tobytes() == away.tobytes() and lost["info"].skipped == len(p)
    m.close()


# ----------------------------------------------------------------------------------------------------------- the scene --
def _D(k):
    return synth.se3_exp(k * TWIST)


@functools.lru_cache(maxsize=None)
def _scene_field(max_dist=MAX_DIST):
    """The specification's field of the dense scene map over its bounds grown by ceil(max_dist / voxel) + 2 cells."""
    rec = tgp._records(True).astype(RAW)
    lo, hi, _ = mapfile.bounds_records(rec)
    lo, n = mapfile.padded_box(lo, hi, int(np.ceil(max_dist / VOXEL)) + 2)
    return mapfile.distance_field_records(rec, lo, n)[0], lo, n


@functools.lru_cache(maxsize=None)
def _source_points(k):
    """The points of the same keyframes' map under D_k^-1, from the specification's voxel map."""
    Di = np.linalg.inv(_D(k))
    r = ref.VoxelMapRef(VOXEL)
    for (xyz, rgb), T in zip(_scene()[3][True], tgp.KF_POSES):
        r.integrate(xyz, rgb, (Di @ T.astype(np.float64)).astype(F))
    return mar.points_of(mrr.records_of(r), 1)[1]


def _source_map(k):
    api, cam, pyrs, _ = _scene()
    Di = np.linalg.inv(_D(k))
    m = api.VoxelMap(cam, VOXEL, dense=True)
    for p, T in zip(pyrs, tgp.KF_POSES):
        m.integrate(p, (Di @ T.astype(np.float64)).astype(F))
    return m


def _err(T, k):
    E = np.linalg.inv(_D(k)) @ np.asarray(T, np.float64)
    return float(np.linalg.norm(E[:3, 3])), synth.rot_angle(np.eye(3), E[:3, :3])


@pytest.mark.parametrize("k", [2, 4, 6])
def test_scene_records_and_loop_follow_the_specification(k):
    dst = tgp._build(True)
    d2, lo, n = _scene_field()
    f = dst.distance_field(lo=lo, n=n)
    assert f.d2.tobytes() == d2.tobytes()
    pts = _source_points(k)
    src = _source_map(k)
    assert src.points()[0].tobytes() == pts.tobytes()
    c = dfr.default_centre(pts, I4)
    got = f.align(pts, max_dist=MAX_DIST)
    T, rec, it, st = dfr.df_align(d2, lo, F(VOXEL), pts, I4, F(MAX_DIST), c)
    dt = float(np.linalg.norm(got["T"][:3, 3].astype(np.float64) - T[:3, 3]))
    da = synth.rot_angle(got["T"][:3, :3], T[:3, :3])
    print("k %d: device %d iterations, status %d; specification %d, %d; poses differ by %.3g m, %.3g rad; error against D_k %.3g m %.3g rad"
          % ((k, got["iterations"], got["status"], it, st, dt, da) + _err(got["T"], k)))
    assert got["centre"].tobytes() == c.tobytes()
    # records at the start pose and at the end pose, bit for bit
    ends = f.align_eval(pts, [I4, got["T"]], MAX_DIST, c)
    assert bytes(ends[0]) == bytes(dfr.df_align_eval(d2, lo, F(VOXEL), pts, I4, F(MAX_DIST), c))
    assert bytes(ends[1]) == bytes(dfr.df_align_eval(d2, lo, F(VOXEL), pts, got["T"], F(MAX_DIST), c)) == bytes(got["info"])
    assert ends[0].matched > 60000 and ends[0].considered == len(pts)
    assert (got["iterations"], got["status"]) == (it, st)
    assert dt < 1e-5 and da < 1e-5  # the project's pose-parity tolerance (test_gpu_map_align.py)
    src.close()


@pytest.mark.parametrize("k", [2, 4, 6, 8, 10])
def test_localize_ends_where_the_specification_does(k):
    """api.localize (field stage, then point-to-plane) against D_k: within twice the specification's own measured error
    (SPEC_ERR; the margin convention of LADDER_ERR_T / R: the device loop may take a different last step)."""
    from revo_amd import api
    dst, src = tgp._build(True), _source_map(k)
    before = dst.export_raw().tobytes(), src.export_raw().tobytes()
    r = api.localize(dst, src, max_dist=MAX_DIST)
    et, er = _err(r["T"], k)
    stages = dict(r["stages"])
    print("k %d: field %d iterations (status %d, error %.3g m %.3g rad), plane %d iterations (status %d), error %.3g m %.3g rad (specification %.3g, %.3g)"
          % ((k, stages["field"]["iterations"], stages["field"]["status"]) + _err(stages["field"]["T"], k)
             + (stages["plane"]["iterations"], stages["plane"]["status"], et, er) + SPEC_ERR[k]))
    assert [s for s, _ in r["stages"]] == ["field", "plane"] and r["status"] == ALIGN_CONVERGED and stages["field"]["status"] != ALIGN_LOST
    assert r["box"][1].tolist() == list(_scene_field()[2]) and C.sizeof(r["info"]) == 208 and r["info"].dst_normals > 1000
    assert et < 2 * SPEC_ERR[k][0] and er < 2 * SPEC_ERR[k][1]
    assert (dst.export_raw().tobytes(), src.export_raw().tobytes()) == before
    if k == 2:  # the other sources: the map's points as an array and a keyframe (no refinement: the source is no map)
        pts = src.points()[0]
        a = api.localize(dst, pts, max_dist=MAX_DIST)
        assert [s for s, _ in a["stages"]] == ["field"] and a["T"].tobytes() == stages["field"]["T"].tobytes()
        assert api.localize(dst, src, max_dist=MAX_DIST, refine=None)["T"].tobytes() == a["T"].tobytes()
        kf = api.localize(dst, _scene()[2][1], np.linalg.inv(_D(2)) @ tgp.KF_POSES[1].astype(np.float64), max_dist=MAX_DIST)
        E = np.linalg.inv(tgp.KF_POSES[1].astype(np.float64)) @ kf["T"].astype(np.float64)
        print("keyframe 1 against the map: %d iterations, status %d, %.3g m %.3g rad from its pose"
              % (kf["iterations"], kf["status"], np.linalg.norm(E[:3, 3]), synth.rot_angle(np.eye(3), E[:3, :3])))
        # A keyframe's raw points against voxel centres: the field stands for a surface up to half a voxel edge from it, and
        # without a refining stage the pose cannot be asked to be better than that discretisation -- half an edge, and half an
        # edge over the metre the cloud spans.  (Measured: 5.24e-3 m, 6.0e-4 rad, at the iteration limit.)
        assert kf["status"] != ALIGN_LOST and np.linalg.norm(E[:3, 3]) < 0.5 * VOXEL and synth.rot_angle(np.eye(3), E[:3, :3]) < 0.5 * VOXEL / 1.0
        with pytest.raises(ValueError):
            api.localize(dst, src, refine="planes")
    src.close()


def test_the_basin_beyond_the_ladder():
    """Past that list: at k = 16 (about 22 voxels) and a half-metre gate the coarse-to-fine ladder alone ends at its
    iteration limit far off, where localize ends within twice the specification's measured error (SPEC_ERR_FAR)."""
    from revo_amd import api
    k = 16
    dst, src = tgp._build(True), _source_map(k)
    lad = api.align_maps(dst, src, metric="plane")
    r = api.localize(dst, src, max_dist=FAR_MAX_DIST)
    (lt, lr), (et, er) = _err(lad["T"], k), _err(r["T"], k)
    print("k %d: the ladder alone ends with status %d, %.3g m %.3g rad off; localize with status %d, %.3g m %.3g rad off"
          % (k, lad["status"], lt, lr, r["status"], et, er))
    assert lad["status"] != ALIGN_CONVERGED or lt > VOXEL
    assert r["status"] == ALIGN_CONVERGED and et < 2 * SPEC_ERR_FAR[k][0] and er < 2 * SPEC_ERR_FAR[k][1]
    src.close()
