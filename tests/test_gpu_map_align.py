"""Registration of voxel maps on the device (revo_map_coarsen / revo_map_align_eval / revo_map_align, api.align_maps):
every record is bit for bit the numpy specification's (tests/map_align_ref.py over the records of tests/map_records_ref.py),
whatever the table size, the integration order, the batching of poses, the output side or the grid; the maps are not changed
and a search full of misses leaves the destination's fault word clear; coarsening equals building at the coarse edge; the
iteration follows the specification's loop and the ladder recovers a known twist."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile, synth  # noqa: E402
from revo_amd.settings import ImgPyramidSettings, MapAlignInfo, MapAlignParams, ALIGN_CONVERGED  # noqa: E402

import map_align_ref as mar  # noqa: E402
import map_records_ref as mrr  # noqa: E402
import voxel_map_ref as ref  # noqa: E402

F = np.float32
INVALID_ARG, CAPACITY = -1, -5
S320 = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
SEEDS = [902, 903]
I4 = np.eye(4, dtype=F)


def _T(tw):
    return synth.se3_exp(np.asarray(tw, np.float64)).astype(F)


KF_POSES = [_T([0, 0, 0, 0, 0, 0]), _T([0.05, 0.01, 0.0, 0.0, 0.03, 0.0])]
D_SMALL = synth.se3_exp(np.array([0.006, -0.004, 0.005, 0.002, -0.001, 0.0015]))
# poses for a source built at D_SMALL * pose: a few millimetres from alignment (D_SMALL^-1), and a voxel and a half (0.02 m
# voxels) along x from it
NEAR = (synth.se3_exp(np.array([0.003, -0.002, 0.002, 0.001, -0.001, 0.0005])) @ np.linalg.inv(D_SMALL)).astype(F)
OFF = (synth.se3_exp(np.array([0.03, 0.0, 0.0, 0.0, 0.0, 0.0])) @ np.linalg.inv(D_SMALL)).astype(F)
D_LADDER = synth.se3_exp(np.array([0.02, -0.015, 0.012, 0.006, -0.005, 0.004]))  # 1.4 voxels of 0.02 m, 0.0088 rad
# The specification's own ladder (shifts 2, 1, 0; edge clouds of SEEDS at KF_POSES, voxel 0.02, source at D_LADDER * pose, from
# identity) ends 4.90e-4 m and 4.05e-4 rad from D_LADDER^-1, measured on the CPU; the smallest Cholesky pivot over its diagonal
# entry is 0.997 at every level (the rank rule refuses 1.4e-14).  The bounds are twice that.
LADDER_ERR_T, LADDER_ERR_R = 2 * 4.90e-4, 2 * 4.05e-4


@functools.lru_cache(maxsize=None)
def _scene():
    """One context and the keyframes every test shares, with their clouds (edge and dense) for the specification."""
    from revo_amd import api
    cam = api.CameraPyr(S320)
    pyrs = [api.ImgPyramidRGBD(S320, cam, *synth.make_pair(sd, S320)["ref"]) for sd in SEEDS]
    clouds = {d: [ref.points_from_pcl(p.generateColoredPcl(0, d)) for p in pyrs] for d in (False, True)}
    return api, cam, pyrs, clouds


@functools.lru_cache(maxsize=None)
def _records(voxel, dense, D_key=None):
    """The specification's records of the keyframes at D * KF_POSES (D_key: None, "small" or "ladder")."""
    clouds = _scene()[3][dense]
    r = ref.VoxelMapRef(voxel)
    for (xyz, rgb), T in zip(clouds, _poses(D_key)):
        r.integrate(xyz, rgb, T)
    return mrr.records_of(r)


def _poses(D_key=None):
    D = {None: np.eye(4), "small": D_SMALL, "ladder": D_LADDER}[D_key]
    return [(D @ T.astype(np.float64)).astype(F) for T in KF_POSES]


def _build(voxel, dense, D_key=None, order=(0, 1), **kw):
    api, cam, pyrs, _ = _scene()
    m = api.VoxelMap(cam, voxel, dense=dense, **kw)
    Ts = _poses(D_key)
    for i in order:
        m.integrate(pyrs[i], Ts[i])
    return m


def _hand(voxel, rows, **kw):
    """A map from hand-made voxels: rows of (index triple, mean point, count); -> (VoxelMap, its records)."""
    api, cam = _scene()[:2]
    rec = np.zeros(len(rows), mapfile.RAW_DTYPE)
    for r, (k, p, n) in zip(rec, rows):
        r["key"] = ref.pack_keys(np.array([k], np.int64))[0]
        q = np.asarray(p, np.float64) * 2.0 ** 20
        assert np.all(q == np.rint(q))  # the point is on the 2^-20 m grid: the voxel's mean is exactly p
        r["count"], r["sum_q"], r["sum_bgr"] = n, (q * n).astype(np.int64), (10 * n, 20 * n, 30 * n)
    rec = rec[np.argsort(rec["key"])]
    m = api.VoxelMap(cam, voxel, **kw)
    m.merge_raw(rec)
    return m, rec.astype(mrr.DTYPE)


def _check(dst, dst_rec, src, src_rec, poses, what, **prm):
    """align_eval on the device against the specification, record by record; -> the records."""
    got = dst.align_eval(src, poses, **prm)
    spec = dict(prm)
    spec.setdefault("max_dist", F(dst.voxel))
    want = [mar.align_eval(dst_rec, F(dst.voxel), src_rec, T, **spec) for T in poses]
    for i, (g, w) in enumerate(zip(got, want)):
        a, b = np.frombuffer(bytes(g), np.uint32), np.frombuffer(bytes(w), np.uint32)
        print("%s, pose %d: matched %d of %d (skipped %d), words differing %d" % (what, i, w.matched, w.considered, w.skipped, int(np.sum(a != b))))
        assert bytes(g) == bytes(w), (what, i)
    return want


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("dense", [False, True], ids=["edges", "dense"])
def test_bit_exact_against_the_specification(dense, min_count):
    voxel = 0.02
    dst, src = _build(voxel, dense), _build(voxel, dense, "small")
    dr, sr = _records(voxel, dense), _records(voxel, dense, "small")
    assert dst.export_raw().tobytes() == dr.tobytes()
    c = mar.default_centre(sr, I4, min_count)
    w = _check(dst, dr, src, sr, [NEAR, OFF], "gate 1 voxel", min_count_dst=min_count, min_count_src=min_count, centre=c)
    assert w[0].matched > 1000 and w[0].considered == int((sr["count"] >= min_count).sum())
    # the pose that is off leaves many voxels unmatched, though the gate is a whole voxel
    assert 0 < w[1].matched < w[0].matched and w[1].considered - w[1].matched > 1000
    w = _check(dst, dr, src, sr, [NEAR, OFF], "gate 1/4 voxel", max_dist=0.005, min_count_dst=min_count, min_count_src=min_count, centre=c)
    assert all(0 < x.matched < x.considered // 2 for x in w)  # a narrow gate: most voxels unmatched at either pose


P0 = (0.5, 0.5, 0.5)  # in voxel (25, 25, 25) of the 0.02 m grid
E7 = 2.0 ** -7


def test_hand_made_tie_takes_the_smaller_key():
    src, sr = _hand(0.02, [((25, 25, 25), P0, 1)])
    dst, dr = _hand(0.02, [((24, 25, 25), (0.5 - E7, 0.5, 0.5), 1), ((25, 25, 25), (0.5 + E7, 0.5, 0.5), 1)])
    w = _check(dst, dr, src, sr, [I4], "tie")[0]
    assert w.matched == 1 and w.S[9] == E7  # r_x = p' - q > 0: the voxel with the smaller key


def test_hand_made_gate_is_inclusive():
    dy = 1.5 * 2.0 ** -19
    src, sr = _hand(0.02, [((25, 25, 25), P0, 1), ((25, 25, 37), (0.5, 0.5, 0.75), 1)])
    dst, dr = _hand(0.02, [((24, 25, 25), (0.5 - E7, 0.5, 0.5), 1), ((24, 24, 37), (0.5 - E7, 0.5 - dy, 0.75), 1)])
    d2 = (F(E7) * F(E7) + F(dy) * F(dy)) + F(0)
    assert d2 == np.nextafter(F(E7) * F(E7), F(1))  # the second pair lies one float above the gate
    w = _check(dst, dr, src, sr, [I4], "gate", max_dist=E7)[0]
    assert w.matched == 1 and w.considered == 2
    w = _check(dst, dr, src, sr, [I4], "gate, one float lower", max_dist=float(np.nextafter(F(E7), F(0))))[0]
    assert w.matched == 0


def test_hand_made_min_count_dst_prefers_a_farther_voxel():
    src, sr = _hand(0.02, [((25, 25, 25), P0, 1)])
    dst, dr = _hand(0.02, [((25, 25, 25), (0.5 + 2.0 ** -9, 0.5, 0.5), 1), ((24, 25, 25), (0.5 - E7, 0.5, 0.5), 2)])
    assert _check(dst, dr, src, sr, [I4], "min_count 1")[0].S[9] == -2.0 ** -9
    assert _check(dst, dr, src, sr, [I4], "min_count 2", min_count_dst=2)[0].S[9] == E7


def test_hand_made_last_index_and_range():
    v = 2.0 ** -9
    top = (1 << 20) - 1
    x = 2048.0 - 2.0 ** -10  # index 2^20 - 1: the neighbours at 2^20 do not exist
    src, sr = _hand(v, [((top, 0, 0), (x, v / 2, v / 2), 1), ((top - 600, 0, 0), (x - 600 * v, v / 2, v / 2), 1)])
    dst, dr = _hand(v, [((top, 0, 0), (x - 2.0 ** -11, v / 2, v / 2), 1), ((top - 88, 0, 0), (x - 88 * v, v / 2, v / 2), 1)])
    w = _check(dst, dr, src, sr, [I4], "last index")[0]
    assert w.matched == 1 and w.skipped == 0 and w.considered == 2
    shift = I4.copy()
    shift[0, 3] = 1.0  # the first voxel passes 2048 m: skipped and counted; the second lands 512 voxels on, at dst's second
    w = _check(dst, dr, src, sr, [shift], "past 2048 m")[0]
    assert w.skipped == 1 and w.matched == 1 and w.considered == 2


def test_hand_made_empty_maps_subtracted_voxels_and_bad_poses():
    api, cam = _scene()[:2]
    src, sr = _hand(0.02, [((25, 25, 25), P0, 1)])
    rows = [((25, 25, 25), (0.5 + 2.0 ** -9, 0.5, 0.5), 1), ((24, 25, 25), (0.5 - E7, 0.5, 0.5), 2)]
    dst, dr = _hand(0.02, rows)
    empty, er = api.VoxelMap(cam, 0.02), np.zeros(0, mrr.DTYPE)
    w = _check(empty, er, src, sr, [I4], "empty destination")[0]
    assert (w.matched, w.considered) == (0, 1) and not any(w.S)
    w = _check(dst, dr, empty, er, [I4], "empty source")[0]
    assert (w.matched, w.considered) == (0, 0) and not any(w.S)
    # a voxel that a subtraction emptied is absent: the match moves to the other one
    near = dr[dr["key"] == ref.pack_keys(np.array([[25, 25, 25]], np.int64))[0]]
    dst.subtract_raw(near.astype(mapfile.RAW_DTYPE))
    w = _check(dst, dr[dr["key"] != near["key"][0]], src, sr, [I4], "after subtract")[0]
    assert w.matched == 1 and w.S[9] == E7
    # poses that are not evaluated
    skew, nan = I4.copy(), I4.copy()
    skew[0, 1] = 0.01
    nan[1, 3] = np.nan
    _check(dst, dr[dr["key"] != near["key"][0]], src, sr, [skew, nan, I4], "bad poses", centre=(0.1, 0.2, 0.3))
    got = dst.align_eval(src, [skew, nan, I4], centre=(0.1, 0.2, 0.3))
    assert [g.flags for g in got] == [1, 1, 0] and got[0].matched == 0 and not any(got[0].S) and got[2].matched == 1
    assert tuple(got[0].centre) == tuple(F([0.1, 0.2, 0.3])) and got[0].max_dist == F(dst.voxel)


def test_same_bytes_whatever_the_launch():
    import torch
    voxel = 0.02
    sr, dr = _records(voxel, True, "small"), _records(voxel, True)
    assert len(sr) > 8 * 512  # several workgroups: the cross-workgroup partials are exercised
    src = _build(voxel, True, "small")
    poses = [NEAR, OFF, I4]
    base = [bytes(w) for w in _check(_build(voxel, True), dr, src, sr, poses, "dense")]
    # (a dense keyframe grows the small table to 2^19 slots at most; 2^20 voxels start at 2^21)
    small, large = _build(voxel, True, initial_voxels=1 << 10), _build(voxel, True, initial_voxels=1 << 20, order=(1, 0))
    assert small.info()["capacity"] != large.info()["capacity"]
    for m in (small, large):
        assert [bytes(g) for g in m.align_eval(src, poses)] == base
        assert [bytes(m.align_eval(src, T)) for T in poses] == base  # one call per pose
    rsrc = _build(voxel, True, "small", order=(1, 0), initial_voxels=1 << 10)
    assert [bytes(g) for g in small.align_eval(rsrc, poses)] == base
    d = torch.zeros(160 * 3 + 16, dtype=torch.uint8, device="cuda")
    assert small.align_eval(src, poses, d_out=d) is None
    out = d.cpu().numpy()
    assert out[:480].tobytes() == b"".join(base) and not out[480:].any()
    # a map against itself: dst == src is allowed
    w = _check(small, dr, small, dr, [I4], "itself")[0]
    assert w.matched == len(dr) and not any(list(w.S)[9:])


def test_maps_unchanged_and_no_fault_after_misses():
    api, cam, pyrs, _ = _scene()
    voxel = 0.02
    dst, src = _build(voxel, False), _build(voxel, False, "small")
    before = dst.export_raw().tobytes(), src.export_raw().tobytes(), dst.info(), src.info()
    away = I4.copy()
    away[:3, 3] = (7.0, -9.0, 11.0)  # nothing of the destination is there: every probe misses
    w = _check(dst, _records(voxel, False), src, _records(voxel, False, "small"), [away, NEAR], "misses")
    assert w[0].matched == 0 and w[0].considered > 1000 and w[1].matched > 1000
    assert (dst.export_raw().tobytes(), src.export_raw().tobytes(), dst.info(), src.info()) == before
    dst.integrate(pyrs[0], KF_POSES[1])  # the fault word is clear: the map goes on working
    info = dst.info()
    assert info["keyframes"] == 3 and info["voxels"] > before[2]["voxels"]


def test_coarsen_on_the_device():
    from revo_amd import _lib
    api, cam, pyrs, clouds = _scene()
    L = _lib.lib()
    for dense, voxel in ((False, 0.01), (True, 0.02)):
        fine = _build(voxel, dense)
        fr = _records(voxel, dense)
        for shift in (1, 3):
            edge = float(np.ldexp(F(voxel), shift))
            c = fine.coarsen(shift)
            direct = _build(edge, dense)
            got = c.export_raw().tobytes()
            assert got == mar.coarsen(fr, shift).tobytes() == direct.export_raw().tobytes() == _records(edge, dense).tobytes()
            ci, fi = c.info(), fine.info()
            assert c.voxel == edge and all(ci[k] == fi[k] for k in ("points_integrated", "points_dropped", "keyframes"))
            assert ci["voxels"] == direct.info()["voxels"] < fi["voxels"]
        assert fine.export_raw().tobytes() == fr.tobytes()  # the source is unchanged
    # refused for max_voxels: the destination keeps what it had
    tight, tr = _hand(float(np.ldexp(F(0.02), 1)), [((1, 2, 3), (0.0625, 0.125, 0.25), 4)], max_voxels=100)
    info = tight.info()
    assert L.revo_map_coarsen(tight._h, fine._h, 1) == CAPACITY
    assert tight.export_raw().tobytes() == tr.astype(mapfile.RAW_DTYPE).tobytes()
    assert {k: v for k, v in tight.info().items() if k not in ("keyframes_rejected", "capacity", "rehashes")} == \
           {k: v for k, v in info.items() if k not in ("keyframes_rejected", "capacity", "rehashes")}
    # argument errors
    ok = api.VoxelMap(cam, float(np.ldexp(F(0.02), 1)))
    other = api.VoxelMap(cam, 0.05)
    assert L.revo_map_coarsen(other._h, fine._h, 1) == INVALID_ARG  # another edge ratio
    assert L.revo_map_coarsen(ok._h, fine._h, 2) == INVALID_ARG
    assert L.revo_map_coarsen(ok._h, fine._h, 0) == INVALID_ARG and L.revo_map_coarsen(ok._h, fine._h, 21) == INVALID_ARG
    assert L.revo_map_coarsen(fine._h, fine._h, 1) == INVALID_ARG and L.revo_map_coarsen(None, fine._h, 1) == INVALID_ARG
    assert ok.info()["voxels"] == 0 and other.info()["voxels"] == 0


def test_align_eval_argument_errors():
    import torch
    from revo_amd import _lib
    L = _lib.lib()
    src, _ = _hand(0.02, [((25, 25, 25), P0, 1)])
    T = np.ascontiguousarray(I4.T).reshape(16)
    Tp = T.ctypes.data_as(C.POINTER(C.c_float))
    out = MapAlignInfo()

    def prm(max_dist=0.02, centre=(0, 0, 0)):
        p = MapAlignParams()
        p.max_dist, p.min_count_dst, p.min_count_src = max_dist, 1, 1
        p.centre[:] = centre
        return C.byref(p)

    def call(dst=src._h, s=src._h, n=1, t=Tp, p=None, o=C.addressof(out), dev=0):
        return L.revo_map_align_eval(dst, s, n, t, p if p is not None else prm(), C.c_void_p(o), dev)

    assert call() == 0 and out.matched == 1
    assert call(dst=None) == INVALID_ARG and call(s=None) == INVALID_ARG and call(t=None) == INVALID_ARG
    assert call(o=None) == INVALID_ARG and call(n=0) == INVALID_ARG
    assert L.revo_map_align_eval(src._h, src._h, 1, Tp, None, C.byref(out), 0) == INVALID_ARG
    for bad in (0.0, -0.01, float(np.nextafter(F(0.02), F(1))), float("nan"), float("inf")):
        assert call(p=prm(max_dist=bad)) == INVALID_ARG, bad
    assert call(p=prm(centre=(0, float("nan"), 0))) == INVALID_ARG and call(p=prm(centre=(float("inf"), 0, 0))) == INVALID_ARG
    d = torch.zeros(160 + 16, dtype=torch.uint8, device="cuda")
    assert call(o=d.data_ptr() + 4, dev=1) == INVALID_ARG and call(o=d.data_ptr(), dev=1) == 0
    assert d.cpu().numpy()[:160].tobytes() == bytes(out)


def test_align_a_map_to_itself():
    voxel = 0.02
    m = _build(voxel, False)
    r = m.align(m, centre=mar.default_centre(_records(voxel, False), I4))
    assert r["status"] == ALIGN_CONVERGED and r["iterations"] == 1
    assert r["T"].tobytes() == I4.tobytes()
    assert r["info"].matched == m.info()["voxels"] and not any(list(r["info"].S)[9:])
    assert r["cov"] is not None and r["sigma2"] == 0.0


def test_align_follows_the_specification_loop():
    voxel = 0.02
    dst, src = _build(voxel, False), _build(voxel, False, "small")
    dr, sr = _records(voxel, False), _records(voxel, False, "small")
    c = mar.default_centre(sr, I4)
    got = dst.align(src, centre=c)
    T, info, it, status = mar.align(dr, F(voxel), sr, I4, F(voxel), centre=c)
    dt = float(np.linalg.norm(got["T"][:3, 3].astype(np.float64) - T[:3, 3]))
    da = synth.rot_angle(got["T"][:3, :3], T[:3, :3])
    print("device %d iterations, status %d; specification %d, %d; poses differ by %.3g m, %.3g rad; record words differing %d"
          % (got["iterations"], got["status"], it, status, dt, da,
             int(np.sum(np.frombuffer(bytes(got["info"]), np.uint32) != np.frombuffer(bytes(info), np.uint32)))))
    assert dt < 1e-5 and da < 1e-5  # the project's pose-parity tolerance
    assert (got["iterations"], got["status"]) == (it, status) and status == ALIGN_CONVERGED and it > 2
    # the pair (T_out, info_out) satisfies the eval contract on its own
    assert bytes(got["info"]) == bytes(mar.align_eval(dr, F(voxel), sr, got["T"], F(voxel), centre=c))
    cov, s2 = got["cov"], got["sigma2"]
    H, _ = mar.system(got["info"])
    assert s2 == float(got["info"].S[15]) / (3 * got["info"].matched - 6) and np.allclose(cov @ H, s2 * np.eye(6), atol=1e-9 * s2 + 1e-15)
    # an iteration limit, and a lost alignment
    assert dst.align(src, centre=c, max_iters=2)["status"] == 1
    away = I4.copy()
    away[:3, 3] = (7.0, -9.0, 11.0)
    lost = dst.align(src, T_init=away, centre=c)
    assert lost["status"] == 2 and lost["iterations"] == 0 and lost["T"].tobytes() == away.tobytes() and lost["info"].matched == 0


def test_ladder_recovers_the_twist():
    from revo_amd import api
    voxel = 0.02
    dst, src = _build(voxel, False), _build(voxel, False, "ladder")
    r = api.align_maps(dst, src)
    E = r["T"].astype(np.float64) @ D_LADDER  # the identity, if the ladder found D^-1
    et, er = float(np.linalg.norm(E[:3, 3])), synth.rot_angle(np.eye(3), E[:3, :3])
    print("ladder: %s iterations, status %d, %d of %d matched, error %.3g m %.3g rad (bounds %.3g, %.3g)"
          % ([lv["iterations"] for lv in r["levels"]], r["status"], r["info"].matched, r["info"].considered, et, er, LADDER_ERR_T, LADDER_ERR_R))
    assert r["status"] == ALIGN_CONVERGED and len(r["levels"]) == 3
    assert et < LADDER_ERR_T and er < LADDER_ERR_R
    assert r["centre"].tobytes() == mar.default_centre(_records(voxel, False, "ladder"), I4).tobytes()
