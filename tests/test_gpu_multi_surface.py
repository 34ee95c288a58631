"""Surfaces for many sequences at once on the device (revo_map_tsdf_fuse_many / revo_map_tsdf_track_eval_many / revo_map_tsdf_track_many,
api.VoxelMap.fuse_many_into / surface_track_eval_many / surface_track_many, api.fuse_surfaces / track_surfaces).  Every
comparison is byte equality against the single calls (revo_map_tsdf_fuse[_color], revo_map_tsdf_track_eval, revo_map_tsdf_track) on copies
of the same volumes, so there is no tolerance anywhere: boxes of mixed sizes in one launch, pyramid and raw views with and without
colour, volumes that hold earlier views, 1 and 65 jobs, the jobs in reverse order, every refusal with sentinel-filled outputs; the
records of jobs with frames of every size and stride and 1, 3 and 65 poses, whatever the number of workgroups; the lockstep loop
with converging, lost and limited jobs in one call."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_seen_cases as sc  # noqa: E402
import map_tsdf_cases as tc  # noqa: E402
import map_tsdf_track_cases as kc  # noqa: E402
import test_gpu_map_raycast as tr  # noqa: E402
import test_gpu_map_tsdf as tt  # noqa: E402

F = np.float32
INVALID_ARG = -1
REC = 208
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOXES = (((-1, -1, 7), (2, 2, 2)), ((-4, 0, 6), (9, 1, 5)), ((-1, -2, 5), (3, 5, 7)), ((-4, -4, 5), (8, 8, 8)), ((-16, -16, 2), (33, 33, 33)))


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _volumes(n, color, fill=0):
    import torch
    shape = tuple(int(x) for x in n)
    d_tsdf = torch.full(shape + (2,), fill, dtype=torch.int32, device="cuda")
    d_color = torch.full(shape + (4,), fill, dtype=torch.int32, device="cuda") if color else None
    return d_tsdf, d_color


def _job(m, lo, n, view, color=False, trunc=None, before=None):
    """One job on fresh volumes (or on copies of `before`, a (d_tsdf, d_color) pair): a dict fuse_many_into takes, with its three info
    records filled with nines.  view: (depth, T, K[, bgr]) with numpy images, or (pyramid, T)."""
    import torch
    if not isinstance(view[0], api.ImgPyramidRGBD):
        view = (_cuda(np.asarray(view[0], F)), view[1], view[2]) + ((_cuda(view[3]),) if color else ())
    d_tsdf, d_color = _volumes(n, color) if before is None else (before[0].clone(), None if before[1] is None else before[1].clone())
    nines = lambda k: torch.full((k,), 9, dtype=torch.int32, device="cuda")  # noqa: E731
    return dict(map=m, lo=tuple(int(x) for x in lo), view=view, trunc=trunc, d_tsdf=d_tsdf, d_color=d_color, d_info=nines(16),
                d_color_info=nines(8) if color else None, d_view_info=nines(8))


def _copy(job):
    c = dict(job)
    for k in ("d_tsdf", "d_color", "d_info", "d_color_info", "d_view_info"):
        c[k] = None if job[k] is None else job[k].clone()
    return c


def _state(job):
    import torch
    torch.cuda.synchronize()
    return tuple(None if job[k] is None else job[k].cpu().numpy().tobytes() for k in ("d_tsdf", "d_color", "d_info", "d_color_info", "d_view_info"))


def _single(job):
    """The job through the single accumulating call on copies of its volumes -> their bytes and the three records'."""
    c = _copy(job)
    m = c["map"]
    m.fuse_into(c["d_tsdf"], [c["view"]], c["lo"], c["trunc"], accumulate=True, d_info=c["d_info"], d_view_info=c["d_view_info"], d_color=c["d_color"],
                d_color_info=c["d_color_info"])
    return _state(c)


def _many(m, jobs):
    cs = [_copy(j) for j in jobs]
    m.fuse_many_into(cs)
    return [_state(c) for c in cs]


def _check(m, jobs, what):
    want = [_single(j) for j in jobs]
    got = _many(m, jobs)
    for i, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("tsdf", "color", "info", "color_info", "view_info"), g, w):
            assert a == b, (what, "job", i, name)
    return want


def _weighted(state):
    return int(np.frombuffer(state[2], np.uint64)[2])


@functools.lru_cache(maxsize=None)
def _maps():
    return tt._map(voxel=tc.V), tt._map(voxel=cc.VOXEL)


def _raw_views(color):
    views = tc.views_all()[:5]
    rng = np.random.default_rng(31)
    return [v + ((rng.integers(0, 256, np.shape(v[0]) + (3,), dtype=np.uint8),) if color else ()) for v in views]


# -------------------------------------------------------------------------------------------------------------------- fuse --
def test_fuse_mixed_boxes_in_one_launch():
    """2x2x2, an axis of 1, 3x5x7 at lo < 0 (105 cells: the tail path), 8x8x8 (one block) and 33x33x33 (36 blocks) in one call, each
    from another view, with and without colour: the single calls' bytes, records included."""
    m = _maps()[0]
    for color in (False, True):
        views = _raw_views(color)
        jobs = [_job(m, lo, n, views[i], color) for i, (lo, n) in enumerate(BOXES)]
        want = _check(m, jobs, ("mixed", color))
        assert sum(_weighted(w) for w in want) > 100  # something was fused
        # the jobs in reverse order: the same bytes per job
        got = _many(m, jobs[::-1])[::-1]
        assert got == want, ("reversed", color)


def test_fuse_pyramid_and_raw_views_with_and_without_colour_and_two_voxel_edges():
    """Pyramid views (on a map of the scene's voxel edge) and device raw views (on the hand-made cases' map), with and without colour, in
    the same call; then a second call into the volumes the first one left (accumulate), against two single calls in a row."""
    import torch
    mv, ms = _maps()
    pyrs, poses = tr._scene()[2], tr._kf_poses()
    lo, n = sc.scene_box(16)
    raw_c, raw = _raw_views(True), _raw_views(False)
    k = cc.intrinsics320()
    plane = _cuda(pyrs[2].returnDepth(0).copy())
    jobs = [_job(ms, lo, n, (pyrs[0], poses[0]), True), _job(mv, *BOXES[2], raw_c[0], True), _job(ms, lo, n, (pyrs[1], poses[1]), False),
            _job(mv, *BOXES[3], raw[1], False), _job(mv, sc.LO, sc.N, raw_c[3], True, trunc=float(sc.M) * 8)]
    want = _check(ms, jobs, "kinds")
    assert _weighted(want[0]) > 0 and _weighted(want[2]) > 0 and _weighted(want[1]) > 0
    # the pyramid form is the raw form of its planes (the single call's property, here through the batched call)
    as_raw = _job(ms, lo, n, (plane.cpu().numpy(), poses[2], k), False)
    assert _many(ms, [as_raw])[0][0] == _many(ms, [_job(ms, lo, n, (pyrs[2], poses[2]), False)])[0][0]
    # accumulate: a second view into what the first call left, job by job
    first = [_copy(j) for j in jobs]
    ms.fuse_many_into(first)
    second_views = [(pyrs[1], poses[1]), raw_c[1], (pyrs[2], poses[2]), raw[2], raw_c[4]]
    again = [_job(j["map"], j["lo"], tuple(j["d_tsdf"].shape[:3]), v, j["d_color"] is not None, j["trunc"], before=(j["d_tsdf"], j["d_color"]))
             for j, v in zip(first, second_views)]
    want2 = _check(mv, again, "accumulate")
    assert any(a[0] != b[0] for a, b in zip(want2, want))  # the second view changed something
    torch.cuda.synchronize()


def test_fuse_one_job_and_65_jobs():
    m = _maps()[0]
    views = _raw_views(True)
    _check(m, [_job(m, *BOXES[2], views[0], True)], "one job")
    jobs = [_job(m, (-1 - i % 3, -2, 5 + i % 2), (3, 5 - i % 2, 7 - i % 4), views[i % 5][:3 + (i % 2)], bool(i % 2)) for i in range(65)]
    _check(m, jobs, "65 jobs")


def test_fuse_surfaces_of_running_sequences():
    """api.fuse_surfaces: each SurfaceVolume holds what its own integrate() leaves, views and per-view counts included."""
    mv = _maps()[0]
    views = [(_cuda(v[0]), v[1], v[2], _cuda(v[3])) for v in _raw_views(True)]
    a = [api.SurfaceVolume(mv, lo, n) for lo, n in BOXES[2:4]]
    b = [api.SurfaceVolume(mv, lo, n) for lo, n in BOXES[2:4]]
    for rnd in range(2):
        api.fuse_surfaces([(s, views[rnd + i]) for i, s in enumerate(a)])
        for i, s in enumerate(b):
            s.integrate(views[rnd + i])
    for s, t in zip(a, b):
        va, vb = s.volume(), t.volume()
        assert va.cells.tobytes() == vb.cells.tobytes() and va.color.tobytes() == vb.color.tobytes()
        assert s.views == t.views == 2 and s.view_counts() == t.view_counts()


def test_fuse_refusals_write_nothing():
    """Every refusal is of the whole call, before anything is enqueued: sentinel-filled volumes and records stay as they are."""
    import torch
    mv, ms = _maps()
    L = _lib.lib()
    views = _raw_views(True)
    other = api.VoxelMap(api.CameraPyr(cc.settings320()), tc.V)  # a map of another context
    host_depth = np.ascontiguousarray(views[0][0], F)
    skew = np.eye(4, dtype=F)
    skew[0, 1] = 0.01

    def jobs():
        js = [_job(mv, *BOXES[2], views[0], True), _job(mv, *BOXES[3], views[1][:3], False)]
        for j in js:
            for k in ("d_tsdf", "d_color"):
                if j[k] is not None:
                    j[k].fill_(0x2B2B2B2B)
        return js

    def refused(mutate, n_jobs=None, what=""):
        js = jobs()
        before = [_state(j) for j in js]
        arr, n, keep = mv._fuse_jobs(js)
        keep.append(mutate(arr, js))
        code = L.revo_map_tsdf_fuse_many(mv._h, n if n_jobs is None else n_jobs, arr)
        mv.sync()
        assert code == INVALID_ARG, (what, code)
        assert [_state(j) for j in js] == before, what

    def overlap(arr, js):
        arr[1].tsdf = arr[0].tsdf + 8 * 16  # inside job 0's volume, 16-byte aligned

    def overlap_colour(arr, js):
        big = torch.zeros(8 * 8 * 8 * 4 + 64, dtype=torch.int32, device="cuda")
        arr[1].color, arr[1].bgr = arr[0].color + 16, arr[0].bgr
        return big

    def set_(i, **kw):
        def f(arr, js):
            for k, v in kw.items():
                setattr(arr[i], k, v)
        return f

    def view_(i, **kw):
        def f(arr, js):
            for k, v in kw.items():
                if k == "T_w_c":
                    arr[i].view.T_w_c[:] = v
                else:
                    setattr(arr[i].view, k, v)
        return f

    refused(overlap, what="overlapping TSDF volumes")
    refused(overlap_colour, what="overlapping colour volumes")
    refused(view_(0, depth=host_depth.ctypes.data), what="a host depth image")
    refused(set_(0, bgr=np.zeros((12, 16, 3), np.uint8).ctypes.data), what="a host colour image")
    refused(set_(1, map=other._h), what="another context's map")
    refused(view_(1, T_w_c=np.ascontiguousarray(skew.T).reshape(16).tolist()), what="a view pose that is no rotation")
    refused(view_(0, T_w_c=[float("nan")] * 16), what="a view pose that is not finite")
    refused(lambda arr, js: None, n_jobs=0, what="no job")
    refused(lambda arr, js: None, n_jobs=1025, what="1025 jobs")
    refused(set_(0, tsdf=None), what="a NULL volume")
    refused(set_(1, trunc=-1.0), what="a negative trunc")
    refused(set_(1, trunc=float("nan")), what="a trunc that is no number")
    refused(set_(1, reserved=1), what="a reserved word")
    refused(set_(0, bgr=None), what="a raw colour view without its image")
    refused(set_(1, bgr=1 << 20), what="an image without a colour volume")
    refused(view_(0, width=0), what="a view rule")
    refused(lambda arr, js: setattr(arr[1].box, "n", (C.c_int32 * 3)(0, 8, 8)), what="a box rule")
    refused(lambda arr, js: setattr(arr[0], "tsdf", arr[0].tsdf + 8), what="a misaligned volume")
    assert L.revo_map_tsdf_fuse_many(None, 1, mv._fuse_jobs(jobs())[0]) == INVALID_ARG and L.revo_map_tsdf_fuse_many(mv._h, 1, None) == INVALID_ARG
    # and the same jobs untouched are taken
    js = jobs()
    for j in js:
        j["d_tsdf"].zero_()
        if j["d_color"] is not None:
            j["d_color"].zero_()
    _check(mv, js, "accepted")
    with pytest.raises(ValueError):
        mv.fuse_many_into([dict(js[0], view=(host_depth,) + tuple(js[0]["view"][1:]))])  # the API's own: host images
    other.close()


# -------------------------------------------------------------------------------------------------------------- track eval --
def _eval_job(c, m=None, poses=None):
    """A case of map_tsdf_track_cases as a job of surface_track_eval_many, volume and frame on the device."""
    return dict(map=m if m is not None else _maps()[0], tsdf=tt._as_tensor(c["cells"]), lo=c["lo"], trunc=c["trunc"],
                frame=(_cuda(c["depth"]), c["camera"], c["zrange"]), poses=c["poses"] if poses is None else poses, max_dist=c["max_dist"], stride=c["stride"],
                min_weight=c["min_weight"], centre=c["centre"] if c["centre"] is not None else (0.0, 0.0, 0.0))


def _eval_single(job):
    m = job["map"]
    recs = m.surface_track_eval(job["tsdf"], job["lo"], job["trunc"], job["frame"], np.asarray(job["poses"], F).reshape(-1, 4, 4), job["max_dist"], job["stride"],
                                job["min_weight"], job["centre"])
    return b"".join(bytes(r) for r in recs)


def _eval_many(m, jobs):
    return [b"".join(bytes(r) for r in recs) for recs in m.surface_track_eval_many(jobs)]


SIZED = ["%dx%d stride %d" % (w, h, s) for (w, h) in ((1, 1), (16, 12), (33, 17), (64, 48)) for s in (1, 2, 3, 8)]


def _pose_sets():
    many = kc.cases()["65 poses"]["poses"]  # a pose that is no rotation at 7, a pose that is not finite at 40
    return {1: many[7:8], 3: many[[3, 40, 5]], 65: many}


def _eval_jobs():
    """Frames of 1x1, 16x12, 33x17 and 64x48 at the strides 1, 2, 3, 8, with 1, 3 or 65 poses each (a NaN pose and a pose that is no
    rotation among them), and further cases of the table on maps of two voxel edges: 21 jobs, 500-odd poses, one launch."""
    sets = _pose_sets()
    jobs = [_eval_job(kc.cases()[name], poses=sets[(1, 3, 65)[i % 3]] if i % 4 != 3 else None) for i, name in enumerate(SIZED)]
    for name in ("3x5x7 lo < 0", "the gate at equality", "a pose that is no rotation, a pose that is not finite", "sphere"):
        jobs.append(_eval_job(kc.cases()[name]))
    jobs.append(_eval_job(kc.cases()["scene 64^3"], m=_maps()[1]))
    return jobs


def test_track_eval_many_is_the_single_calls():
    mv = _maps()[0]
    jobs = _eval_jobs()
    want = [_eval_single(j) for j in jobs]
    got = _eval_many(mv, jobs)
    assert [len(g) for g in got] == [len(w) for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, ("job", i)
    flags = np.concatenate([np.frombuffer(w, mapfile.TSDF_TRACK_DTYPE)["flags"] for w in want])
    matched = np.concatenate([np.frombuffer(w, mapfile.TSDF_TRACK_DTYPE)["matched"] for w in want])
    assert (flags & 1).sum() >= 8 and (matched > 0).sum() > 100  # records without an evaluation and records with one
    # one job alone, the jobs in reverse order, and the records straight into device memory
    assert _eval_many(mv, jobs[5:6]) == want[5:6]
    assert _eval_many(mv, jobs[::-1])[::-1] == want
    import torch
    total = sum(len(w) for w in want)
    d_out = torch.full((total + REC,), 0x2B, dtype=torch.uint8, device="cuda")
    assert mv.surface_track_eval_many(jobs, d_out=d_out) is None
    mv.sync()
    out = d_out.cpu().numpy().tobytes()
    assert out[:total] == b"".join(want) and out[total:] == bytes([0x2B]) * REC


def test_track_eval_many_refusals_write_nothing():
    import torch
    mv = _maps()[0]
    L = _lib.lib()
    c = kc.cases()["65 poses"]
    other = api.VoxelMap(api.CameraPyr(cc.settings320()), tc.V)

    def call(jobs, mutate=None, n_jobs=None, device_out=0):
        arr, n, counts, keep = mv._track_jobs(jobs, True)
        if mutate is not None:
            keep.append(mutate(arr))
        out = np.full((sum(counts) + 1) * REC, 0x2B, np.uint8)
        code = L.revo_map_tsdf_track_eval_many(mv._h, n if n_jobs is None else n_jobs, arr, out.ctypes.data_as(C.c_void_p), device_out)
        mv.sync()
        return code, out

    # 4097 poses in total: 63 jobs of 65 and one of 2; 4096 are taken
    base = _eval_job(c)
    code, out = call([base] * 63 + [dict(base, poses=c["poses"][:2])])
    assert code == INVALID_ARG and np.all(out == 0x2B)
    code, out = call([base] * 63 + [dict(base, poses=c["poses"][:1])])
    assert code == 0 and out[:65 * REC].tobytes() == _eval_single(base) and out[4095 * REC:4096 * REC].tobytes() == _eval_single(base)[:REC]
    host = np.ascontiguousarray(c["depth"], F)
    for what, kw in (("no job", dict(n_jobs=0)), ("1025 jobs", dict(n_jobs=1025)), ("device_out", dict(device_out=2)),
                     ("n_poses", dict(mutate=lambda a: setattr(a[0], "n_poses", 0))), ("poses", dict(mutate=lambda a: setattr(a[1], "poses", None))),
                     ("volume", dict(mutate=lambda a: setattr(a[0], "tsdf", None))), ("misaligned", dict(mutate=lambda a: setattr(a[0], "tsdf", a[0].tsdf + 8))),
                     ("context", dict(mutate=lambda a: setattr(a[1], "map", other._h))), ("trunc", dict(mutate=lambda a: setattr(a[1], "trunc", 0.0))),
                     ("stride", dict(mutate=lambda a: setattr(a[0].prm, "stride", 9))), ("host image", dict(mutate=lambda a: setattr(a[1].frame, "depth", host.ctypes.data))),
                     ("host volume", dict(mutate=lambda a: setattr(a[0], "tsdf", np.zeros(1 << 16, np.int64).ctypes.data & ~15)))):
        code, out = call([base, dict(base, poses=c["poses"][:3])], **kw)
        assert code == INVALID_ARG and np.all(out == 0x2B), what
    torch.cuda.synchronize()
    other.close()


CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_multi_surface as t
jobs = t._eval_jobs()
print("records", b"".join(t._eval_many(t._maps()[0], jobs)).hex())
"""


def test_the_workgroups_do_not_show():
    """REVO_MAP_TSDF_TRACK_GROUPS=1, 3 and the default, each in a fresh process: the same bytes, the single calls'."""
    outs = []
    for groups in ("1", "3", None):
        env = dict(os.environ)
        env.pop("REVO_MAP_TSDF_TRACK_GROUPS", None)
        if groups is not None:
            env["REVO_MAP_TSDF_TRACK_GROUPS"] = groups
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append([ln.split()[1] for ln in r.stdout.decode().splitlines() if ln.startswith("records ")])
    assert outs[0] == outs[1] == outs[2] and len(outs[0]) == 1
    assert bytes.fromhex(outs[0][0]) == b"".join(_eval_single(j) for j in _eval_jobs())


# -------------------------------------------------------------------------------------------------------------- track loop --
def _loop_jobs():
    """The 64^3 scene box from three of the convergence table's starts, the fronto-parallel wall (rank-deficient: LOST), and a start
    with its own limit of two iterations (ITER_LIMIT)."""
    mv, ms = _maps()
    cells, lo, trunc, views = kc.scene()
    k = cc.intrinsics320()
    starts, _ = kc.scene_starts()
    centre = kc.scene_centre()
    vol, frame = tt._as_tensor(cells), (_cuda(views[0][0]), k[:4], k[4:])
    jobs = [dict(map=ms, tsdf=vol, lo=lo, trunc=trunc, frame=frame, T_init=starts[name], centre=centre) for name in ("t1 x", "r2 y", "tr2 z")]
    w = kc.cases()["wall"]
    jobs.append(dict(map=mv, tsdf=tt._as_tensor(w["cells"]), lo=w["lo"], trunc=w["trunc"], frame=(_cuda(w["depth"]), w["camera"], w["zrange"]), T_init=w["poses"][1],
                     centre=(0.0, 0.0, 0.0)))
    jobs.append(dict(jobs[1], max_iters=2))
    return jobs


def test_track_many_is_the_single_loops():
    mv = _maps()[0]
    jobs = _loop_jobs()
    want = []
    for j in jobs:
        kw = dict(max_iters=j["max_iters"]) if "max_iters" in j else {}
        want.append(j["map"].surface_track(j["tsdf"], j["lo"], j["trunc"], j["frame"], j["T_init"], centre=j["centre"], **kw))
    got, rounds = mv.surface_track_many(jobs)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["T"].tobytes() == w["T"].tobytes(), ("pose", i, g["T"], w["T"])
        assert bytes(g["info"]) == bytes(w["info"]), ("record", i)
        assert (g["iterations"], g["status"]) == (w["iterations"], w["status"]), ("loop", i, g["iterations"], g["status"], w["iterations"], w["status"])
        assert g["evaluations"] == w["iterations"] + (2 if w["status"] == mapfile.ALIGN_LOST else 1), i
        assert g["centre"].tobytes() == w["centre"].tobytes() and (g["cov"] is None) == (w["cov"] is None)
    assert [w["status"] for w in want] == [mapfile.ALIGN_CONVERGED] * 3 + [mapfile.ALIGN_LOST, mapfile.ALIGN_ITER_LIMIT]
    assert want[4]["iterations"] == 2 and want[3]["iterations"] == 0
    assert rounds == max(w["iterations"] + (2 if w["status"] == mapfile.ALIGN_LOST else 1) for w in want)
    print("rounds", rounds, [(w["iterations"], w["status"]) for w in want])
    # one option set for all: with max_iters = 1 every scene job stops at the limit, the wall is still lost
    got1, rounds1 = mv.surface_track_many(jobs[:4], max_iters=1)
    want1 = [j["map"].surface_track(j["tsdf"], j["lo"], j["trunc"], j["frame"], j["T_init"], centre=j["centre"], max_iters=1) for j in jobs[:4]]
    assert [(g["T"].tobytes(), bytes(g["info"]), g["iterations"], g["status"]) for g in got1] == [(w["T"].tobytes(), bytes(w["info"]), w["iterations"], w["status"]) for w in want1]
    assert rounds1 == 2 and [g["status"] for g in got1] == [mapfile.ALIGN_ITER_LIMIT] * 3 + [mapfile.ALIGN_LOST]


def test_track_surfaces_of_running_sequences():
    """api.track_surfaces over SurfaceVolumes: SurfaceVolume.track's results, loop by loop."""
    ms = _maps()[1]
    lo, n, views = tc.scene64()
    k = cc.intrinsics320()
    starts, _ = kc.scene_starts()
    centre = kc.scene_centre()
    surfs = []
    for upto in (4, 3):
        s = api.SurfaceVolume(ms, lo, n, color=False)
        for d, T, kk in views[:upto]:
            s.integrate((_cuda(d), T, kk))
        surfs.append(s)
    frame = (_cuda(views[0][0]), k[:4], k[4:])
    triples = [(surfs[0], frame, starts["t1 x"]), (surfs[1], frame, starts["tr1 y"])]
    got, rounds = api.track_surfaces(triples, centre=centre)
    for (s, f, T), g in zip(triples, got):
        w = s.track(f, T, centre=centre)
        assert g["T"].tobytes() == w["T"].tobytes() and bytes(g["info"]) == bytes(w["info"]) and (g["iterations"], g["status"]) == (w["iterations"], w["status"])
    assert rounds == max(g["evaluations"] for g in got) and got[0]["status"] == mapfile.ALIGN_CONVERGED


def test_track_many_refusals():
    mv = _maps()[0]
    L = _lib.lib()
    from revo_amd.settings import MapAlignOpts, MapTsdfTrackResult
    jobs = _loop_jobs()[3:4] * 2

    def call(mutate=None, opt=None, n_jobs=None, results=True):
        arr, n, _, keep = mv._track_jobs(jobs, False)
        if mutate is not None:
            keep.append(mutate(arr))
        res = (MapTsdfTrackResult * 3)()
        C.memset(res, 0x2B, C.sizeof(res))
        rounds = C.c_int32(77)
        code = L.revo_map_tsdf_track_many(mv._h, n if n_jobs is None else n_jobs, arr, None if opt is None else C.byref(opt), res if results else None, C.byref(rounds))
        return code, bytes(res) == bytes([0x2B]) * C.sizeof(res) and rounds.value == 77

    nan_T = np.eye(4, dtype=F).reshape(16)
    nan_T[13] = np.nan
    for what, kw in (("T_init", dict(mutate=lambda a: setattr(a[1], "poses", nan_T.ctypes.data))), ("max_iters", dict(opt=MapAlignOpts(0, 0, 1e-6, 1e-6, 12))),
                     ("a job's max_iters", dict(mutate=lambda a: setattr(a[0], "n_poses", -1))), ("no job", dict(n_jobs=0)), ("1025 jobs", dict(n_jobs=1025)),
                     ("results", dict(results=False)), ("T_init NULL", dict(mutate=lambda a: setattr(a[0], "poses", None)))):
        code, untouched = call(**kw)
        assert code == INVALID_ARG and untouched, what
    code, untouched = call()
    assert code == 0 and not untouched


# ------------------------------------------------------------------------------------------------------------------ driver --
DRIVER_SEEDS, DRIVER_FRAMES, DRIVER_BIAS = (41, 42, 43), 70, (1, 0, 2)
DRIVER_BOX = dict(lo=(-16, -16, 14), n=(32, 32, 32))
DRIVER_VOXEL = 0.05


@functools.lru_cache(maxsize=None)
def _driver_sequences():
    from lm_settings_cases import S160
    from revo_amd import synth
    from test_gpu_voxel_map import BIASES
    return [[(f[0], f[1], f[2]) for f in synth.make_sequence(seed, S160, DRIVER_FRAMES, max_t=0.01, max_rot_deg=0.4, bias=BIASES[b])]
            for seed, b in zip(DRIVER_SEEDS, DRIVER_BIAS)]


def _volume_bytes(surf):
    v = surf.volume()
    return v.cells.tobytes(), None if v.color is None else v.color.tobytes()


def _tracks_bytes(tracks):
    return [(ts, T0.tobytes(), T.tobytes(), None if info is None else bytes(info), status) for ts, T0, T, info, status in tracks]


@functools.lru_cache(maxsize=None)
def _single_driver(track):
    """vo.REVO(surface=SurfaceVolume, surface_track=track) on each sequence alone -> per sequence (poses, volume bytes, surface_tracks,
    keyframes: [(timestamp, T_w_kf, the keyframe's level-0 depth plane and colour image)], the last view's weighted cells)."""
    from lm_settings_cases import S160
    from revo_amd import vo
    out = []
    for frames in _driver_sequences():
        cam = api.CameraPyr(S160)
        vm = api.VoxelMap(cam, DRIVER_VOXEL, dense=True)
        surf = api.SurfaceVolume(vm, **DRIVER_BOX)
        g = vo.REVO(S160, cameraPyr=cam, voxelMap=vm, surface=surf, surface_track=True if track else None)
        by_ts = {float(f[2]): f[0] for f in frames}
        kfs = []
        for f in frames:
            _, kf = g.push(f[0], f[1], f[2])
            if kf:
                pyr, T = g.keyframe()
                kfs.append((float(pyr.returnTimestamp()), np.array(T, F), pyr.returnDepth(0).copy(), np.ascontiguousarray(by_ts[float(pyr.returnTimestamp())])))
        vol = surf.volume()
        out.append(dict(poses=[(ts_, T.copy()) for ts_, T in g.poses], volume=(vol.cells.tobytes(), vol.color.tobytes()), tracks=list(g.surface_tracks),
                        kfs=kfs, weighted=int((vol.cells["weight"] > 0).sum()), views=surf.views, counts=surf.view_counts(), skipped=g.surface_skipped))
        vm.close()
    return out


def _multi_driver(track, **kw):
    from lm_settings_cases import S160
    from revo_amd import vo
    mv = vo.MultiREVO(S160, 3, map_voxel=DRIVER_VOXEL, map_dense=True, surface=dict(DRIVER_BOX), surface_track=True if track else None, **kw)
    return mv, mv.run(_driver_sequences())


@pytest.mark.parametrize("track", (True, False))
def test_the_driver_fuses_every_stream_as_the_single_driver_does(track, monkeypatch):
    """MultiREVO with 3 streams, a 32^3 box per sequence: per stream the TSDF and colour volumes and the surface_tracks are those of
    vo.REVO(surface=, surface_track=) on that sequence alone, and those of a replay of the reported keyframes through the single track
    and integrate calls.  The two drivers' own poses are equal bit for bit when the tracker's work is split the same way
    (test_gpu_vo_multi's SAME_PARTITION), so the test runs under it."""
    from test_gpu_configs import SAME_PARTITION
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    single = _single_driver(True)
    for i, s in enumerate(single):  # the comparison cannot pass on empty volumes
        statuses = [t[4] for t in s["tracks"]]
        print("sequence", i, "keyframes", len(s["kfs"]), "statuses", statuses, "weighted", s["weighted"])
        assert len(s["kfs"]) >= 3 and mapfile.ALIGN_CONVERGED in statuses and mapfile.ALIGN_LOST in statuses and s["weighted"] > 0, i
    single = _single_driver(track)
    mv, res = _multi_driver(track)
    for i, (r, s) in enumerate(zip(res, single)):
        poses_equal = len(r.poses) == len(s["poses"]) and all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(r.poses, s["poses"]))
        print("sequence", i, "the two drivers' poses equal:", poses_equal)
        # the replay of the reported keyframes through the single calls: the binding comparison
        vm = api.VoxelMap(mv.camPyr, DRIVER_VOXEL, dense=True)
        surf = api.SurfaceVolume(vm, **DRIVER_BOX)
        replay = []
        kf_of = {ts_: (T, d, bgr) for ts_, T, d, bgr in s["kfs"]}
        kts = [ts_ for ts_, *_ in r.surface_tracks] if track else [ts_ for ts_, *_ in s["kfs"]]
        if poses_equal:
            for ts_ in kts:
                T0, d, bgr = kf_of[ts_]
                T = T0
                if track:
                    info, status = None, mapfile.ALIGN_LOST
                    if mapfile.pose_is_orthogonal(T0[:3, :3]):
                        g = surf.track((_cuda(d), None), T0)
                        info, status = g["info"], g["status"]
                        T = g["T"] if status == mapfile.ALIGN_CONVERGED else T0
                    replay.append((ts_, T0, T, info, status))
                if mapfile.pose_is_orthogonal(np.asarray(T, F)[:3, :3]):
                    surf.integrate((_cuda(d), T, None, _cuda(bgr)))
            assert _volume_bytes(r.surface) == _volume_bytes(surf), ("replay", i)
            if track:
                assert _tracks_bytes(r.surface_tracks) == _tracks_bytes(replay), ("replay tracks", i)
        vm.close()
        assert poses_equal, i
        assert _volume_bytes(r.surface) == s["volume"], i
        assert _tracks_bytes(r.surface_tracks) == _tracks_bytes(s["tracks"] if track else []), i
        assert r.surface_skipped == s["skipped"] and r.surface.views == s["views"] and r.surface.view_counts() == s["counts"], i
        assert r.map.export_raw().tobytes() != b"" and r.surface.map is r.map
    for r in res:
        r.map.close()


def test_detaching_stops_the_fusing():
    """attach_surface(None) and reset(): the volumes stay as they are from then on; a surface needs a map of the handle's context."""
    from lm_settings_cases import S160
    from revo_amd import vo
    frames = _driver_sequences()[0]
    mv = vo.MultiREVO(S160, 2)
    vms = [api.VoxelMap(mv.camPyr, DRIVER_VOXEL, dense=True) for _ in range(2)]
    surfs = [api.SurfaceVolume(vm, **DRIVER_BOX) for vm in vms]
    for s in range(2):
        mv.attach_map(s, vms[s])
        mv.attach_surface(s, surfs[s], track=True)
    with pytest.raises(api.RevoError):
        mv.surface_last(0)  # no keyframe yet
    for f in frames[:3]:
        mv.submit([(0, f[0], f[1], f[2]), (1, f[0], f[1], f[2])])
        mv.step()
    rep = mv.surface_last(0)
    assert rep.fused == 1 and rep.keyframes_fused == 1 and rep.status == mapfile.ALIGN_LOST and rep.tracked == 1 and rep.track.matched == 0
    assert sum(getattr(rep.view_info, k) for k in ("outside", "unknown", "free_space", "confirmed", "occluded", "edge")) == 32 ** 3
    assert surfs[0].views == 1 and len(surfs[0].surface_tracks) == 1 and _volume_bytes(surfs[0]) == _volume_bytes(surfs[1])
    before = _volume_bytes(surfs[0])
    assert any(before[0]) and any(before[1])
    mv.attach_surface(0, None)
    while mv.pending(1) > 0:
        mv.step()
    mv.reset(1)
    for f in frames[:3]:  # a new sequence on stream 1, more frames on stream 0: keyframes are promoted, nothing is fused
        mv.submit([(0, f[0], f[1], f[2] + 100.0), (1, f[0], f[1], f[2] + 100.0)])
        mv.step()
    assert mv.nKeyFrames(1) == 1 and _volume_bytes(surfs[0]) == before and _volume_bytes(surfs[1]) == before and surfs[1].views == 1
    with pytest.raises(api.RevoError):
        mv.surface_last(1)
    other = api.VoxelMap(api.CameraPyr(S160), DRIVER_VOXEL)
    with pytest.raises(api.RevoError):
        mv.attach_surface(0, api.SurfaceVolume(other, **DRIVER_BOX))
    with pytest.raises(ValueError):
        vo.MultiREVO(S160, 2, surface=dict(DRIVER_BOX))  # without map_voxel
    other.close()
    for vm in vms:
        vm.close()


# ------------------------------------------------------------------------------------------------------------ command line --
def test_run_tum_streams_surface_writes_the_sequential_files(tmp_path, monkeypatch, capsys):
    """run_tum --streams 2 --streams-surface [--streams-surface-track] on two datasets: per dataset the PLY bytes and surface_poses_*.txt
    of the sequential --surface [--surface-track] run (under SAME_PARTITION, which makes the two drivers' poses equal)."""
    from lm_settings_cases import S160
    from revo_amd import run_tum, synth, tum
    from test_gpu_configs import SAME_PARTITION
    from test_gpu_voxel_map import BIASES
    from test_gpu_vo_multi import _tum_yaml
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    names = ["rgbd_synth_a", "rgbd_synth_b"]
    for k, (n, lens) in enumerate(zip(names, (16, 22))):
        tum.write_synthetic_dataset(str(tmp_path / "data" / n), synth.make_sequence(41 + 2 * k, S160, lens, max_t=0.01, max_rot_deg=0.4, bias=BIASES[1 + k]))
    _tum_yaml(tmp_path, S160, names)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "0", "--map", "0.05"]
    box = ["--surface-box", "-40", "-40", "0", "80", "80", "100", "--surface-trunc", "0.2"]
    runs = (("seq", ["--surface", "surface.ply", "--surface-track"]), ("multi", ["--streams", "2", "--streams-surface", "surface.ply", "--streams-surface-track"]),
            ("seq0", ["--surface", "surface.ply"]), ("multi0", ["--streams", "2", "--streams-surface", "surface.ply"]))
    for sub, extra in runs:
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra + box) == 0, sub
    out = capsys.readouterr().out
    assert "Surface track:" in out and "Surface:" in out
    for n in names:
        for a, b in (("seq", "multi"), ("seq0", "multi0")):
            assert (tmp_path / a / ("poses_%s.txt" % n)).read_bytes() == (tmp_path / b / ("poses_%s.txt" % n)).read_bytes(), n
            ply_a, ply_b = (tmp_path / a / ("surface_%s.ply" % n)).read_bytes(), (tmp_path / b / ("surface_%s.ply" % n)).read_bytes()
            assert ply_a == ply_b and len(ply_a) > 10000, (n, a, len(ply_a))
        sp = (tmp_path / "seq" / ("surface_poses_%s.txt" % n)).read_bytes()
        assert sp == (tmp_path / "multi" / ("surface_poses_%s.txt" % n)).read_bytes() and len(sp.splitlines()) >= 3
        assert not (tmp_path / "multi0" / ("surface_poses_%s.txt" % n)).exists()
