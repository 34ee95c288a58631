"""Batched exact unfuse on the device (revo_map_tsdf_unfuse_many, api.VoxelMap.unfuse_many_into, api.unfuse_surfaces / repose_surfaces,
api.fuse_surfaces with SurfaceWindows, vo.MultiREVO(surface=dict(window=N))).  Every comparison is byte equality against the
single call (revo_map_tsdf_unfuse with n = 1 on copies of the same volumes), so there is no tolerance anywhere: boxes of mixed sizes in
one call, pyramid and raw views with and without colour and two voxel edges, 1 and 65 jobs, the jobs reversed; refused jobs between
fitting ones with guard cells around their volumes; results in device and host memory and none at all; everything taken out again;
every argument error with sentinel-filled outputs; the api calls against SurfaceVolume.remove / repose / SurfaceWindow.integrate; the
multi-stream driver's windows against the sequential driver's and against fresh fuses."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile  # noqa: E402
from revo_amd._lib import RevoError  # noqa: E402
from revo_amd.settings import MapTsdfUnfuseJob, MapTsdfUnfuseResult  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_seen_cases as sc  # noqa: E402
import map_tsdf_cases as tc  # noqa: E402
import test_gpu_map_raycast as tr  # noqa: E402
import test_gpu_multi_surface as ms  # noqa: E402

F = np.float32
INVALID_ARG = -1
BOXES = ms.BOXES
GUARD = 16  # cells in front of and behind each volume that no call may write (a multiple of 2: the volume stays 16-byte aligned)
SENT = 0x2B2B2B2B
vp = C.c_void_p


def _guarded(n, words):
    """A zero volume of the box with `words` int32 per cell between two runs of GUARD sentinel cells -> (the volume, the whole)."""
    import torch
    cells = int(np.prod(n))
    whole = torch.full(((cells + 2 * GUARD) * words,), SENT, dtype=torch.int32, device="cuda")
    vol = whole[GUARD * words:(GUARD + cells) * words].view(tuple(int(x) for x in n) + (words,))
    vol.zero_()
    return vol, whole


def _device_view(view, color):
    if isinstance(view[0], api.ImgPyramidRGBD) or hasattr(view[0], "data_ptr"):
        return view
    return (ms._cuda(np.asarray(view[0], F)), view[1], view[2]) + ((ms._cuda(view[3]),) if color else ())


def _job(m, lo, n, fused, view, color=False, trunc=None, fuse_trunc="same"):
    """An unfuse job: guarded volumes that hold the views `fused` (through the existing single accumulating fuse, with fuse_trunc or
    the job's trunc), the view to take out, and info / view_info records filled with nines."""
    import torch
    d_tsdf, w_t = _guarded(n, 2)
    d_color, w_c = _guarded(n, 4) if color else (None, None)
    lo = tuple(int(x) for x in lo)
    fused = [_device_view(v, color) for v in fused]
    if fused:
        m.fuse_into(d_tsdf, fused, lo, trunc if fuse_trunc == "same" else fuse_trunc, accumulate=True, d_color=d_color)
    nines = lambda k: torch.full((k,), 9, dtype=torch.int32, device="cuda")  # noqa: E731
    return dict(map=m, lo=lo, view=_device_view(view, color), trunc=trunc, d_tsdf=d_tsdf, d_color=d_color, d_info=nines(16), d_view_info=nines(8),
                whole=(w_t, w_c))


def _copy(job):
    """The job on copies of its volumes, guards included, and of its records."""
    c = dict(job)
    wholes = []
    for key, words, whole in (("d_tsdf", 2, job["whole"][0]), ("d_color", 4, job["whole"][1])):
        if whole is None:
            wholes.append(None)
            continue
        w = whole.clone()
        c[key] = w[GUARD * words:w.numel() - GUARD * words].view(job[key].shape)
        wholes.append(w)
    c["whole"] = tuple(wholes)
    for k in ("d_info", "d_view_info"):
        c[k] = job[k].clone()
    return c


def _state(job):
    """The bytes of both volumes with their guards, and of the two records."""
    import torch
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy().tobytes() for t in (job["whole"][0], job["whole"][1], job["d_info"], job["d_view_info"]))


def _info_bytes(info):
    return np.array([info[k] for k in mapfile.TSDF_UNFUSE_INFO_KEYS] + [0], np.uint64).tobytes()


def _single(job):
    """The job through revo_map_tsdf_unfuse on copies (n = 1, device_in = 1, device_tsdf = 1) -> (the state with the single call's info in
    the record's place, status)."""
    c = _copy(job)
    try:
        info, status = c["map"].unfuse_into(c["d_tsdf"], [c["view"]], c["lo"], c["trunc"], d_color=c["d_color"], d_view_info=c["d_view_info"]), 0
    except RevoError as e:
        assert e.code == INVALID_ARG and e.misfits > 0
        info, status = e.info, INVALID_ARG
    s = _state(c)
    return (s[0], s[1], _info_bytes(info), s[3]), status


def _many(m, jobs, results="host"):
    """The jobs through one revo_map_tsdf_unfuse_many on copies -> ([state per job], [(info bytes, status) per job] or None)."""
    import torch
    cs = [_copy(j) for j in jobs]
    args = [{k: v for k, v in c.items() if k != "whole"} for c in cs]
    if results == "host":
        res = [(_info_bytes(i), s) for i, s in m.unfuse_many_into(args, wait=True)]
    elif results == "device":
        d_res = torch.full((20 * len(cs),), 9, dtype=torch.int32, device="cuda")
        m.unfuse_many_into(args, wait=False, d_results=d_res)
        m.sync()
        raw = d_res.cpu().numpy().view(np.uint8).reshape(len(cs), 80)
        assert not raw[:, 68:].any()  # the reserved words are zero
        res = [(r[:64].tobytes(), int(r[64:68].view(np.int32)[0])) for r in raw]
    else:
        m.unfuse_many_into(args, wait=False)
        m.sync()
        res = None
    return [_state(c) for c in cs], res


def _check(m, jobs, what, results="host"):
    """Every job of the batched call against the single call on copies: volumes with their guards, info, view_info, status."""
    want = [_single(j) for j in jobs]
    got, res = _many(m, jobs, results)
    for i, (g, (w, status)) in enumerate(zip(got, want)):
        for name, a, b in zip(("tsdf", "color", "info", "view_info"), g, w):
            assert a == b, (what, "job", i, name)
        assert res[i] == (w[2], status), (what, "job", i, "result")
    return want


def _updates(state):
    return int(np.frombuffer(state[2], np.uint64)[1])


def _maps():
    return ms._maps()


def _raw_views(color):
    return ms._raw_views(color)


# ------------------------------------------------------------------------------------------------------- single-call equality --
def test_unfuse_mixed_boxes_in_one_call():
    """2x2x2, an axis of 1, 3x5x7 at lo < 0 (the tail path), 8x8x8 (one block) and 33^3 (36 blocks: the ticket is drawn by many) in one
    call, with and without colour: volumes that hold A and B lose B, byte for byte as through the single call; then the jobs reversed."""
    m = _maps()[0]
    for color in (False, True):
        views = _raw_views(color)
        jobs = [_job(m, lo, n, [views[i], views[(i + 1) % 5]], views[(i + 1) % 5], color) for i, (lo, n) in enumerate(BOXES)]
        want = _check(m, jobs, ("mixed", color))
        assert all(s == 0 for _, s in want) and sum(_updates(w) for w, _ in want) > 100  # every job fitted and something was taken out
        got, _ = _many(m, jobs[::-1])
        assert got[::-1] == [w for w, _ in want], ("reversed", color)
        # ... and what is left is the fuse of A alone
        for i, (j, (w, _)) in enumerate(zip(jobs, want)):
            alone = _job(m, j["lo"], tuple(j["d_tsdf"].shape[:3]), [views[i]], views[0], color)
            assert _state(alone)[:2] == w[:2], ("A alone", color)


def test_unfuse_pyramid_and_raw_views_with_and_without_colour_and_two_voxel_edges():
    """Pyramid views (on a map of the scene's voxel edge) and raw device views (on the hand-made cases' map), with and without colour, in
    one call; the pyramid form equals the raw form of its planes."""
    mv, mscene = _maps()
    pyrs, poses = tr._scene()[2], tr._kf_poses()
    lo, n = sc.scene_box(16)
    raw_c, raw = _raw_views(True), _raw_views(False)
    pv = [(pyrs[i], poses[i]) for i in range(3)]
    jobs = [_job(mscene, lo, n, [pv[0], pv[1]], pv[1], True), _job(mv, *BOXES[2], [raw_c[0], raw_c[1]], raw_c[0], True),
            _job(mscene, lo, n, [pv[1], pv[2]], pv[2], False), _job(mv, *BOXES[3], [raw[1], raw[2]], raw[2], False),
            _job(mv, sc.LO, sc.N, [raw_c[3], raw_c[4]], raw_c[3], True, trunc=float(sc.M) * 8)]
    want = _check(mscene, jobs, "kinds")
    assert all(s == 0 for _, s in want) and all(_updates(w) > 0 for w, _ in want)
    k = cc.intrinsics320()
    as_raw = dict(jobs[2], view=(ms._cuda(pyrs[2].returnDepth(0).copy()), poses[2], k))
    assert _many(mscene, [as_raw])[0][0] == want[2][0]


def test_unfuse_one_job_and_65_jobs():
    m = _maps()[0]
    views = _raw_views(True)
    _check(m, [_job(m, *BOXES[2], [views[0], views[1]], views[1], True)], "one job")
    jobs = []
    for i in range(65):
        color = bool(i % 2)
        a, b = views[i % 5][:3 + color], views[(i + 2) % 5][:3 + color]
        jobs.append(_job(m, (-1 - i % 3, -2, 5 + i % 2), (3, 5 - i % 2, 7 - i % 4), [a, b], b, color))
    want = _check(m, jobs, "65 jobs")
    assert sum(_updates(w) for w, _ in want) > 65


# ------------------------------------------------------------------------------------------------------------ mixed verdicts --
def _refused_cases(m, color):
    """Fitting jobs with three refused ones between them (first, middle, last are refused): a view that was never fused, a cell of the
    view pre-set to the full weight 2^20, and a trunc that differs from the fuse's."""
    import torch
    views = _raw_views(color)
    fit = lambda i, b: _job(m, *BOXES[b], [views[i], views[(i + 1) % 5]], views[i], color)  # noqa: E731
    never = _job(m, *BOXES[2], [views[0]], views[3], color)
    full = _job(m, *BOXES[3], [views[1], views[2]], views[2], color)
    only = _job(m, *BOXES[3], [views[2]], views[2], color)  # the cells the view updates
    hit = (only["d_tsdf"][..., 1] > 0).nonzero()
    assert len(hit)
    x, y, z = (int(v) for v in hit[len(hit) // 2])
    full["d_tsdf"][x, y, z, 1] = 1 << 20
    other_trunc = _job(m, *BOXES[4], [views[3], views[4]], views[4], color, trunc=float(tc.V) * 8, fuse_trunc=None)
    torch.cuda.synchronize()
    return [never, fit(0, 2), fit(1, 0), full, fit(2, 1), fit(3, 4), other_trunc], (0, 3, 6)


def test_unfuse_refused_jobs_between_fitting_ones():
    m = _maps()[0]
    for color in (False, True):
        jobs, refused = _refused_cases(m, color)
        single = [_single(j) for j in jobs]
        # the case cannot go vacuous: the single call refuses exactly these jobs and applies exactly the others
        assert [i for i, (_, s) in enumerate(single) if s] == list(refused), color
        for i, (w, s) in enumerate(single):
            misfits, updates = (int(x) for x in np.frombuffer(w[2], np.uint64)[[4, 1]])
            assert (misfits > 0 and updates == 0) if s else (misfits == 0 and updates > 0), (i, color)
        for results in ("host", "device"):
            _check(m, jobs, ("verdicts", color, results), results)
        got, _ = _many(m, jobs)
        for i in refused:  # no byte of a refused job's volumes or of the guards around them has changed
            before = _state(jobs[i])
            assert got[i][0] == before[0] and got[i][1] == before[1], (i, color)
        for i in set(range(len(jobs))) - set(refused):  # the neighbours are applied
            assert got[i][0] != _state(jobs[i])[0], (i, color)


def test_unfuse_results_on_either_side_and_none():
    """Results in device and in host memory are the same bytes; without results the volumes and the jobs' own records are the same."""
    m = _maps()[0]
    jobs, _ = _refused_cases(m, True)
    host_state, host = _many(m, jobs, "host")
    dev_state, dev = _many(m, jobs, "device")
    none_state, none = _many(m, jobs, None)
    assert host == dev and none is None
    assert host_state == dev_state == none_state
    # the record a job names itself holds the result's info
    for s, (info, _) in zip(host_state, host):
        assert s[2] == info


def test_unfuse_everything_leaves_zero_volumes():
    m = _maps()[0]
    for color in (False, True):
        views = _raw_views(color)
        jobs = [_job(m, lo, n, [views[i], views[(i + 2) % 5]], views[i], color) for i, (lo, n) in enumerate(BOXES)]
        args = [{k: v for k, v in j.items() if k != "whole"} for j in jobs]
        first = m.unfuse_many_into(args, wait=True)
        second = m.unfuse_many_into([dict(a, view=_device_view(views[(i + 2) % 5], color)) for i, a in enumerate(args)], wait=True)
        assert all(s == 0 for _, s in first + second)
        for j, (info, _) in zip(jobs, second):
            assert not j["d_tsdf"].any() and (not color or not j["d_color"].any())
            assert info["cells_weighted"] == 0 and info["cells_colored"] == 0 and info["updates"] > 0


# ------------------------------------------------------------------------------------------------------------ argument errors --
def test_unfuse_argument_errors_write_nothing():
    """Every argument error is of the whole call, before anything is enqueued: sentinel-filled volumes, records and results stay."""
    import torch
    mv = _maps()[0]
    L = _lib.lib()
    views = _raw_views(True)
    other = api.VoxelMap(api.CameraPyr(cc.settings320()), tc.V)  # a map of another context
    host_depth = np.ascontiguousarray(views[0][0], F)
    skew = np.eye(4, dtype=F)
    skew[0, 1] = 0.01

    def jobs():
        js = [_job(mv, *BOXES[2], [], views[0], True), _job(mv, *BOXES[3], [], views[1][:3], False)]
        for j in js:
            for w in j["whole"]:
                if w is not None:
                    w.fill_(SENT)
        return js

    def table(js):
        """The revo_map_tsdf_unfuse_job array of the jobs, as unfuse_many_into builds it."""
        fj, n, keep = mv._fuse_jobs([{k: v for k, v in j.items() if k != "whole"} for j in js])
        arr = (MapTsdfUnfuseJob * n)()
        for a, f in zip(arr, fj):
            for name, _t in MapTsdfUnfuseJob._fields_:
                setattr(a, name, getattr(f, name))
        return arr, n, keep

    def refused(mutate, n_jobs=None, what="", device_out=1, results="device"):
        js = jobs()
        d_res = torch.full((20 * 2 + 4,), 9, dtype=torch.int32, device="cuda")
        h_res = (MapTsdfUnfuseResult * 2)()
        C.memset(h_res, 0x2B, C.sizeof(h_res))
        before = [_state(j) for j in js]
        arr, n, keep = table(js)
        keep.append(mutate(arr, js))
        res = {"device": vp(d_res.data_ptr()), "misaligned": vp(d_res.data_ptr() + 8), "host": C.cast(h_res, vp), "host as device": C.cast(h_res, vp)}[results]
        code = L.revo_map_tsdf_unfuse_many(mv._h, n if n_jobs is None else n_jobs, arr, res, device_out)
        mv.sync()
        assert code == INVALID_ARG, (what, code)
        assert [_state(j) for j in js] == before, what
        assert bool((d_res == 9).all()) and bytes(h_res) == b"\x2b" * C.sizeof(h_res), what

    def overlap(arr, js):
        arr[1].tsdf = arr[0].tsdf + 8 * 16  # inside job 0's volume, 16-byte aligned

    def overlap_colour(arr, js):
        arr[1].color, arr[1].bgr = arr[0].color + 16, arr[0].bgr

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

    nothing = lambda arr, js: None  # noqa: E731
    refused(overlap, what="overlapping TSDF volumes")
    refused(overlap_colour, what="overlapping colour volumes")
    refused(view_(0, depth=host_depth.ctypes.data), what="a host depth image")
    refused(set_(0, bgr=np.zeros((12, 16, 3), np.uint8).ctypes.data), what="a host colour image")
    refused(set_(1, map=other._h), what="another context's map")
    refused(view_(1, T_w_c=np.ascontiguousarray(skew.T).reshape(16).tolist()), what="a view pose that is no rotation")
    refused(view_(0, T_w_c=[float("nan")] * 16), what="a view pose that is not finite")
    refused(nothing, n_jobs=0, what="no job")
    refused(nothing, n_jobs=1025, what="1025 jobs")
    refused(set_(0, tsdf=None), what="a NULL volume")
    refused(set_(1, trunc=-1.0), what="a negative trunc")
    refused(set_(1, trunc=float("nan")), what="a trunc that is no number")
    refused(set_(1, reserved=1), what="a reserved word")
    refused(set_(0, bgr=None), what="a raw colour view without its image")
    refused(set_(1, bgr=1 << 20), what="an image without a colour volume")
    refused(view_(0, width=0), what="a view rule")
    refused(lambda arr, js: setattr(arr[1].box, "n", (C.c_int32 * 3)(0, 8, 8)), what="a box rule")
    refused(lambda arr, js: setattr(arr[0], "tsdf", arr[0].tsdf + 8), what="a misaligned volume")
    refused(lambda arr, js: setattr(arr[0], "info", arr[0].info + 8), what="a misaligned info record")
    refused(set_(1, view_info=host_depth.ctypes.data), what="a host view_info record")
    refused(nothing, device_out=2, what="device_out outside 0 / 1")
    refused(nothing, device_out=-1, results="host", what="device_out below 0")
    refused(nothing, results="misaligned", what="misaligned device results")
    refused(nothing, results="host as device", what="host results given as device results")
    arr, n, keep = table(jobs())
    assert L.revo_map_tsdf_unfuse_many(None, 1, arr, None, 0) == INVALID_ARG and L.revo_map_tsdf_unfuse_many(mv._h, 1, None, None, 0) == INVALID_ARG
    # and the same jobs untouched are taken: empty volumes do not hold the views, so both jobs are refused per job, not as a call
    js = jobs()
    for j in js:
        j["d_tsdf"].zero_()
        if j["d_color"] is not None:
            j["d_color"].zero_()
    want = _check(mv, js, "accepted")
    assert [s for _, s in want] == [INVALID_ARG, INVALID_ARG]
    with pytest.raises(ValueError):
        mv.unfuse_many_into([dict({k: v for k, v in js[0].items() if k != "whole"}, view=(host_depth,) + tuple(js[0]["view"][1:]))])  # the API's own: host images
    other.close()


# ------------------------------------------------------------------------------------------------------------------ api calls --
def _dev_views():
    return [(ms._cuda(v[0]), v[1], v[2], ms._cuda(v[3])) for v in _raw_views(True)]


def _same(a, b):
    va, vb = a.volume(), b.volume()
    return va.cells.tobytes() == vb.cells.tobytes() and va.color.tobytes() == vb.color.tobytes() and a.views == b.views and a.view_counts() == b.view_counts()


def test_unfuse_surfaces_and_repose_surfaces_against_remove_and_repose():
    mv = _maps()[0]
    views = _dev_views()
    a = [api.SurfaceVolume(mv, lo, n) for lo, n in BOXES[2:5]]
    b = [api.SurfaceVolume(mv, lo, n) for lo, n in BOXES[2:5]]
    for s in a + b:
        for v in views[:3]:
            s.integrate(v)
    # surface 1 is asked for a view it does not hold: refused, unchanged, and its neighbours are applied
    asked = [views[1], views[4], views[0]]
    res = api.unfuse_surfaces(list(zip(a, asked)))
    assert [s for _, s in res] == [0, INVALID_ARG, 0]
    for i, (s, v) in enumerate(zip(b, asked)):
        if i == 1:
            with pytest.raises(RevoError) as e:
                s.remove(v)
            assert e.value.info == res[i][0] and res[i][0]["misfits"] > 0
        else:
            assert s.remove(v) == res[i][0]
    assert all(_same(s, t) for s, t in zip(a, b)) and [s.views for s in a] == [2, 3, 2]
    # repose: a view moved to another pose; surface 1 names the view it does not hold: refused, not fused, unchanged
    T_new = np.array(views[3][1], F)
    quads = [(a[0], views[0], views[0][1], T_new), (a[1], views[4], views[4][1], T_new), (a[2], views[2], views[2][1], T_new)]
    res = api.repose_surfaces(quads)
    assert [s for _, s in res] == [0, INVALID_ARG, 0]
    for (_, v, T_old, T_n), t, (info, _) in zip(quads, b, res):
        assert t.repose(v, T_old, T_n) == info
    assert all(_same(s, t) for s, t in zip(a, b))


def test_fuse_surfaces_honours_windows():
    """api.fuse_surfaces with SurfaceWindows of windows 1 and 3 (and a plain SurfaceVolume beside them) over 5 views: after every step
    each surface is what its own integrate leaves, held views included."""
    mv = _maps()[0]
    views = _dev_views()
    make = lambda: [api.SurfaceWindow(mv, *BOXES[2], window=1), api.SurfaceWindow(mv, *BOXES[3], window=3), api.SurfaceVolume(mv, *BOXES[4])]  # noqa: E731
    a, b = make(), make()
    for step in range(5):
        api.fuse_surfaces([(s, views[(step + i) % 5]) for i, s in enumerate(a)])
        for i, s in enumerate(b):
            s.integrate(views[(step + i) % 5])
        assert all(_same(s, t) for s, t in zip(a, b)), step
        assert [s.views for s in a] == [1, min(step + 1, 3), step + 1]
        for s, t in zip(a[:2], b[:2]):
            assert len(s.held_views()) == len(t.held_views()) == s.views
            assert all(x[1].tobytes() == y[1].tobytes() and all(p.cpu().numpy().tobytes() == q.cpu().numpy().tobytes() for p, q in ((x[0], y[0]), (x[3], y[3])))
                       for x, y in zip(s.held_views(), t.held_views()))  # the bytes: a depth image may hold NaNs
    # a window's surface is a fresh fuse of the views it holds
    fresh = api.SurfaceVolume(mv, *BOXES[3])
    for v in a[1].held_views():
        fresh.integrate(v)
    assert fresh.volume().cells.tobytes() == a[1].volume().cells.tobytes() and fresh.volume().color.tobytes() == a[1].volume().color.tobytes()


def test_fuse_surfaces_refused_eviction_keeps_the_view_and_raises_behind_every_job():
    """A window whose oldest view cannot be taken out (a cell at the full weight) holds window + 1 views afterwards, as after
    SurfaceWindow.integrate; the other window of the call is evicted all the same, and the error comes behind both."""
    mv = _maps()[0]
    views = _dev_views()
    a = [api.SurfaceWindow(mv, *BOXES[3], window=1), api.SurfaceWindow(mv, *BOXES[2], window=1)]
    b = [api.SurfaceWindow(mv, *BOXES[3], window=1), api.SurfaceWindow(mv, *BOXES[2], window=1)]
    for s in a + b:
        s.integrate(views[2])
    hit = (a[0].d_tsdf[..., 1] > 0).nonzero()
    x, y, z = (int(v) for v in hit[len(hit) // 2])
    for s in (a[0], b[0]):
        s.map.sync()
        s.d_tsdf[x, y, z, 1] = 1 << 20
    with pytest.raises(RevoError) as e:
        api.fuse_surfaces([(s, views[1]) for s in a])
    assert [w for w, _ in e.value.refused] == [a[0]] and e.value.misfits > 0
    with pytest.raises(RevoError):
        b[0].integrate(views[1])
    b[1].integrate(views[1])
    assert [s.views for s in a] == [2, 1] and all(_same(s, t) for s, t in zip(a, b))


# --------------------------------------------------------------------------------------------------------------- the driver --
# The late keyframes of test_gpu_multi_surface's sequences see no cell of a box around the first camera (the tracker has lost the scene
# by then: that test wants LOST tracks), and a window of two such views is an empty volume.  So the box is 3.2 m around the first
# camera, and every sequence is cut in front of its first keyframe that updates no cell of it.
WINDOW_BOX = dict(lo=(-32, -32, 0), n=(64, 64, 64))


@functools.lru_cache(maxsize=None)
def _window_sequences():
    """test_gpu_multi_surface's three sequences, each up to the frame of its first keyframe that sees nothing of WINDOW_BOX: that frame is
    tracked and never promoted (a keyframe is promoted by the frame behind it).  Tracking is causal, so the keyframes of a cut sequence
    are the first ones of the whole."""
    from lm_settings_cases import S160
    full = ms._single_driver(False)
    vm = api.VoxelMap(api.CameraPyr(S160), ms.DRIVER_VOXEL, dense=True)
    out = []
    for frames, s in zip(ms._driver_sequences(), full):
        assert s["skipped"] == 0
        probe = api.SurfaceVolume(vm, **WINDOW_BOX)
        for _, T, d, bgr in s["kfs"]:
            probe.integrate((ms._cuda(d), T, None, ms._cuda(bgr)))
        blind = [k for k, c in enumerate(probe.view_counts()) if c["free"] + c["confirmed"] == 0]
        out.append(list(frames) if not blind else [f for f in frames if float(f[2]) <= s["kfs"][blind[0]][0]])
    vm.close()
    return out


def _sequential_windows(track):
    """vo.REVO(voxelMap=MapWindow, surface=SurfaceWindow(window=2)) on each of test_gpu_multi_surface's sequences alone -> per sequence
    the volumes' bytes, the fused keyframes [(depth, T_fused, None, bgr)], the per-view counts and the poses."""
    from lm_settings_cases import S160
    from revo_amd import vo
    out = []
    for frames in _window_sequences():
        cam = api.CameraPyr(S160)
        win = api.MapWindow(cam, ms.DRIVER_VOXEL, dense=True, window=2)
        surf = api.SurfaceWindow(win, window=2, **WINDOW_BOX)
        g = vo.REVO(S160, cameraPyr=cam, voxelMap=win, surface=surf, surface_track=True if track else None)
        by_ts = {float(f[2]): f[0] for f in frames}
        kfs = []
        for f in frames:
            _, kf = g.push(f[0], f[1], f[2])
            if kf:
                pyr, T = g.keyframe()
                T = np.array(g.surface_tracks[-1][2] if track else T, F)  # the pose it was fused at
                kfs.append((pyr.returnDepth(0).copy(), T, None, np.ascontiguousarray(by_ts[float(pyr.returnTimestamp())])))
        out.append(dict(volume=ms._volume_bytes(surf), kfs=kfs, counts=surf.view_counts(), views=surf.views, skipped=g.surface_skipped,
                        poses=[(ts_, T.copy()) for ts_, T in g.poses], tracks=list(g.surface_tracks)))
        win.close()
    return out


@pytest.mark.parametrize("track", (False, True))
def test_the_driver_keeps_a_window_per_stream(track, monkeypatch):
    """MultiREVO with 3 streams (test_gpu_multi_surface's sequences, see _window_sequences) and surface=dict(..., window=2): per stream the volumes are byte for byte those of the sequential driver
    with a MapWindow and a SurfaceWindow(window=2) on that sequence alone, and those of a fresh fuse of its last two fused keyframes at
    their T_fused; two views are held and fused - 2 were evicted, none refused.  With tracking the keyframes are tracked against the
    windowed surface as it stands, so the same holds.  Under SAME_PARTITION, which makes the two drivers' poses equal."""
    from lm_settings_cases import S160
    from revo_amd import vo
    from test_gpu_configs import SAME_PARTITION
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    single = _sequential_windows(track)
    for i, s in enumerate(single):  # the window must evict at least once per stream
        print("sequence", i, "keyframes fused", len(s["kfs"]), "skipped", s["skipped"], "the held views' counts", s["counts"])
        assert len(s["kfs"]) >= 3 and s["skipped"] == 0 and s["views"] == 2, i
        # the comparison cannot pass on empty volumes: both held views update cells of the box, and confirm some
        assert all(c["free"] + c["confirmed"] > 0 for c in s["counts"]) and any(c["confirmed"] > 0 for c in s["counts"]), i
    mv = vo.MultiREVO(S160, 3, map_voxel=ms.DRIVER_VOXEL, map_dense=True, surface=dict(WINDOW_BOX, window=2), surface_track=True if track else None)
    res = mv.run(_window_sequences())
    for i, (r, s) in enumerate(zip(res, single)):
        assert len(r.poses) == len(s["poses"]) and all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(r.poses, s["poses"])), i
        assert ms._volume_bytes(r.surface) == s["volume"], ("the sequential window", i)
        fresh = api.SurfaceVolume(r.map, **WINDOW_BOX)
        for d, T, _, bgr in s["kfs"][-2:]:
            fresh.integrate((ms._cuda(d), T, None, ms._cuda(bgr)))
        assert ms._volume_bytes(r.surface) == ms._volume_bytes(fresh), ("a fresh fuse of the last two", i)
        assert any(s["volume"][0]) and any(s["volume"][1])
        fused = len(s["kfs"])
        assert r.surface.views == 2 and r.surface_evictions == fused - 2 and r.surface_evictions_refused == 0 and r.surface_skipped == 0, i
        assert r.surface.view_counts() == s["counts"] == fresh.view_counts(), i
        if track:
            assert ms._tracks_bytes(r.surface_tracks) == ms._tracks_bytes(s["tracks"]), i
    for r in res:
        r.map.close()


def test_the_window_of_a_stream_by_hand():
    """attach_surface(window=): the report before and behind the first eviction, the rules of the two calls, and what frees the window."""
    from lm_settings_cases import S160
    from revo_amd import vo
    L = _lib.lib()
    frames = ms._driver_sequences()[0]
    mv = vo.MultiREVO(S160, 2)
    vms = [api.VoxelMap(mv.camPyr, ms.DRIVER_VOXEL, dense=True) for _ in range(2)]
    surfs = [api.SurfaceVolume(vm, **ms.DRIVER_BOX) for vm in vms]
    assert L.revo_vo_multi_surface_window(mv._h, 0, 1) == INVALID_ARG  # no surface attached
    with pytest.raises(ValueError) as e:
        mv.attach_surface(0, api.SurfaceWindow(vms[0], window=2, **ms.DRIVER_BOX))
    assert "window=" in str(e.value)
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            mv.attach_surface(0, surfs[0], window=bad)
    for s in range(2):
        mv.attach_map(s, vms[s])
    mv.attach_surface(0, surfs[0], window=1)
    mv.attach_surface(1, surfs[1])  # without a window, as before
    assert L.revo_vo_multi_surface_window(mv._h, 0, 1025) == INVALID_ARG and L.revo_vo_multi_surface_window(mv._h, 0, -1) == INVALID_ARG
    assert L.revo_vo_multi_surface_window(mv._h, 2, 1) == INVALID_ARG
    with pytest.raises(RevoError):
        mv.surface_window_last(1)  # no window on this stream
    rep = mv.surface_window_last(0)
    assert (rep.window, rep.held, rep.evictions, rep.evicted.status) == (1, 0, 0, 0) and not any(bytes(rep.evicted))
    first_kf_ts = None
    for f in frames:
        mv.submit([(0, f[0], f[1], f[2]), (1, f[0], f[1], f[2])])
        mv.step()
        if first_kf_ts is None and mv.nKeyFrames(0) == 1:
            first_kf_ts = float(f[2])
            rep = mv.surface_window_last(0)
            assert (rep.held, rep.evictions) == (1, 0) and surfs[0].views == 1
        if mv.nKeyFrames(0) == 2:  # the step that promotes the second keyframe fuses it, keeps it and evicts the first
            break
    assert mv.nKeyFrames(0) == 2 == mv.nKeyFrames(1)
    rep = mv.surface_window_last(0)
    assert (rep.window, rep.held, rep.evictions, rep.evicted.status) == (1, 1, 1, 0) and rep.evicted_timestamp == first_kf_ts
    assert rep.evicted.info.updates > 0 and rep.evicted.info.misfits == 0 and rep.evicted.info.cells == 32 ** 3
    assert surfs[0].views == 1 and surfs[1].views == 2 and surfs[0].surface_evictions == 1 and surfs[0].surface_evictions_refused == 0
    # stream 0 holds its second keyframe alone; stream 1, which saw the same frames, holds both
    a, b = ms._volume_bytes(surfs[0]), ms._volume_bytes(surfs[1])
    assert a != b and any(a[0])
    assert int((surfs[0].volume().cells["weight"] > 1).sum()) == 0 and int((surfs[1].volume().cells["weight"] > 1).sum()) > 0
    # detaching frees the window; a new attachment starts without one
    mv.attach_surface(0, None)
    mv.attach_surface(0, surfs[0])
    with pytest.raises(RevoError):
        mv.surface_window_last(0)
    del mv
    for vm in vms:
        vm.close()
