"""The buffers, descriptor staging and timing events that revo_map_render and revo_map_raycast share a type for
(revo_internal.h: DevBuf, HostRows, EventTimer) on ONE handle, features interleaved and view counts growing and shrinking: every
output is byte for byte what the same call gives alone on a fresh handle holding the same records, each *_last_ms call answers
once its own feature has run and refuses before.  Hand-made map (about 480 voxels in a 1 024-slot table), 64 x 48 views.

Behind it the same demand on every feature that keeps scratch on the handle (map_shared_cases.py: the distance field and its
users, planning, known space, view gain, the TSDF calls, registration), along one fixed schedule and three random ones with the
record set changing on the way; the timing queries across all of them; and the wait=False device forms back to back."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile, synth  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_shared_cases as sc  # noqa: E402

F = np.float32
RAW = mapfile.RAW_DTYPE
INVALID_ARG = -1
W, H = 64, 48
CAM = (16.0, 16.0, 32.0, 24.0, W, H)
ZR = (cc.ZMIN, cc.ZMAX)
POSES = [synth.se3_exp(np.asarray(t, np.float64)).astype(F) for t in cc.TWISTS + ((0.02, -0.04, 0.01, 0.02, 0.0, -0.03),)]


def _fresh(*record_sets):
    from revo_amd import api
    m = api.VoxelMap(api.CameraPyr(cc.settings320()), cc.VOXEL, initial_voxels=1)
    for rec in record_sets:
        m.merge_raw(rec.astype(RAW))
    return m


def _render(m, n):
    d, b, c = m.render(POSES[:n], camera=CAM, zrange=ZR)
    return [x.tobytes() for x in d] + [x.tobytes() for x in b] + [tuple(c)]


def _render_device(m, n):
    import torch
    dev = "cuda:%d" % m.cameraPyr.device
    d = torch.full((n, H, W), -1.0, dtype=torch.float32, device=dev)
    b = torch.full((n, H, W, 3), 7, dtype=torch.uint8, device=dev)
    c = torch.full((n,), -1, dtype=torch.int32, device=dev)
    m.render_into(d, b, POSES[:n], camera=CAM, zrange=ZR, d_covered=c)
    return [t.cpu().numpy().tobytes() for t in (d, b, c)]


def _raycast(m, n):
    d, b, h, k = m.raycast(POSES[:n], camera=CAM, zrange=ZR, keys=True)
    return [x.tobytes() for x in d] + [x.tobytes() for x in b] + [x.tobytes() for x in k] + [tuple(h), sorted(m.ray_info.items())]


def _raycast_device(m, n):
    import torch
    dev = "cuda:%d" % m.cameraPyr.device
    d = torch.full((n, H, W), -1.0, dtype=torch.float32, device=dev)
    b = torch.full((n, H, W, 3), 7, dtype=torch.uint8, device=dev)
    k = torch.full((n, H, W), 5, dtype=torch.int64, device=dev)
    h = torch.full((n,), -1, dtype=torch.int32, device=dev)
    i = torch.full((64,), 9, dtype=torch.uint8, device=dev)
    m.raycast_into(d, b, POSES[:n], camera=CAM, zrange=ZR, d_keys=k, d_hits=h, d_info=i)
    return [t.cpu().numpy().tobytes() for t in (d, b, k, h, i)]


def _carve_eval(m):
    k = CAM[:4] + ZR
    views = [(np.full((H, W), 2.0, F), POSES[0], k), (np.full((H, W), 1.5, F), POSES[1], k)]
    rec, info, vinfo = m.carve_eval(views)
    assert info["voxels_carved"] > 0 and len(rec) == info["voxels_carved"]
    return [rec.tobytes(), sorted(info.items()), [sorted(v.items()) for v in vinfo]]


def _pose_raw(m):
    rec, info = m.pose_raw(POSES[2], voxel=2 * cc.VOXEL)
    assert info["voxels_moved"] > 0
    return [rec.tobytes(), sorted(info.items())]


def _last_ms(m, which):
    """-> (return code, milliseconds) of revo_map_render_last_ms / revo_map_raycast_last_ms."""
    from revo_amd import _lib
    ms = C.c_float(float("nan"))
    return getattr(_lib.lib(), "revo_map_%s_last_ms" % which)(m._h, C.byref(ms)), ms.value


def _timed(m, which):
    rc, ms = _last_ms(m, which)
    return rc == 0 and math.isfinite(ms) and ms > 0


def test_features_interleaved_on_one_handle():
    rec = cc.filled_records()
    more = cc.free_grid(600)  # with the 480 held: past the 1 024-slot table's load of 0.5
    m = _fresh(rec)
    assert m.info()["capacity"] == 1024 and m.info()["rehashes"] == 0
    assert _last_ms(m, "render")[0] == INVALID_ARG and _last_ms(m, "raycast")[0] == INVALID_ARG

    def same(call, *args, records=(rec,)):
        got, want = call(m, *args), call(_fresh(*records), *args)
        assert got == want, "%s%r differs from the call alone on a fresh handle" % (call.__name__, args)

    same(_render, 1)
    assert _timed(m, "render") and _last_ms(m, "raycast")[0] == INVALID_ARG  # its own feature has not run
    same(_raycast, 3)
    assert _timed(m, "raycast") and _timed(m, "render")
    same(_render_device, 5)
    same(_carve_eval)
    same(_raycast_device, 2)
    same(_pose_raw)
    same(_render, 1)
    m.merge_raw(more.astype(RAW))
    assert m.info()["rehashes"] == 1 and m.info()["capacity"] > 1024
    same(_render, 1, records=(rec, more))
    same(_raycast, 1, records=(rec, more))
    assert _timed(m, "render") and _timed(m, "raycast")

    only_rays = _fresh(rec)  # the other way round: a handle that has cast but never rendered
    _raycast(only_rays, 1)
    assert _timed(only_rays, "raycast") and _last_ms(only_rays, "render")[0] == INVALID_ARG


# ------------------------------------------------------------------------- every feature of the handle (map_shared_cases) --
@functools.lru_cache(maxsize=None)
def _context():
    from revo_amd import api
    return api.CameraPyr(cc.settings320())


def _handle(mutations=()):
    """A fresh handle holding the base records, with `mutations` replayed onto it."""
    from revo_amd import api
    m = api.VoxelMap(_context(), sc.VOXEL, initial_voxels=1)
    m.merge_raw(sc.base_records())
    for name in mutations:
        sc.MUTATIONS[name](m)
    return m


def _close(m):
    if getattr(m, "_shared_source", None) is not None:
        m._shared_source.close()
    m.close()


_ALONE = {}  # (feature, size, mutations so far) -> the comparable of the call alone: computed once, shared by the tests below


def _alone(name, size, prefix=()):
    key = (name, size, prefix)
    if key not in _ALONE:
        ref = _handle(prefix)
        _ALONE[key] = sc.FEATURES[name](ref, size)
        _close(ref)
    return _ALONE[key]


def _say(step):
    return "%s(%s)" % step[1:] if step[0] == "call" else "mutation %s" % step[1]


def _run(steps):
    m = _handle()
    assert m.info()["capacity"] == 1024 and m.info()["rehashes"] == 0
    prefix, infos = (), {}
    for i, step in enumerate(steps):
        if step[0] == "mutate":
            sc.MUTATIONS[step[1]](m)
            prefix += (step[1],)
            infos.setdefault(step[1], m.info())  # behind its first run
            continue
        got, want = sc.FEATURES[step[1]](m, step[2]), _alone(step[1], step[2], prefix)
        assert got == want, "step %d: %s differs from the call alone on a fresh handle with the mutations %s replayed; before it: %s" % (
            i, _say(step), list(prefix), ", then ".join(_say(x) for x in steps[max(i - 2, 0):i]) or "nothing")
    _close(m)
    return prefix, infos


def test_every_feature_interleaved_scripted():
    prefix, infos = _run(sc.scripted())
    assert prefix == tuple(sc.MUTATIONS)
    grown, less, carved = (infos[k] for k in ("merge_grow", "subtract_part", "carve_view"))
    assert grown["rehashes"] == 1 and grown["capacity"] > 1024  # the table every later call reads is another one
    assert grown["voxels"] > less["voxels"] > carved["voxels"] > 0 and infos["clear_merge"]["voxels"] == len(sc.base_records())


@pytest.mark.parametrize("seed", sc.RANDOM_SEEDS)
def test_every_feature_interleaved_random(seed):
    _run(sc.random_schedule(seed, sc.RANDOM_LENGTH))


# query -> the features whose entry points own its events
OWNERS = {"render": ("render", "render_into"), "raycast": ("raycast", "raycast_into", "cast_rays", "cast_rays_device"),
          "distance_field": ("distance_field", "distance_field_into"), "plan": ("plan", "plan_into")}


def _query(m, which):
    """-> (return code, milliseconds) of revo_map_render_last_ms / _raycast_last_ms / _distance_field_last_ms / revo_map_plan_last."""
    if which != "plan":
        return _last_ms(m, which)
    from revo_amd import _lib
    ms, rounds = C.c_float(float("nan")), C.c_uint32()
    return _lib.lib().revo_map_plan_last(m._h, C.byref(ms), C.byref(rounds)), ms.value


def _answers(m, which):
    rc, ms = _query(m, which)
    return rc == 0 and math.isfinite(ms) and ms > 0


def test_timing_queries_answer_for_their_own_feature_only():
    owned = {f for fs in OWNERS.values() for f in fs}
    m = _handle()
    assert all(_query(m, q)[0] == INVALID_ARG for q in OWNERS)
    # every other feature of the schedule first -- the ones that run another feature's kernels or share its buffers in front:
    # view_gain marches with the ray cast's kernels, the known-space calls build the distance field's bit volume, plan_paths
    # walks a loaded cost field
    others = ["view_gain", "view_gain_into", "frontiers", "frontiers_into", "known_field", "known_field_into", "observe", "observe_into", "plan_paths",
              "plan_paths_into"]
    others += [f for f in sc.FEATURES if f not in owned and f not in others]
    for name in others:
        sc.FEATURES[name](m, "small")
        for q in OWNERS:
            assert _query(m, q)[0] == INVALID_ARG, "revo_map_%s's timing query answers after %s alone" % (q, name)
    # then each query's own feature: it answers, the ones whose feature has not run still refuse
    for i, q in enumerate(OWNERS):
        sc.FEATURES[OWNERS[q][0]](m, "small")
        assert _answers(m, q), q
        assert all(_query(m, later)[0] == INVALID_ARG for later in list(OWNERS)[i + 1:]), q
    # and a call of another feature behind it leaves the query with the call it describes: the gain's march records into no
    # event of the ray cast's (on a handle that has never cast the query went on refusing above), nor do the others
    for name in ("view_gain", "view_gain_into", "known_field_into", "frontiers", "plan_paths"):
        sc.FEATURES[name](m, "large")
        assert all(_answers(m, q) for q in OWNERS), name
    _close(m)
    for q, features in OWNERS.items():  # every owning form, each on a handle of its own
        for name in features:
            m = _handle()
            assert _query(m, q)[0] == INVALID_ARG
            sc.FEATURES[name](m, "small")
            assert _answers(m, q) and all(_query(m, o)[0] == INVALID_ARG for o in OWNERS if o != q), name
            _close(m)


def test_wait_false_forms_in_stream_order():
    m = _handle()
    jobs = []
    for j, name in enumerate(sc.NO_WAIT + sc.NO_WAIT):  # an odd number of forms: each comes once large and once small
        size = ("large", "small")[j % 2]
        jobs.append((name, size) + sc.FEATURES[name].args(m, size))  # every tensor of every call exists before the first call
    for name, size, out, call in jobs:
        call(False)
    m.sync()
    for j, (name, size, out, call) in enumerate(jobs):
        assert [sc._b(x) for x in out] == _alone(name, size), "call %d, %s(%s), differs from the waited call alone on a fresh handle" % (j, name, size)
    _close(m)
