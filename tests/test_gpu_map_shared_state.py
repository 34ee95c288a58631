"""The buffers, descriptor staging and timing events that revo_map_render and revo_map_raycast share a type for
(revo_internal.h: DevBuf, HostRows, EventTimer) on ONE handle, features interleaved and view counts growing and shrinking: every
output is byte for byte what the same call gives alone on a fresh handle holding the same records, each *_last_ms call answers
once its own feature has run and refuses before.  Hand-made map (about 480 voxels in a 1 024-slot table), 64 x 48 views."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile, synth  # noqa: E402

import map_carve_cases as cc  # noqa: E402

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
