"""Schedules for the shared-state tests of the voxel map (test_map_shared_cases_cpu.py, test_gpu_map_shared_state.py): every
feature that keeps scratch on the map handle (struct revo_map, revo_map_impl.h) as a function (map, size) -> comparable, the
calls that change the record set, which member of the handle which features go through, and the orders in which one handle
runs them.  The GPU test demands of every call the comparable of the same call on a fresh handle that has only had the
mutations so far replayed.  No GPU and no torch at import: a feature imports what it needs when it is called.

One map for all of it: map_carve_cases' hand-made voxels (2 cm, about 480 in a 1 024-slot table) with a cluster inside the boxes
below, so that fields, frontiers and predicted views have something to show.  Inputs that another call would have made (a seen
volume, a field, a cost field, a TSDF volume) come from revo_amd.mapfile's restatements, once per size: a feature's input then
never depends on the handle under test.  Two sizes per feature, "large" needing strictly more bytes than "small" in every
buffer whose size a call chooses (bkeys follows the map's table and grows with the rehash instead).  Test infrastructure only."""
import functools
import random
import re

import numpy as np

from revo_amd import mapfile, synth

import map_carve_cases as cc

F = np.float32
RAW = mapfile.RAW_DTYPE
VOXEL = cc.VOXEL
ZR = (cc.ZMIN, cc.ZMAX)
SIZES = ("small", "large")
NV = {"small": 1, "large": 5}  # views or poses of a call
POSES = [synth.se3_exp(np.asarray(t, np.float64)).astype(F) for t in cc.TWISTS + ((0.02, -0.04, 0.01, 0.02, 0.0, -0.03),)]
# the camera the whole map is seen through (render, raycast, carve_eval), and the one that looks at the boxes (observe, fuse,
# view_gain, the surface views): (fx, fy, cx, cy), (width, height)
MAP_CAM = {"small": ((6.0, 6.0, 12.0, 8.0), (24, 16)), "large": ((16.0, 16.0, 32.0, 24.0), (64, 48))}
BOX_CAM = {"small": ((32.0, 32.0, 12.0, 8.0), (24, 16)), "large": ((48.0, 48.0, 32.0, 24.0), (64, 48))}
# lo, n: around the optical axis at a depth of 1 m; neither z length is a multiple of 32
BOX = {"small": ((-4, -3, 48), (9, 7, 5)), "large": ((-16, -10, 45), (33, 20, 11))}
GAIN_POSES = 65  # one more than GAIN_CHUNK (revo_gain_host.h): view_gain_into's large call takes two launches
MISS_DEPTH = {"small": 0.0, "large": 1.5}  # view_gain: a miss is a depth hole, or free space seen up to 1.5 m (k_gain_fill_miss runs)
SENTINEL = 7


# ------------------------------------------------------------------------------------------------------------- inputs --
def _cluster(n=60, seed=23):
    """Voxels inside the large box, the first 20 inside the small one, at their cells' centres rounded to the 2^-20 m grid."""
    rng = np.random.default_rng(seed)
    cells = set()
    for size, want in (("small", 20), ("large", n)):
        lo, nn = BOX[size]
        while len(cells) < want:
            cells.add(tuple(int(a + rng.integers(0, b)) for a, b in zip(lo, nn)))
    rows = [cc._row(np.rint((np.asarray(c) + 0.5) * VOXEL * 2.0 ** 20) / 2.0 ** 20, int(rng.integers(1, 4))) for c in sorted(cells)]
    rec = cc.pack(rows)[0]
    assert sorted(map(tuple, mapfile.key_axes(rec["key"]).tolist())) == sorted(cells)
    return rec


@functools.lru_cache(maxsize=None)
def base_records():
    """What every handle starts from: 484 records, a load just under 0.5 of 1 024 slots."""
    rec = np.concatenate([cc.filled_records(n_fill=400).astype(RAW), _cluster().astype(RAW)])
    assert len(np.unique(rec["key"])) == len(rec) and 480 <= len(rec) <= 512
    return rec[np.argsort(rec["key"])]


@functools.lru_cache(maxsize=None)
def grid_records():
    """600 voxels at 1 m: with the base records past the 1 024-slot table's load of 0.5."""
    return cc.free_grid(600).astype(RAW)


def _k(cam):
    return tuple(cam[0]) + ZR


@functools.lru_cache(maxsize=None)
def box_views(size):
    """NV[size] raw views of the box: (depth, T_w_c, intrinsics, bgr).  A tilted plane through the box with three holes."""
    (fx, fy, cx, cy), (w, h) = BOX_CAM[size]
    u, v = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    out = []
    for i in range(NV[size]):
        d = (F(1.0) + F(0.004) * (u - F(cx)) + F(0.003) * (v - F(cy)) + F(0.01) * F(i)).astype(F)
        d[2, 3], d[h - 3, w - 4], d[h // 2, 1] = 0.0, np.nan, cc.ZMAX
        bgr = np.stack([(3 * u + 5 * v + 7 * i) % 256, (11 * u + v) % 256, (u + 13 * v + i) % 256], -1).astype(np.uint8)
        out.append((d, POSES[i], _k(BOX_CAM[size]), bgr))
    return out


def _depth_views(size):
    return [v[:3] for v in box_views(size)]


@functools.lru_cache(maxsize=None)
def seen_volume(size):
    return mapfile.observe_records(VOXEL, *BOX[size], _depth_views(size))[0]


@functools.lru_cache(maxsize=None)
def field(size):
    return mapfile.distance_field_records(base_records(), *BOX[size])[0]


def _seeds(size):
    lo, n = BOX[size]
    rel = [(0, 0, 0)] if size == "small" else [(0, 0, 0), (n[0] - 1, n[1] - 1, n[2] - 1), (n[0] // 2, 1, n[2] - 2)]
    return [tuple(a + b for a, b in zip(lo, r)) for r in rel]


@functools.lru_cache(maxsize=None)
def cost_field(size):
    return mapfile.plan_records(field(size), *BOX[size], _seeds(size), 2)[0]


@functools.lru_cache(maxsize=None)
def tsdf_volume(size):
    """-> (cells, colour cells) of the box's views."""
    views = box_views(size)
    r = mapfile.tsdf_records(VOXEL, *BOX[size], [v[:3] for v in views], bgr=[v[3] for v in views])
    return r[0], r[3]


def _points(size, n, seed, pad=0.05):
    lo, nn = BOX[size]
    a, b = np.asarray(lo) * VOXEL, (np.asarray(lo) + nn) * VOXEL
    return np.random.default_rng(seed).uniform(a - pad, b + pad, (n, 3)).astype(F)


def _rays(size):
    n = 64 if size == "small" else 4096
    rng = np.random.default_rng(31)
    o = rng.uniform(-0.2, 0.2, (n, 3)).astype(F)
    d = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), np.ones((n, 1))], 1).astype(F)
    return o, d, F(0.1), F(4.0)


# ------------------------------------------------------------------------------------------------------------ helpers --
def _b(x):
    """bytes of a numpy array, a torch tensor or a ctypes structure."""
    if hasattr(x, "data_ptr"):
        return x.cpu().numpy().tobytes()
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x).tobytes()
    return bytes(x)


def _dev(m):
    return "cuda:%d" % m.cameraPyr.device


def _full(m, shape, dtype, value=SENTINEL):
    import torch
    return torch.full(tuple(shape), value, dtype=dtype, device=_dev(m))


def _to(m, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev(m))


def _info64(m):
    import torch
    return _full(m, (8,), torch.int64, 9)


def _seen(m, size):
    from revo_amd import api
    return api.SeenVolume(seen_volume(size), BOX[size][0], VOXEL)


def _tsdf(m, size, color):
    from revo_amd import api
    cells, col = tsdf_volume(size)
    return api.TsdfVolume(cells, BOX[size][0], VOXEL, mapfile.tsdf_trunc(VOXEL), color=col if color else None)


def _d_tsdf(m, size):
    cells, col = tsdf_volume(size)
    n = BOX[size][1]
    return _to(m, cells.view(np.int32).reshape(n + (2,))), _to(m, col.view(np.uint32).astype(np.int32).reshape(n + (4,)))


def _device_views(m, size, color):
    return [(_to(m, d), T, k) + ((_to(m, bgr),) if color else ()) for d, T, k, bgr in box_views(size)]


def _items(d):
    return sorted(d.items())


def deferred(args):
    """args(m, size) -> (the call's device outputs, call(wait)), with every tensor made before the call -> the feature, which
    waits; test_wait_false_forms_in_stream_order takes .args and issues the calls of several features back to back."""
    @functools.wraps(args)
    def feature(m, size):
        out, call = args(m, size)
        call(True)
        return [_b(x) for x in out]
    feature.args = args
    return feature


# ----------------------------------------------------------------------------------------------------------- features --
def render(m, size):
    cam, wh = MAP_CAM[size]
    d, b, c = m.render(POSES[:NV[size]], camera=cam + wh, zrange=ZR)
    return [_b(x) for x in d] + [_b(x) for x in b] + [tuple(c)]


@deferred
def render_into(m, size):
    import torch
    cam, (w, h) = MAP_CAM[size]
    n = NV[size]
    d, b, c = _full(m, (n, h, w), torch.float32, -1.0), _full(m, (n, h, w, 3), torch.uint8), _full(m, (n,), torch.int32, -1)
    return [d, b, c], lambda wait: m.render_into(d, b, POSES[:n], camera=cam + (w, h), zrange=ZR, d_covered=c, wait=wait)


def raycast(m, size):
    cam, wh = MAP_CAM[size]
    d, b, h, k = m.raycast(POSES[:NV[size]], camera=cam + wh, zrange=ZR, keys=True)
    return [_b(x) for x in d] + [_b(x) for x in b] + [_b(x) for x in k] + [tuple(h), _items(m.ray_info)]


def raycast_into(m, size):
    import torch
    cam, (w, h) = MAP_CAM[size]
    n = NV[size]
    d, b = _full(m, (n, h, w), torch.float32, -1.0), _full(m, (n, h, w, 3), torch.uint8)
    k, hits, i = _full(m, (n, h, w), torch.int64, 5), _full(m, (n,), torch.int32, -1), _full(m, (64,), torch.uint8, 9)
    m.raycast_into(d, b, POSES[:n], camera=cam + (w, h), zrange=ZR, d_keys=k, d_hits=hits, d_info=i)
    return [_b(t) for t in (d, b, k, hits, i)]


def cast_rays(m, size, device=False):
    key, s, cells, status, info = m.cast_rays(*_rays(size), device=device)
    return [_b(key), _b(s), _b(cells), _b(status), _items(info)]


def cast_rays_device(m, size):
    return cast_rays(m, size, device=True)


def carve_eval(m, size):
    cam, (w, h) = MAP_CAM[size]
    views = [(np.full((h, w), z, F), POSES[i], _k(MAP_CAM[size])) for i, z in enumerate((2.0, 1.5)[:1 if size == "small" else 2])]
    rec, info, vinfo = m.carve_eval(views)  # host records: ascending key order
    return [_b(rec), _items(info), [_items(v) for v in vinfo]]


def pose_raw(m, size):
    rec, info = m.pose_raw(POSES[2], voxel=VOXEL if size == "small" else 2 * VOXEL)  # host records: the canonical form
    return [_b(rec), _items(info)]


def bounds(m, size):
    lo, hi, n = m.bounds(min_count=2 if size == "small" else 1)
    return [_b(lo), _b(hi), n]


def distance_field(m, size):
    f = m.distance_field(lo=BOX[size][0], n=BOX[size][1])
    return [_b(f.d2), _items(f.info)]


@deferred
def distance_field_into(m, size):
    import torch
    d, i = _full(m, BOX[size][1], torch.int32), _info64(m)
    return [d, i], lambda wait: m.distance_field_into(d, *BOX[size], d_info=i, wait=wait)


def known_field(m, size):
    f = m.distance_field(seen=_seen(m, size))
    return [_b(f.d2), _items(f.info)]


@deferred
def known_field_into(m, size):
    import torch
    d, i, seen = _full(m, BOX[size][1], torch.int32), _info64(m), _to(m, seen_volume(size))
    return [d, i], lambda wait: m.known_field_into(d, seen, *BOX[size], d_info=i, wait=wait)


def df_sample(m, size):
    from revo_amd import api
    return [_b(m.df_sample(api.DistanceField(field(size), BOX[size][0], VOXEL), _points(size, 20 if size == "small" else 300, 2)))]


@deferred
def sample_into(m, size):
    import torch
    pts = _points(size, 20 if size == "small" else 300, 2)
    out, d2, d_pts = _full(m, (len(pts), 4), torch.float32, -3.0), _to(m, field(size).view(np.int32)), _to(m, pts)
    return [out], lambda wait: m.sample_into(out, d2, BOX[size][0], d_pts, wait=wait)


def _dfa_args(size):
    return _points(size, 30 if size == "small" else 200, 4, pad=0.0), POSES[:NV[size]], 8 * VOXEL


def df_align_eval(m, size):
    pts, poses, max_dist = _dfa_args(size)
    return [_b(r) for r in m.df_align_eval(field(size), BOX[size][0], pts, np.stack(poses), max_dist)]


def df_align_eval_device(m, size):
    import ctypes as C
    import torch
    from revo_amd.settings import MapDfAlignInfo
    pts, poses, max_dist = _dfa_args(size)
    out = _full(m, (len(poses) * C.sizeof(MapDfAlignInfo),), torch.uint8)
    m.df_align_eval(_to(m, field(size).view(np.int32)), BOX[size][0], _to(m, pts), np.stack(poses), max_dist, d_out=out)
    m.sync()
    return [_b(out)]


def plan(m, size):
    from revo_amd import api
    cost, info = m.plan(api.DistanceField(field(size), BOX[size][0], VOXEL), _seeds(size), 2)
    return [_b(cost), _items(info)]  # milliseconds and rounds (revo_map_plan_last) depend on the implementation: left out


def plan_into(m, size):
    import torch
    c, i = _full(m, BOX[size][1], torch.int32), _info64(m)
    m.plan_into(c, _to(m, field(size).view(np.int32)), *BOX[size], _seeds(size), 2, d_info=i)
    return [_b(c), _b(i)]


def _starts(size):
    lo, n = BOX[size]
    rel = [(n[0] - 1, n[1] - 1, n[2] - 1)] if size == "small" else [(n[0] - 1, 0, 0), (5, 7, 3), (20, 15, 9), (n[0], 0, 0), (12, 3, 10)]
    return [tuple(a + b for a, b in zip(lo, r)) for r in rel], 16 if size == "small" else 64


def plan_paths(m, size):
    starts, max_len = _starts(size)
    return [(_b(cells), status, cost) for cells, status, cost in m.plan_paths(cost_field(size), BOX[size][0], starts, max_len)]


@deferred
def plan_paths_into(m, size):
    import torch
    starts, max_len = _starts(size)
    cells, paths = _full(m, (len(starts), max_len, 3), torch.int32, 0), _full(m, (16 * len(starts),), torch.uint8)
    cost = _to(m, cost_field(size).view(np.int32))  # cells past a path's length are not written: zeros before
    return [cells, paths], lambda wait: m.plan_paths_into(cells, paths, cost, BOX[size][0], starts, max_len, wait=wait)


def _seen_result(s):
    return [_b(s.seen), _items(s.info), [_items(v) for v in s.view_info]]


def observe(m, size):
    return _seen_result(m.observe(_depth_views(size), lo=BOX[size][0], n=BOX[size][1]))


def observe_accumulate(m, size):
    return _seen_result(m.observe(_depth_views(size), into=_seen(m, size)))


def _observe_into(m, size, accumulate):
    import torch
    d = _to(m, seen_volume(size)) if accumulate else _full(m, BOX[size][1], torch.uint8)
    i, vi, views = _info64(m), _full(m, (32 * NV[size],), torch.uint8), _device_views(m, size, False)
    return [d, i, vi], lambda wait: m.observe_into(d, views, BOX[size][0], accumulate=accumulate, d_info=i, d_view_info=vi, wait=wait)


@deferred
def observe_into(m, size):
    return _observe_into(m, size, False)


@deferred
def observe_into_accumulate(m, size):
    return _observe_into(m, size, True)


def frontiers(m, size):
    return [_b(m.frontiers(_seen(m, size)))]  # host records: ascending order of the cell's place in the box


def frontiers_into(m, size):
    import torch
    n = BOX[size][1]
    cells = _full(m, (n[0] * n[1] * n[2], 4), torch.int32)
    k = m.frontiers_into(cells, _to(m, seen_volume(size)), BOX[size][0])
    rec = cells[:k].cpu().numpy()
    # device records come in unspecified order: compared as a sorted set, as test_gpu_map_seen.py compares them
    return [k, _b(rec[np.lexsort(rec.T[::-1])])]


def view_gain(m, size):
    cam, wh = BOX_CAM[size]
    g = m.view_gain(_seen(m, size), np.stack(POSES[:NV[size]]), camera=cam, size=wh, zrange=ZR, miss_depth=MISS_DEPTH[size])
    return [_b(np.asarray(g)), _items(g.info)]


def view_gain_into(m, size):
    import torch
    cam, wh = BOX_CAM[size]
    k = 1 if size == "small" else GAIN_POSES
    poses = np.stack([POSES[i % len(POSES)].T for i in range(k)]).reshape(k, 16)  # column-major
    out, i = _full(m, (32 * k,), torch.uint8), _info64(m)
    m.view_gain_into(out, _to(m, seen_volume(size)), BOX[size][0], _to(m, poses), camera=cam, size=wh, zrange=ZR, d_info=i,
                     miss_depth=MISS_DEPTH[size])
    return [_b(out), _b(i)]


def _tsdf_result(t):
    out = [_b(t.cells), _items(t.info), [_items(v) for v in t.view_info]]
    return out + ([_b(t.color), _items(t.color_info)] if t.color is not None else [])


def fuse(m, size):
    return _tsdf_result(m.fuse(_depth_views(size), lo=BOX[size][0], n=BOX[size][1]))


def fuse_accumulate(m, size):
    return _tsdf_result(m.fuse(_depth_views(size), into=_tsdf(m, size, False)))


def fuse_color(m, size):
    return _tsdf_result(m.fuse(box_views(size), lo=BOX[size][0], n=BOX[size][1], color=True))


def _fuse_into(m, size, color):
    import torch
    n = BOX[size][1]
    t, i, vi = _full(m, n + (2,), torch.int32), _info64(m), _full(m, (32 * NV[size],), torch.uint8)
    c, ci = (_full(m, n + (4,), torch.int32), _full(m, (32,), torch.uint8)) if color else (None, None)
    views = _device_views(m, size, color)
    return [t, i, vi] + ([c, ci] if color else []), lambda wait: m.fuse_into(t, views, BOX[size][0], d_info=i, d_view_info=vi, wait=wait,
                                                                             d_color=c, d_color_info=ci)


@deferred
def fuse_into(m, size):
    return _fuse_into(m, size, False)


@deferred
def fuse_into_color(m, size):
    return _fuse_into(m, size, True)


def _mesh_result(g):
    # one canonical order on both sides (revo_map_tsdf_mesh): compared as it comes
    return [_b(g.vertices), _b(g.triangles), _items(g.info)] + [_b(a) for a in (g.normals, g.colors) if a is not None]


def mesh(m, size):
    return _mesh_result(m.mesh(_tsdf(m, size, False)))


def mesh_attr(m, size):
    return _mesh_result(m.mesh(_tsdf(m, size, True), normals=True, colors=True))


def mesh_into(m, size, attr=False):
    import torch
    t, c = _d_tsdf(m, size)
    nv, nt, _ = m.mesh_into(None, None, t, BOX[size][0])
    v, tri = _full(m, (max(nv, 1), 3), torch.float32), _full(m, (max(nt, 1), 3), torch.int32)
    nrm, col = (_full(m, (max(nv, 1), 3), torch.float32), _full(m, (max(nv, 1), 4), torch.uint8)) if attr else (None, None)
    got = m.mesh_into(v, tri, t, BOX[size][0], d_normals=nrm, d_colors=col, d_color=c if attr else None)
    m.sync()
    return [got[0], got[1], _items(got[2]), _b(v), _b(tri)] + ([_b(nrm), _b(col)] if attr else [])


def mesh_into_attr(m, size):
    return mesh_into(m, size, attr=True)


def surface_raycast(m, size, color=True):
    cam, wh = BOX_CAM[size]
    r = m.surface_raycast(_tsdf(m, size, color), np.stack(POSES[:NV[size]]), camera=cam, size=wh, zrange=ZR, normals=color, colors=color)
    out = [_b(x) for x in r["depth"]] + [tuple(r["hits"]), _items(r["info"])]
    return out + ([_b(x) for x in r["normals"]] + [_b(x) for x in r["bgr"]] if color else [])


def surface_raycast_plain(m, size):
    return surface_raycast(m, size, color=False)


def surface_raycast_into(m, size, color=True):
    import torch
    cam, (w, h) = BOX_CAM[size]
    n = NV[size]
    t, c = _d_tsdf(m, size)
    d, hits, i = _full(m, (n, h, w), torch.float32, -1.0), _full(m, (n,), torch.int32, -1), _info64(m)
    nrm, bgr = (_full(m, (n, h, w, 3), torch.float32, -2.0), _full(m, (n, h, w, 3), torch.uint8)) if color else (None, None)
    m.surface_raycast_into(d, t, BOX[size][0], np.stack(POSES[:n]), camera=cam, size=(w, h), zrange=ZR, d_normals=nrm, d_bgr=bgr,
                           d_color=c if color else None, d_hits=hits, d_info=i)
    return [_b(x) for x in (d, hits, i) + ((nrm, bgr) if color else ())]


def surface_raycast_into_plain(m, size):
    return surface_raycast_into(m, size, color=False)


def normals(m, size):
    return [_b(a) for a in m.normals(min_count=2 if size == "small" else 1)]


def _source(m):
    """The source map of the registration calls, one per handle under test: every third base record."""
    if getattr(m, "_shared_source", None) is None:
        from revo_amd import api
        m._shared_source = api.VoxelMap(m.cameraPyr, VOXEL, initial_voxels=1)
        m._shared_source.merge_raw(base_records()[::3].copy())
    return m._shared_source


def align_eval(m, size):
    return [_b(r) for r in m.align_eval(_source(m), np.stack(POSES[:NV[size]]))]  # max_dist: the voxel edge


def align_plane_eval(m, size):
    return [_b(r) for r in m.align_plane_eval(_source(m), np.stack(POSES[:NV[size]]))]  # max_dist: the voxel edge


FEATURES = {f.__name__: f for f in (
    render, render_into, raycast, raycast_into, cast_rays, cast_rays_device, carve_eval, pose_raw,
    bounds, distance_field, distance_field_into, known_field, known_field_into, df_sample, sample_into,
    df_align_eval, df_align_eval_device, plan, plan_into, plan_paths, plan_paths_into,
    observe, observe_accumulate, observe_into, observe_into_accumulate, frontiers, frontiers_into,
    view_gain, view_gain_into,
    fuse, fuse_accumulate, fuse_color, fuse_into, fuse_into_color, mesh, mesh_attr, mesh_into, mesh_into_attr,
    surface_raycast, surface_raycast_plain, surface_raycast_into, surface_raycast_into_plain,
    normals, align_eval, align_plane_eval)}

# host-output form -> device-output form, where a call has both
FORMS = {"render": "render_into", "raycast": "raycast_into", "cast_rays": "cast_rays_device", "distance_field": "distance_field_into",
         "known_field": "known_field_into", "df_sample": "sample_into", "df_align_eval": "df_align_eval_device", "plan": "plan_into",
         "plan_paths": "plan_paths_into", "observe": "observe_into", "observe_accumulate": "observe_into_accumulate",
         "frontiers": "frontiers_into", "view_gain": "view_gain_into", "fuse": "fuse_into", "fuse_color": "fuse_into_color",
         "mesh": "mesh_into", "mesh_attr": "mesh_into_attr", "surface_raycast": "surface_raycast_into",
         "surface_raycast_plain": "surface_raycast_into_plain"}

# the device forms test_wait_false_forms_in_stream_order issues with wait=False back to back (each a `deferred` feature)
NO_WAIT = ("render_into", "known_field_into", "observe_into", "fuse_into", "distance_field_into", "sample_into", "plan_paths_into")


# ---------------------------------------------------------------------------------------------------------- mutations --
def merge_grow(m):
    """merge_raw of a set that takes the table past a load of 0.5: a rehash where the table is still the first one."""
    m.merge_raw(grid_records())


def subtract_part(m):
    """subtract_raw of half of what merge_grow brought: the freed voxels go in the live-only compaction."""
    m.subtract_raw(grid_records()[:300])


def carve_view(m):
    """carve with a 2 m image in front of which the grid's remaining voxels lie: they leave, the table is compacted."""
    m.carve([(cc.depth64(), cc.I4, cc.K64)], records=False)


def clear_merge(m):
    m.clear()
    m.merge_raw(base_records())


# in an order in which each is valid after the one before; clear_merge leaves what merge_grow starts from
MUTATIONS = {f.__name__: f for f in (merge_grow, subtract_part, carve_view, clear_merge)}
AFTER_MUTATION = ("raycast", "view_gain", "distance_field", "frontiers", "render")


# ------------------------------------------------------------------------------------------------------------- shares --
_VIEW, _RAY = ("render", "render_into"), ("raycast", "raycast_into", "cast_rays", "cast_rays_device")
_GAIN, _DF = ("view_gain", "view_gain_into"), ("distance_field", "distance_field_into", "known_field", "known_field_into")
_FUSE = ("fuse", "fuse_accumulate", "fuse_color", "fuse_into", "fuse_into_color")
_MESH, _SRAY = ("mesh", "mesh_attr", "mesh_into", "mesh_into_attr"), ("surface_raycast", "surface_raycast_plain", "surface_raycast_into", "surface_raycast_into_plain")
_OBS = ("observe", "observe_accumulate", "observe_into", "observe_into_accumulate")
# member of struct revo_map (or a piece of the map's state) -> the features whose calls go through it
SHARES = {
    "zbuf": _VIEW, "cov": _VIEW, "views": _VIEW, "render_time": _VIEW,
    "bkeys": _RAY + _GAIN, "rcnt": _RAY, "rviews": ("raycast", "raycast_into"), "rout": ("raycast", "cast_rays"), "ray_time": _RAY,
    "dfbits": _DF + ("frontiers", "frontiers_into") + _GAIN, "dfcnt": _DF + ("frontiers", "frontiers_into", "bounds") + _GAIN,
    "dfout": ("distance_field", "known_field"), "df_time": ("distance_field", "distance_field_into"),
    "dfa_poses": ("df_align_eval", "df_align_eval_device"), "dfa_work": ("df_align_eval", "df_align_eval_device"),
    "planwork": ("plan", "plan_into"), "planseeds": ("plan", "plan_into", "plan_paths", "plan_paths_into"),
    "plan_pin": ("plan", "plan_into"), "plan_rounds": ("plan", "plan_into"), "plan_time": ("plan", "plan_into"),
    "seen_views": _OBS, "seencnt": _OBS,
    "seenvol": ("observe", "observe_accumulate", "known_field", "frontiers", "view_gain"),
    "gaindepth": _GAIN, "gaindesc": _GAIN, "gaincnt": _GAIN,
    "tsdf_views": _FUSE, "tsdfcnt": _FUSE, "tsdf_bgr": ("fuse_color", "fuse_into_color"),
    "tsdfvol": ("fuse", "fuse_accumulate", "fuse_color", "mesh", "mesh_attr", "surface_raycast", "surface_raycast_plain"),
    "tsdfcol": ("fuse_color", "mesh_attr", "surface_raycast"),
    "meshwork": _MESH, "meshout": ("mesh", "mesh_attr"),
    "tsdfraywork": _SRAY, "tsdfray_views": _SRAY, "tsdfrayout": ("surface_raycast", "surface_raycast_plain"),
    # the table pointer and mask, across a rehash and a compaction: every feature reads the table the mutations replace
    "table": AFTER_MUTATION,
}
# members of the three owner types that only one feature of the schedule goes through, and why
NOT_SHARED = {
    "vout": "the device outputs of a host-output render: render alone stages through it",
    "plancost": "the device cost field of a host-output plan: plan alone stages through it",
    "gainout": "the device records of a host-output view_gain: view_gain alone stages through it",
}


def handle_members(header_text):
    """The DevBuf, HostRows and EventTimer members of struct revo_map, from the text of revo_map_impl.h."""
    body = re.search(r"struct revo_map \{(.*?)\n\};", header_text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = []
    for kind, decl in re.findall(r"\b(DevBuf|HostRows<[^;]*?>|EventTimer)\s+([^;]*);", body):
        names += [re.sub(r"\s*=.*", "", d).strip() for d in decl.split(",")]
    return names


# ---------------------------------------------------------------------------------------------------------- schedules --
def sharing_pairs():
    """Every ordered pair of different features that go through one member of SHARES."""
    pairs = set()
    for users in SHARES.values():
        pairs |= {(a, b) for a in users for b in users if a != b}
    return sorted(pairs)


def _chain(pairs):
    """A walk that takes every ordered pair once as two consecutive calls, going on from the last call where a pair allows."""
    left, out = set(pairs), []
    while left:
        follow = sorted(p for p in left if out and p[0] == out[-1])
        a, b = follow[0] if follow else min(left)
        if not follow:
            out.append(a)
        out.append(b)
        left.discard((a, b))
    return out


@functools.lru_cache(maxsize=None)
def scripted():
    """The fixed schedule: a tuple of ("call", feature, size) and ("mutate", mutation) steps.  Every feature large, small, large;
    host form then device form and back; every sharing pair in both orders, the sizes alternating along the walk; every mutation
    followed at once by AFTER_MUTATION."""
    steps = []
    for name in FEATURES:
        steps += [("call", name, s) for s in ("large", "small", "large")]
    for host, device in FORMS.items():
        steps += [("call", host, "large"), ("call", device, "small"), ("call", host, "small"), ("call", device, "large")]
    steps += [("call", name, SIZES[i % 2]) for i, name in enumerate(_chain(sharing_pairs()))]
    for name in MUTATIONS:
        steps.append(("mutate", name))
        steps += [("call", f, SIZES[i % 2]) for i, f in enumerate(AFTER_MUTATION)]
    return tuple(steps)


def random_schedule(seed, length):
    """A seeded draw from FEATURES x SIZES with a mutation about every tenth step; the mutations come in MUTATIONS' order, in
    which each is valid after the one before."""
    rng = random.Random(seed)
    names, muts = sorted(FEATURES), list(MUTATIONS)
    steps, k = [], 0
    for _ in range(length):
        if rng.random() < 0.1:
            steps.append(("mutate", muts[k % len(muts)]))
            k += 1
        else:
            steps.append(("call", rng.choice(names), rng.choice(SIZES)))
    return tuple(steps)


RANDOM_SEEDS, RANDOM_LENGTH = (1, 2, 3), 40
