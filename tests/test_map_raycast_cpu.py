"""Rays through the voxel map without a GPU: the exports and the records' layout, revo_amd.mapfile.raycast_records /
cast_rays_records against the per-ray loop of tests/map_raycast_ref.py bit for bit (hand-made cameras, random poses, a sample of
the scene's pixels), one hand-made case per rule of the march, the wall that is only 26-connected, occlusion, the scene's
coverage and wrong-pixel counts against the splat, and the host checks of revo_map_raycast (tests/cpp/ray_host.cpp, built with
the host sanitizers)."""
import ctypes as C
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, mapfile, synth
from revo_amd.settings import MapRay, MapRayHit, MapRayInfo, MapRayParams, MapView

import map_carve_cases as cc
import map_raycast_cases as rc
import map_raycast_ref as rr
import map_render_ref as mr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = mapfile.RAW_DTYPE
I4 = cc.I4
V = rc.V


def _same_view(rec, voxel, T, k, size, pixels=None, got=None, **kw):
    """mapfile.raycast_records against the loop, bit for bit, on all pixels of the view or the given ones; -> the loop's dict."""
    if got is None:
        got = mapfile.raycast_records(rec.astype(RAW), voxel, [(T, k, size)], **kw)
    want = rr.raycast(rec, voxel, mr.View(size[0], size[1], *k, T), pixels=pixels, **kw)
    idx = np.arange(size[0] * size[1]) if pixels is None else np.array([y * size[0] + x for x, y in pixels])
    for name in ("depth", "bgr", "key", "s", "cells", "status"):
        a = got[name][0].reshape((size[0] * size[1],) + got[name][0].shape[2:])[idx]
        assert a.dtype == want[name].dtype and a.tobytes() == want[name].tobytes(), name
    if pixels is None:
        assert got["info"] == want["info"] and got["hits"] == [want["info"]["hits"]]
        assert sum(want["info"][n] for n in rr.STATUS[1:]) + want["info"]["hits"] == want["info"]["rays"] == size[0] * size[1]
    return want


def test_declared_exported_and_laid_out(tmp_path):
    for name in ("revo_map_raycast", "revo_map_cast_rays", "revo_map_raycast_last_ms"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    structs = {"revo_map_ray_params": (MapRayParams, 16), "revo_map_ray": (MapRay, 32), "revo_map_ray_hit": (MapRayHit, 16),
               "revo_map_ray_info": (MapRayInfo, 64)}
    body = ""
    for cname, (cls, _) in structs.items():
        body += '  printf("%s %%zu\\n", sizeof(%s));\n' % (cname, cname)
        for field, _ in cls._fields_:
            body += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (cname, field, cname, field)
    for i, name in enumerate(("HIT", "RANGE", "OUTSIDE", "EXHAUSTED")):
        body += '  printf("REVO_RAY_%s %%u\\n", REVO_RAY_%s);\n' % (name, name)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "revo_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines())
    for cname, (cls, size) in structs.items():
        assert int(got[cname]) == size == C.sizeof(cls), cname
        for field, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, field)]) == getattr(cls, field).offset, (cname, field)
    assert [n for n, _ in MapRayInfo._fields_][:6] == list(rr.INFO_KEYS) == list(mapfile.RAY_INFO_KEYS)
    assert [int(got["REVO_RAY_" + n.upper()]) for n in rr.STATUS] == [0, 1, 2, 3] and mapfile.RAY_STATUS == rr.STATUS
    assert (rr.HIT, rr.RANGE, rr.OUTSIDE, rr.EXHAUSTED) == (rc.HIT, rc.RANGE, rc.OUTSIDE, rc.EXHAUSTED)


@pytest.mark.parametrize("k, size", [(cc.K16, (16, 12)), (cc.K8, (8, 8)), (cc.K64, (64, 64))], ids=["K16", "K8", "K64"])
def test_views_against_the_loop(k, size):
    rec = cc.filled_records()
    want = _same_view(rec, cc.VOXEL, I4, k, size)
    print(k[:4], want["info"])
    assert want["info"]["hits"] > 0 and want["info"]["range"] > 0
    if size == (16, 12):  # transparent to a higher min_count, short of steps, and several views in one call
        for kw in (dict(min_count=3), dict(max_steps=40), dict(max_steps=1)):
            w2 = _same_view(rec, cc.VOXEL, I4, k, size, **kw)
            assert w2["info"]["hits"] < want["info"]["hits"] and (w2["info"]["exhausted"] > 0) == ("max_steps" in kw)
        views = [(I4, k, size), (I4, cc.K8, (8, 8)), (I4, k, (5, 3))]
        both = mapfile.raycast_records(rec.astype(RAW), cc.VOXEL, views)
        singles = [mapfile.raycast_records(rec.astype(RAW), cc.VOXEL, [vw]) for vw in views]
        for name in ("depth", "bgr", "key"):
            assert [a.tobytes() for a in both[name]] == [s[name][0].tobytes() for s in singles]
        assert both["hits"] == [s["hits"][0] for s in singles]
        assert both["info"] == {n: sum(s["info"][n] for s in singles) for n in rr.INFO_KEYS}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_poses_against_the_loop(seed):
    rng = np.random.default_rng(seed)
    rec = cc.filled_records()
    T = synth.se3_exp(np.concatenate([rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.15, 0.15, 3)])).astype(F)
    k, size = ((cc.K16, (16, 12)), (cc.K8, (8, 8)), ((9.0, 7.0, 6.5, 4.25, 0.25, 3.0), (13, 9)))[seed]
    want = _same_view(rec, cc.VOXEL, T, k, size, min_count=1 + seed // 2)
    print(seed, want["info"])
    assert want["info"]["hits"] > 0
    # the same rays through cast_rays_records: its voxels have no depth range, so only the rays are compared with the loop
    o, s0, d, s1 = mapfile.ray_view_rays(mapfile.ray_view(T, k, size))
    rays = np.concatenate([o, s0[:, None], d, s1[:, None]], 1)
    for kw in (dict(), dict(min_count=2, max_steps=50)):
        got, want = mapfile.cast_rays_records(rec.astype(RAW), cc.VOXEL, rays, **kw), rr.cast_rays(rec, cc.VOXEL, rays, **kw)
        assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got[:4], want[:4])) and got[4] == want[4]


def _check_ray_case(case, got):
    name, rows, ray, min_count, max_steps, (status, hit, s, cells) = case
    key, gs, gcells, gstatus = int(got[0]), got[1], int(got[2]), int(got[3])
    assert gstatus == status, name
    assert key == (rc.key_of(*hit) if hit is not None else rc.EMPTY), name
    assert s is None or gs == F(s), (name, gs)
    assert cells is None or gcells == cells, (name, gcells)
    assert (gcells == 0) == (status == rc.OUTSIDE and cells == 0), name


def test_one_case_per_rule():
    seen = set()
    for case in rc.ray_cases():
        name, rows, ray, min_count, max_steps, want = case
        rec = rc.records(rows)
        rays = np.asarray([ray], F)
        loop = rr.cast_rays(rec, V, rays, min_count, max_steps)
        vec = mapfile.cast_rays_records(rec.astype(RAW), V, rays, min_count, max_steps)
        assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(vec[:4], loop[:4])) and vec[4] == loop[4], name
        _check_ray_case(case, [x[0] for x in loop[:4]])
        assert loop[4]["rays"] == 1 and loop[4][rr.STATUS[want[0]] + ("s" if want[0] == rc.HIT else "")] == 1 and loop[4]["cells"] == int(loop[2][0])
        seen.add(want[0])
    assert seen == {rc.HIT, rc.RANGE, rc.OUTSIDE, rc.EXHAUSTED}
    # all the cases of one map in one call, and in another order
    rays = np.asarray([c[2] for c in rc.ray_cases() if c[1] is rc.ALONG_X and c[3] == 1 and c[4] == 4096], F)
    rec = rc.records(rc.ALONG_X)
    a = mapfile.cast_rays_records(rec.astype(RAW), V, rays)
    b = mapfile.cast_rays_records(rec.astype(RAW), V, rays[::-1])
    loop = rr.cast_rays(rec, V, rays)
    assert all(x.tobytes() == y[::-1].tobytes() == z.tobytes() for x, y, z in zip(a[:4], b[:4], loop[:4])) and a[4] == b[4] == loop[4]


def test_a_view_sees_only_its_depth_range():
    for name, rows, min_count, z in rc.view_cases():
        rec = rc.records(rows)
        want = _same_view(rec, V, I4, rc.VIEW_K, rc.VIEW_SIZE, min_count=min_count)
        p = 4 * 8 + 4
        if z is None:
            assert want["status"][p] == rc.RANGE and want["depth"][p] == 0 and want["key"][p] == rc.EMPTY and not want["bgr"][p].any(), name
        else:
            assert want["status"][p] == rc.HIT and want["depth"][p] == F(z) > 0 and tuple(want["bgr"][p]) == (10, 20, 30), name
        assert want["cells"][p] == (12 if z is None else int(np.floor(z / V)) - 3), name  # the cells (0, 0, 4) .. (0, 0, 15)
        assert not np.any((want["depth"] != 0) & ((want["depth"] <= F(rc.VIEW_K[4])) | (want["depth"] >= F(rc.VIEW_K[5]))))


def test_no_leak_through_a_diagonal_wall():
    rec = rc.wall_records()
    got = mapfile.raycast_records(rec.astype(RAW), V, [(I4, rc.WALL_K, rc.WALL_SIZE)])
    px = rc.wall_reaching_pixels()
    assert len(px) == 34 * 64
    _same_view(rec, V, I4, rc.WALL_K, rc.WALL_SIZE, pixels=px[::7], got=got)
    status, key = got["status"][0], got["key"][0]
    for x, y in px:
        assert status[y, x] == rc.HIT, (x, y)
    b = np.int64(1 << 20)
    hit = key[status == rc.HIT]
    kx, kz = (hit >> np.uint64(42)).astype(np.int64) - b, (hit & np.uint64(0x1fffff)).astype(np.int64) - b
    assert np.all(kx + kz == rc.WALL_C) and np.all(np.isin(hit, rec["key"]))
    print("wall: %d of %d rays hit, %d had to" % (got["hits"][0], 64 * 64, len(px)))


def test_occlusion_and_subtract():
    rec = rc.records([rc.cell(1, 0, 0, 2), rc.cell(3, 0, 0, 1), rc.cell(0, 5, 0, 1)]).astype(RAW)
    rays = np.asarray([rc.ray(rc.C0, 0.0, (1, 0, 0), 1.0)], F)
    key, s, cells, status, _ = mapfile.cast_rays_records(rec, V, rays)
    assert (int(key[0]), s[0], int(cells[0]), int(status[0])) == (rc.key_of(1, 0, 0), F(0.5 * V), 2, rc.HIT)
    near = rec[rec["key"] == np.uint64(rc.key_of(1, 0, 0))]
    rest = mapfile.subtract_records(rec, near)
    key, s, cells, status, _ = mapfile.cast_rays_records(rest, V, rays)
    assert (int(key[0]), s[0], int(cells[0]), int(status[0])) == (rc.key_of(3, 0, 0), F(2.5 * V), 4, rc.HIT)
    half = near.copy()  # one of its two points leaves: the voxel stays, and stays in the way
    half["count"], half["sum_q"], half["sum_bgr"] = 1, near["sum_q"] // 2, near["sum_bgr"] // 2
    assert int(mapfile.cast_rays_records(mapfile.subtract_records(rec, half), V, rays)[0][0]) == rc.key_of(1, 0, 0)


@functools.lru_cache(maxsize=None)
def _scene_cast():
    """The scene map from its own two keyframe poses: computed once for the two scene tests."""
    s = cc.settings320()
    rec = cc.scene_records().astype(RAW)
    views = [(cc.poses()[i].astype(F), cc.intrinsics320(), (s.width, s.height)) for i in (0, 1)]
    return rec, views, mapfile.raycast_records(rec, cc.VOXEL, views)


def test_scene_pixels_against_the_loop():
    rec, views, got = _scene_cast()
    s = cc.settings320()
    px = [(x, y) for y in range(0, s.height, 5) for x in range(0, s.width, 7)]
    for i, (T, k, size) in enumerate(views):
        one = {n: [got[n][i]] for n in ("depth", "bgr", "key", "s", "cells", "status")}
        want = _same_view(rec, cc.VOXEL, T, k, size, pixels=px, got=one)
        print("view %d: %d sampled pixels, %s" % (i, len(px), want["info"]))
        assert want["info"]["hits"] > 0.9 * len(px)


def test_the_scene_is_covered_and_nearer_the_truth_than_the_splat():
    """DESIGN 20's table.  From the poses of the map's own two keyframes every pixel whose true depth is usable is a hit, and
    fewer pixels are more than 5 cm from the true depth than in the splat at splat_max = 4."""
    rec, views, got = _scene_cast()
    s = cc.settings320()
    xyz, rgb, _ = mapfile.to_points(rec)
    for i, (T, k, size) in enumerate(views):
        truth = cc.scene_frames()[0][i][1]
        usable = np.isfinite(truth) & (truth > s.depth_min) & (truth < s.depth_max)
        d = got["depth"][i]
        sd, sb, cov = mr.render(xyz, rgb, cc.VOXEL, mr.view_of(s, T, 4))
        wrong = int((np.abs(d - truth)[(d > 0) & usable] > 0.05).sum())
        wrong_splat = int((np.abs(sd - truth)[(sd > 0) & usable] > 0.05).sum())
        err = np.abs(d - truth)[(d > 0) & usable]
        print("view %d: %d of %d pixels hit, %d of %d usable ones; > 5 cm from the truth: %d (splat_max 4: %d of %d covered); median error %.3g m; "
              "%d cells, %.0f per ray" % (i, got["hits"][i], d.size, int(((d > 0) & usable).sum()), int(usable.sum()), wrong, wrong_splat, cov,
                                         float(np.median(err)), int(got["cells"][i].sum()), got["cells"][i].mean()))
        assert np.all(d[usable] > 0)
        assert wrong < wrong_splat
        assert got["hits"][i] == int((d > 0).sum()) == int((got["key"][i] != mapfile.RAY_EMPTY).sum())
        # a hit shows a voxel of the map, its colour and the depth of its mean
        assert np.all(np.isin(got["key"][i][d > 0], rec["key"]))
    assert got["info"]["rays"] == 2 * s.width * s.height and got["info"]["hits"] == sum(got["hits"]) and got["info"]["exhausted"] == 0


def test_refusals():
    rec = cc.class_records()[0].astype(RAW)
    nan = I4.copy()
    nan[1, 3] = np.nan
    view = (I4, cc.K16, (16, 12))
    for bad in ([], [view] * 65, [(nan, cc.K16, (16, 12))], [(I4, cc.K16, (0, 12))], [(I4, cc.K16, (16, 2049))],
                [(I4, (0.0,) + cc.K16[1:], (16, 12))], [(I4, cc.K16[:4] + (1.0, 1.0), (16, 12))], [(I4, cc.K16[:4] + (-1.0, 1.0), (16, 12))],
                [(I4, cc.K16[:4] + (0.1, np.inf), (16, 12))]):
        with pytest.raises(ValueError):
            mapfile.raycast_records(rec, cc.VOXEL, bad)
    for kw in (dict(max_steps=0), dict(max_steps=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            mapfile.raycast_records(rec, cc.VOXEL, [view], **kw)
        with pytest.raises(ValueError):
            mapfile.cast_rays_records(rec, cc.VOXEL, np.zeros((1, 8), F), **kw)
    with pytest.raises(ValueError):
        mapfile.cast_rays_records(rec, cc.VOXEL, np.zeros((0, 8), F))
    with pytest.raises(ValueError):
        mapfile.cast_rays_records(rec[::-1], cc.VOXEL, np.zeros((1, 8), F))
    # a skewed pose is revo_map_render's to take, and so the march's
    skew = I4.copy()
    skew[0, 1] = 0.01
    assert mapfile.raycast_records(rec, cc.VOXEL, [(skew, cc.K16, (16, 12))], max_steps=1 << 20)["info"]["rays"] == 192
    # an empty map: every ray runs out of range
    empty = mapfile.raycast_records(rec[:0], cc.VOXEL, [view])
    assert empty["hits"] == [0] and not empty["depth"][0].any() and np.all(empty["key"][0] == mapfile.RAY_EMPTY) and empty["info"]["range"] == 192


def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "ray_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "ray_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def _view_bytes(w, h, k, T, splat_max=0, min_count=1):
    v = MapView()
    v.width, v.height = w, h
    v.fx, v.fy, v.cx, v.cy, v.zmin, v.zmax = [float(x) for x in k]
    v.T_w_c[:] = np.ascontiguousarray(np.asarray(T, F).T).reshape(16).tolist()
    v.splat_max, v.min_count = splat_max, min_count
    return bytes(v)


def test_host_checks(tmp_path):
    """revo_ray_host.h over views, groups of views and parameter sets: the views the restatement accepts, o, R, Rc and tc as it
    forms them, the common min_count, and the effective max_steps."""
    exe = _host(tmp_path)
    ctx = list(cc.K16)
    T = synth.se3_exp(np.array([0.3, -0.2, 0.1, 0.4, -0.3, 0.2])).astype(F)
    skew, nan = I4.copy(), I4.copy()
    skew[0, 1] = 0.01
    nan[1, 3] = np.nan
    zero, own = [0.0] * 6, [500.0, 510.0, 320.0, 240.0, 0.5, 8.0]
    # (w, h, intrinsics, pose, splat_max, min_count) -> the intrinsics it is taken with, or None
    views = [((640, 480, own, T, 0, 1), own), ((8, 8, zero, T, 0, 0), ctx), ((16, 12, zero, I4, 99, 1), ctx), ((1, 2048, zero, skew, -5, 3), ctx),
             ((2048, 1, own, np.diag(F([1, 1, -1, 1])), 0, 3), own), ((0, 8, zero, T, 0, 1), None), ((8, 2049, zero, T, 0, 1), None),
             ((8, 8, [0.0] + own[1:], T, 0, 1), None), ((8, 8, own[:1] + [-2.0] + own[2:], T, 0, 1), None),
             ((8, 8, own[:2] + [np.nan] + own[3:], T, 0, 1), None), ((8, 8, own[:4] + [-0.5, 8.0], T, 0, 1), None),
             ((8, 8, own[:4] + [8.0, 8.0], T, 0, 1), None), ((8, 8, own[:4] + [0.0, 8.0], T, 0, 1), own[:4] + [0.0, 8.0]),
             ((8, 8, zero, nan, 0, 1), None)]
    groups = [((0, 1), 1), ((0, 2), 1), ((0, 3), 1), ((0, 4), 0), ((3, 2), 3), ((1, 1), 1), ((3, 1), 3)]
    params = [(0, (9, 9, 9, 9)), (1, (4096, 0, 0, 0)), (1, (1, 0, 0, 0)), (1, (1 << 20, 0, 0, 0)), (1, (0, 0, 0, 0)), (1, ((1 << 20) + 1, 0, 0, 0)),
              (1, (16, 1, 0, 0)), (1, (16, 0, 1, 0)), (1, (16, 0, 0, 1))]
    want_params = [4096, 4096, 1, 1 << 20] + [None] * 5
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.asarray(ctx, F).tobytes() + struct.pack("<I", len(views)))
        for (w, h, k, P, sp, mc), _ in views:
            f.write(_view_bytes(w, h, k, P, sp, mc))
        f.write(struct.pack("<I", len(groups)))
        for (first, count), _ in groups:
            f.write(struct.pack("<2I", first, count))
        f.write(struct.pack("<I", len(params)))
        for has, p in params:
            f.write(struct.pack("<i4I", has, *p))
    subprocess.run([exe, inp, out], check=True, timeout=120)
    raw = open(out, "rb").read()
    o = 0
    for (w, h, k, P, sp, mc), want in views:
        ok = raw[o]
        o += 1
        assert bool(ok) == (want is not None), (w, h, k)
        if not ok:
            with pytest.raises(ValueError):
                mapfile.ray_view(P, k if any(k) else ctx, (w, h))
            continue
        gw, gh = struct.unpack_from("<2i", raw, o)
        f30 = np.frombuffer(raw, F, 30, o + 8)
        o += 8 + 120
        vo, vR, vRc, vtc, vk, vsize = mapfile.ray_view(P, want, (w, h))
        Rc, tc = mr.world_to_camera(np.asarray(P, F))
        assert (gw, gh) == (w, h) == vsize
        assert f30[:3].tobytes() == vo.tobytes() == np.asarray(P, F)[:3, 3].tobytes()
        assert f30[3:12].tobytes() == vR.tobytes() == np.ascontiguousarray(np.asarray(P, F)[:3, :3]).tobytes()
        assert f30[12:21].tobytes() == vRc.tobytes() == Rc.tobytes() and f30[21:24].tobytes() == vtc.tobytes() == tc.tobytes()
        assert f30[24:].tobytes() == vk.tobytes() == np.asarray(want, F).tobytes()
    for _, want in groups:
        assert struct.unpack_from("<I", raw, o)[0] == want
        o += 4
    for (has, p), want in zip(params, want_params):
        ok = raw[o]
        o += 1
        assert bool(ok) == (want is not None), p
        if ok:
            assert struct.unpack_from("<I", raw, o)[0] == want
            o += 4
    assert o == len(raw)
