"""Free-space carving without a GPU: the exports and the records' layout, revo_amd.mapfile.carve_records against the
per-voxel loop of tests/map_carve_ref.py bit for bit on hand-made voxels (one case per rule) and random ones, the three exact
properties (idempotence, view order, carving in parts), carve followed by merge, the synthetic scene with a moved box,
`python -m revo_amd.mapfile carve`, and the host checks of revo_map_carve (tests/cpp/carve_host.cpp, built with the host
sanitizers)."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, mapfile
from revo_amd.settings import MapCarveInfo, MapCarveParams, MapCarveView, MapCarveViewInfo

import map_carve_cases as cc
import map_carve_ref as mc
import map_render_ref as mr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = mapfile.RAW_DTYPE
I4 = cc.I4
VIEW16 = (cc.depth16(), I4, cc.K16)


def _same(rec, views, **kw):
    """mapfile.carve_records against the reference loop, bit for bit; -> (removed, info, counts, classes)."""
    want, winfo, wcounts, cls = mc.carve_eval(rec, cc.VOXEL, views, **kw)
    got, ginfo, gcounts = mapfile.carve_records(rec.astype(RAW), cc.VOXEL, views, **kw)
    assert got.dtype == RAW and got.tobytes() == want.tobytes() and ginfo == winfo and gcounts == wcounts
    assert all(sum(c.values()) == winfo["voxels_considered"] for c in wcounts)
    return got, ginfo, gcounts, cls


def test_declared_exported_and_laid_out(tmp_path):
    for name in ("revo_map_carve_eval", "revo_map_carve"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    structs = {"revo_map_carve_info": (MapCarveInfo, 64), "revo_map_carve_view_info": (MapCarveViewInfo, 32),
               "revo_map_carve_view": (MapCarveView, 112), "revo_map_carve_params": (MapCarveParams, 24)}
    body = ""
    for cname, (cls, _) in structs.items():
        body += '  printf("%s %%zu\\n", sizeof(%s));\n' % (cname, cname)
        for field, _ in cls._fields_:
            body += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (cname, field, cname, field)
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
    assert [n for n, _ in MapCarveInfo._fields_][:4] == list(mc.INFO_KEYS) == list(mapfile.CARVE_INFO_KEYS)
    assert [n.replace("free_space", "free") for n, _ in MapCarveViewInfo._fields_][:6] == list(mc.CLASSES) == list(mapfile.CARVE_CLASSES)
    assert [getattr(MapCarveViewInfo, n).offset for n, _ in MapCarveViewInfo._fields_][:6] == [4 * i for i in range(6)]


def test_one_voxel_per_rule():
    rec, where, expect = cc.class_records()
    got, info, counts, cls = _same(rec, [VIEW16], margin=cc.M)
    named = {n: mc.CLASSES[cls[i, 0]] for n, i in where.items()}
    assert named == expect
    assert set(expect.values()) == set(mc.CLASSES)  # every class occurs
    free = sorted(rec["key"][[i for n, i in where.items() if expect[n] == "free"]].tolist())
    assert got["key"].tolist() == free and info["voxels_carved"] == len(free) == info["votes"] == counts[0]["free"]
    assert info["points_carved"] == int(rec["count"][np.isin(rec["key"], free)].sum()) > len(free)  # the count-8 voxel is one of them
    # the two boundaries: equal is not beyond, one float32 step is
    z = mapfile.to_points(rec)[0][:, 2]
    assert z[where["free_boundary"]] == F(2.0 - cc.M) and z[where["free_one_below"]] == np.nextafter(F(2.0 - cc.M), F(0))
    assert z[where["confirmed_boundary"]] == F(2.0 + cc.M) and z[where["occluded_one_above"]] == np.nextafter(F(2.0 + cc.M), F(9))
    # u + 0.5 exactly on an integer: pixel 6, whose own depth says free once the window no longer holds pixel 5
    i = where["half_pixel"]
    v = mc.View(*VIEW16)
    p = mapfile.to_points(rec)[0][i]
    assert (v.fx * p[0]) / p[2] + v.cx == F(5.5)
    assert mc.CLASSES[mc.classify(p, v, 0, F(cc.M), F(0))] == "free" and mc.CLASSES[mc.classify(p, v, 1, F(cc.M), F(0))] == "edge"
    moved = cc.depth16()
    moved[6, 5], moved[6, 6] = 2.0, 0.5  # the depths of pixels 5 and 6 swapped: were pixel 5 the nearest, this would be free
    assert mc.CLASSES[mc.classify(p, mc.View(moved, I4, cc.K16), 0, F(cc.M), F(0))] == "occluded"


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_every_radius_and_margin(radius):
    rec, where, expect = cc.class_records()
    per_margin = []
    for kw in (dict(margin=cc.M), dict(margin=0.0), dict(margin=cc.M, margin_rel=2.0 ** -5), dict(margin=None)):
        got, info, counts, cls = _same(rec, [VIEW16], radius=radius, **kw)
        per_margin.append(info["voxels_carved"])
        # a border voxel is outside exactly when its window leaves the image
        assert (mc.CLASSES[cls[where["border_left_in"], 0]] == "outside") == (radius > 1)
        assert (mc.CLASSES[cls[where["border_left"], 0]] == "outside") == (radius > 0)
        assert mc.CLASSES[cls[where["off_image"], 0]] == "outside"
    assert (per_margin[0] > 0) == (radius < 3)  # at radius 3 every window of the class cases holds a hole or leaves the image
    filled = cc.filled_records()
    g, info, counts, _ = _same(filled, [VIEW16], radius=radius, margin=cc.M)
    assert min(counts[0][k] for k in ("outside", "free", "occluded")) > 5 and counts[0]["confirmed"] > 0
    if radius:
        assert counts[0]["unknown"] > 0 and counts[0]["edge"] > 0
    for seed, (h, w, k) in enumerate(((8, 8, cc.K8), (12, 16, cc.K16))):
        rr, view = cc.random_case(seed, h, w, k)
        _, ri, rc, _ = _same(rr, [view], radius=radius, margin=0.05, margin_rel=0.01)
        if radius < 3:
            assert ri["voxels_carved"] > 0 and rc[0]["unknown"] > 0


def test_min_views_min_count_max_count_and_the_empty_map():
    rec, where, expect = cc.class_records()
    views = cc.three_views()
    carved = []
    for mv in (0, 1, 2, 3, 4):
        got, info, counts, cls = _same(rec, views, margin=cc.M, min_views=mv)
        votes = (cls == mc.FREE).sum(1)
        assert info["votes"] == int(votes.sum()) and got["key"].tolist() == rec["key"][votes >= max(mv, 1)].tolist()
        carved.append(len(got))
    assert (votes[where["free"]], votes[where["border_right_in"]], votes[where["border_left_in"]]) == (1, 2, 3)
    assert carved[0] == carved[1] > carved[2] > carved[3] > carved[4] == 0
    # counts: the one-float cases have counts 8 and 4, every other voxel 1
    assert _same(rec, [VIEW16], margin=cc.M, min_count=2)[1]["voxels_considered"] == 2
    assert _same(rec, [VIEW16], margin=cc.M, min_count=5)[0]["key"].tolist() == [int(rec["key"][where["free_one_below"]])]
    g, info, _, _ = _same(rec, [VIEW16], margin=cc.M, max_count=1)
    assert info["voxels_considered"] == len(rec) - 2 and int(rec["key"][where["free_one_below"]]) not in g["key"].tolist()
    assert _same(rec, [VIEW16], margin=cc.M, min_count=4, max_count=4)[1] == dict(voxels_considered=1, voxels_carved=0, points_carved=0, votes=0)
    g, info, counts, _ = _same(np.zeros(0, mc.mrr.DTYPE), views, margin=cc.M)
    assert len(g) == 0 and info == dict.fromkeys(mc.INFO_KEYS, 0) and counts == [dict.fromkeys(mc.CLASSES, 0)] * 3


def test_the_three_exact_properties_and_the_way_back():
    rec = cc.filled_records().astype(RAW)
    views = cc.three_views()
    other = cc.random_case(5, 12, 16, cc.K16)[1]
    A, B = views[:2], [views[2], other]
    kw = dict(margin=cc.M)
    gone, info, _ = mapfile.carve_records(rec, cc.VOXEL, A + B, **kw)
    left = mapfile.subtract_records(rec, gone)
    assert 0 < len(gone) < len(rec) and left.tobytes() == mc.remaining(rec, gone).tobytes()
    # a second identical carve removes nothing
    again, info2, _ = mapfile.carve_records(left, cc.VOXEL, A + B, **kw)
    assert len(again) == 0 and info2["votes"] == 0 and info2["voxels_considered"] == len(left)
    # the order of the views cannot show
    for mv in (1, 2, 3):
        a = mapfile.carve_records(rec, cc.VOXEL, A + B, min_views=mv, **kw)
        b = mapfile.carve_records(rec, cc.VOXEL, (A + B)[::-1], min_views=mv, **kw)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2] == b[2][::-1]
    # min_views = 1: views A, then views B on what is left, is one carve with both
    ga = mapfile.carve_records(rec, cc.VOXEL, A, **kw)[0]
    la = mapfile.subtract_records(rec, ga)
    gb = mapfile.carve_records(la, cc.VOXEL, B, **kw)[0]
    assert len(ga) and len(gb) and mapfile.subtract_records(la, gb).tobytes() == left.tobytes()
    assert mapfile.merge_records(ga, gb).tobytes() == gone.tobytes()
    # carve, then merge the removed records: the map is back
    assert mapfile.merge_records(left, gone).tobytes() == rec.tobytes()
    assert mc.counters_after(dict(voxels=len(rec), points_integrated=int(rec["count"].sum()), points_dropped=3, keyframes=2), info) == \
        dict(voxels=len(left), points_integrated=int(left["count"].sum()), points_dropped=3, keyframes=2)


def test_refusals():
    rec = cc.class_records()[0].astype(RAW)
    skew, nan = I4.copy(), I4.copy()
    skew[0, 1] = 0.01
    nan[1, 3] = np.nan
    D = cc.depth16()
    k = list(cc.K16)
    bad_views = [(D, skew, cc.K16), (D, nan, cc.K16), (D, np.diag(F([1, 1, -1, 1])), cc.K16), (np.zeros((0, 4), F), I4, cc.K16),
                 (np.zeros((4, 2049), F), I4, cc.K16), (D, I4, [0.0] + k[1:]), (D, I4, k[:1] + [-1.0] + k[2:]), (D, I4, k[:2] + [np.inf] + k[3:]),
                 (D, I4, k[:4] + [-0.1, 5.0]), (D, I4, k[:4] + [2.0, 2.0]), (D, I4, k[:4] + [np.nan, 2.0])]
    for v in bad_views:
        with pytest.raises(ValueError):
            mapfile.carve_records(rec, cc.VOXEL, [v])
        with pytest.raises(ValueError):
            mc.carve_eval(rec, cc.VOXEL, [v])
    for kw in (dict(radius=-1), dict(radius=4), dict(margin=-0.01), dict(margin=np.nan), dict(margin_rel=-1.0), dict(margin_rel=np.inf)):
        with pytest.raises(ValueError):
            mapfile.carve_records(rec, cc.VOXEL, [VIEW16], **kw)
        with pytest.raises(ValueError):
            mc.carve_eval(rec, cc.VOXEL, [VIEW16], **kw)
    for views in ([], [VIEW16] * 65):
        with pytest.raises(ValueError):
            mapfile.carve_records(rec, cc.VOXEL, views)
        with pytest.raises(ValueError):
            mc.carve_eval(rec, cc.VOXEL, views)
    assert mapfile.carve_records(rec, cc.VOXEL, [VIEW16] * 64)[1]["voxels_considered"] == len(rec)


def test_the_scene_with_a_moved_box():
    """DESIGN 19's figures.  The map of views 0 and 1 of scene 902 holds box 3; four views of the scene as it was carve nothing,
    four views of the scene with the box gone carve the box and nothing else."""
    rec = cc.scene_records().astype(RAW)
    ghost = cc.ghost_mask(rec)
    print("map: %d voxels, %d of them the ghost" % (len(rec), int(ghost.sum())))
    assert len(rec) > 30000 and ghost.sum() > 1000
    kw = dict(radius=1, margin=0.02, margin_rel=0.0)
    same, info, counts = mapfile.carve_records(rec, cc.VOXEL, cc.scene_views(False), **kw)
    print("unchanged scene:", info, counts)
    assert len(same) == 0  # the consistent scene loses nothing
    for mv in (1, 2):
        gone, info, counts = mapfile.carve_records(rec, cc.VOXEL, cc.scene_views(True), min_views=mv, **kw)
        is_ghost = np.isin(gone["key"], rec["key"][ghost])
        print("changed scene, min_views %d: %d of %d ghost voxels carved, %d others; %s" % (mv, int(is_ghost.sum()), int(ghost.sum()),
                                                                                         int((~is_ghost).sum()), counts))
        assert int((~is_ghost).sum()) == 0  # no voxel outside the ghost is carved
        if mv == 1:
            assert is_ghost.sum() >= 0.9 * ghost.sum()
            # the loop of the specification agrees bit for bit on the candidates that matter: the ghost and a slice of the rest
            part = np.concatenate([rec[ghost], rec[~ghost][::40]])
            part = part[np.argsort(part["key"])]
            _same(part, cc.scene_views(True), **kw)
    no_window = mapfile.carve_records(rec, cc.VOXEL, cc.scene_views(False), radius=0, margin=0.02)[0]
    print("unchanged scene, radius 0: %d voxels carved" % len(no_window))
    assert len(no_window) > 100  # why the window exists


def test_command_line_round_trip(tmp_path, capsys):
    from PIL import Image
    from revo_amd import vo
    rec = cc.filled_records().astype(RAW)
    a, out, removed, back, folder = (str(tmp_path / n) for n in ("a.rvm", "out.rvm", "removed.rvm", "back.rvm", "views"))
    mapfile.write(a, mapfile.make_header(cc.VOXEL, 1, rec, 7, 2), rec)
    # a --map-views folder written by hand: 16-bit depth at 5000 per metre, associate.txt, poses.txt
    os.makedirs(os.path.join(folder, "depth"))
    os.makedirs(os.path.join(folder, "rgb"))
    D = cc.depth16()
    D[~np.isfinite(D)] = 0.0
    views = []
    T2 = np.eye(4, dtype=F)
    T2[0, 3] = 0.25
    stamps = [(1.5, I4), (2.5, T2)]
    with open(os.path.join(folder, "poses.txt"), "w") as f:
        f.write("".join(line + "\n" for line in vo.tum_lines(stamps)))
    with open(os.path.join(folder, "associate.txt"), "w") as f:
        for ts, T in stamps:
            name = "%.6f.png" % ts
            raw = np.rint(D * 5000.0).astype(np.uint16)
            Image.fromarray(raw).save(os.path.join(folder, "depth", name))
            Image.fromarray(np.zeros((12, 16, 3), np.uint8)).save(os.path.join(folder, "rgb", name))
            f.write("%.6f rgb/%s %.6f depth/%s\n" % (ts, name, ts, name))
            views.append((raw.astype(F) / F(5000.0), T, cc.K16))
    args = ["--camera", "4", "4", "8", "6", "--zrange", "%.9g" % cc.ZMIN, "%.9g" % cc.ZMAX, "--margin", str(cc.M)]
    assert mapfile.main(["carve", a, "--views", folder, "-o", out, "--removed", removed] + args) == 0
    want_left, want_gone, winfo, _ = mc.carve(rec, cc.VOXEL, views, margin=cc.M)
    h, left = mapfile.read(out)
    hg, gone = mapfile.read(removed)
    assert left.tobytes() == want_left.astype(RAW).tobytes() and gone.tobytes() == want_gone.astype(RAW).tobytes() and len(gone) > 0
    assert (h["voxel"], h["dense"], h["points_dropped"], h["keyframes"]) == (mapfile.read(a)[0]["voxel"], 1, 7, 2)
    assert (hg["points_dropped"], hg["keyframes"]) == (0, 0)
    assert mapfile.main(["merge", back, out, removed]) == 0
    assert open(back, "rb").read() == open(a, "rb").read()
    # parameters reach the rule
    assert mapfile.main(["carve", a, "--views", folder, "-o", out, "--min-views", "2", "--radius", "0"] + args) == 0
    assert mapfile.read(out)[1].tobytes() == mc.carve(rec, cc.VOXEL, views, margin=cc.M, min_views=2, radius=0)[0].astype(RAW).tobytes()
    assert mapfile.main(["carve", a, "--views", folder, "-o", out, "--radius", "4"] + args) == 1
    assert mapfile.main(["carve", a, "--views", str(tmp_path / "nothing"), "-o", out]) == 1
    assert mapfile.main(["carve", a, "-o", out]) == 2
    capsys.readouterr()


def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "carve_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "carve_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def test_host_checks(tmp_path):
    """revo_carve_host.h over views, parameter sets and unsorted records: the views the reference accepts, Rc and tc as
    map_render_ref forms them, the effective parameters, and the records in ascending key order."""
    from revo_amd import synth
    exe = _host(tmp_path)
    ctx = list(cc.K16)
    T = synth.se3_exp(np.array([0.3, -0.2, 0.1, 0.4, -0.3, 0.2])).astype(F)
    skew, nan = I4.copy(), I4.copy()
    skew[0, 1] = 0.01
    nan[1, 3] = np.nan
    zero, own = [0.0] * 6, [500.0, 510.0, 320.0, 240.0, 0.5, 8.0]
    # (has_kf, has_depth, w, h, intrinsics, pose) -> accepted, and with what
    views = [((0, 1, 640, 480, own, T), (640, 480, own)), ((0, 1, 8, 8, zero, T), (8, 8, ctx)), ((1, 0, 0, 0, zero, I4), (16, 12, ctx)),
             ((1, 0, 5, 5, own, T), (16, 12, ctx)), ((1, 1, 8, 8, zero, T), None), ((0, 0, 8, 8, zero, T), None),
             ((0, 1, 0, 8, zero, T), None), ((0, 1, 8, 2049, zero, T), None), ((0, 1, 2048, 1, zero, T), (2048, 1, ctx)),
             ((0, 1, 8, 8, [0.0] + own[1:], T), None), ((0, 1, 8, 8, own[:1] + [-2.0] + own[2:], T), None),
             ((0, 1, 8, 8, own[:2] + [np.nan] + own[3:], T), None), ((0, 1, 8, 8, own[:4] + [-0.5, 8.0], T), None),
             ((0, 1, 8, 8, own[:4] + [8.0, 8.0], T), None), ((0, 1, 8, 8, own[:4] + [0.0, 8.0], T), (8, 8, own[:4] + [0.0, 8.0])),
             ((0, 1, 8, 8, zero, skew), None), ((0, 1, 8, 8, zero, nan), None), ((0, 1, 8, 8, zero, np.diag(F([1, 1, -1, 1]))), None)]
    params = [(0, (9, 9, 9, 9, 9.0, 9.0)), (1, (0, 0, 0, 0, 0.0, 0.0)), (1, (3, 2, 3, 4, 0.5, 0.25)), (1, (4, 1, 1, 0, 0.1, 0.0)),
              (1, (-1, 1, 1, 0, 0.1, 0.0)), (1, (1, 1, 1, 0, -0.1, 0.0)), (1, (1, 1, 1, 0, np.nan, 0.0)), (1, (1, 1, 1, 0, 0.1, -1.0)),
              (1, (1, 1, 1, 0, 0.1, np.inf))]
    want_params = [(1, 1, 1, 0, F(0.02), F(0)), (0, 1, 1, 0, F(0), F(0)), (3, 2, 3, 4, F(0.5), F(0.25))] + [None] * 6
    rng = np.random.default_rng(4)
    rec = np.zeros(300, RAW)
    rec["key"] = rng.permutation(1 << 20)[:300].astype(np.uint64) << np.uint64(13)
    rec["count"] = rng.integers(1, 1 << 20, 300)
    rec["sum_q"] = rng.integers(-(1 << 61), 1 << 61, (300, 3))
    rec["sum_bgr"] = rng.integers(0, 1 << 40, (300, 3))
    for r in (rec, rec[:1], rec[:0]):
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.asarray(ctx, F).tobytes() + struct.pack("<2i", 16, 12) + struct.pack("<I", len(views)))
            for (kf, dp, w, h, k, P), _ in views:
                f.write(struct.pack("<4i", kf, dp, w, h) + np.asarray(k, F).tobytes() + np.ascontiguousarray(np.asarray(P, F).T).tobytes())
            f.write(struct.pack("<I", len(params)))
            for has, p in params:
                f.write(struct.pack("<i", has) + struct.pack("<i3I2f", *p))
            f.write(struct.pack("<f", 0.02) + struct.pack("<Q", len(r)) + r.tobytes())
        subprocess.run([exe, inp, out], check=True, timeout=120)
        raw = open(out, "rb").read()
        o = 0
        for (kf, dp, w, h, k, P), want in views:
            ok = raw[o]
            o += 1
            assert bool(ok) == (want is not None), (kf, dp, w, h, k)
            if not ok:
                continue
            gw, gh = struct.unpack_from("<2i", raw, o)
            f18 = np.frombuffer(raw, F, 18, o + 8)
            o += 8 + 72
            Rc, tc = mr.world_to_camera(np.asarray(P, F))
            assert (gw, gh) == want[:2] and f18[:9].tobytes() == Rc.tobytes() and f18[9:12].tobytes() == tc.tobytes()
            assert f18[12:].tobytes() == np.asarray(want[2], F).tobytes()
            if not kf:  # the same views pass the specification's own check
                mc.View(np.zeros((h, w), F), P, want[2])
        for (has, p), want in zip(params, want_params):
            ok = raw[o]
            o += 1
            assert bool(ok) == (want is not None), p
            if ok:
                assert struct.unpack_from("<i3I2f", raw, o) == tuple(float(x) if isinstance(x, np.floating) else x for x in want)
                o += 24
        m = struct.unpack_from("<Q", raw, o)[0]
        assert m == len(r) and raw[o + 8:] == r[np.argsort(r["key"])].tobytes()
