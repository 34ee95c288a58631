"""View gain without a GPU: the export and the records' layout; revo_amd.mapfile's vectorised gain_records against
the per-pose, per-cell specification tests/map_gain_ref.py on every shared case; what the wall scene's poses must see; the
identity with observe; the independence of a pose's record from the other poses of a call; next_view_records on the wall
scene; the gain and next-view commands on the golden map; and tests/cpp/gain_host.cpp: the header host and device code share,
with the cull against brute force."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, mapfile
from revo_amd.settings import MapGain, MapGainInfo, MapGainParams

import map_carve_ref as mc
import map_gain_cases as gc
import map_gain_ref as gr

F = np.float32
RAW = mapfile.RAW_DTYPE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "small_map.rvm")
NAMES = list(gc.cases()) + ["device poses"]


def _case(name):
    return gc.device_case() if name == "device poses" else gc.cases()[name]


def _gain(c, poses=None, device_poses=False, **over):
    return mapfile.gain_records(c["rec"].astype(RAW), gc.V, c["lo"], c["n"], c["seen"], c["view"], c["poses"] if poses is None else poses,
                                device_poses=device_poses, **dict(c["params"], **over))


def _fields(g):
    return np.stack([g[f] for f in gr.FIELDS], 1)


def test_declared_exported_and_laid_out(tmp_path):
    assert "revo_map_view_gain" in _lib.declared_symbols() and hasattr(_lib.lib(), "revo_map_view_gain")
    recs = {"revo_map_gain_params": (MapGainParams, 32), "revo_map_gain": (MapGain, 32), "revo_map_gain_info": (MapGainInfo, 64)}
    body = ""
    for cname, (cls, _) in recs.items():
        body += '  printf("%s %%zu\\n", sizeof(%s));\n' % (cname, cname)
        for f, _t in cls._fields_:
            body += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (cname, f, cname, f)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "revo_hip.h"\nint main(void) {\n%s  return 0;\n}\n' % body)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = dict(ln.split(None, 1) for ln in subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines())
    for cname, (cls, size) in recs.items():
        assert int(got[cname]) == size == C.sizeof(cls)
        for f, _t in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)
    assert mapfile.GAIN_INFO_KEYS == gr.INFO_KEYS == tuple(f for f, _ in MapGainInfo._fields_)
    assert mapfile.GAIN_DTYPE.names[:4] == gr.FIELDS and mapfile.GAIN_DTYPE.itemsize == C.sizeof(MapGain)
    assert [mapfile.GAIN_DTYPE.fields[f][1] for f in gr.FIELDS] == [getattr(MapGain, f).offset for f in gr.FIELDS]


@pytest.mark.parametrize("name", NAMES)
def test_gain_records_follow_the_specification(name):
    c = _case(name)
    want, info, _ = gc.spec(name)
    got = _gain(c, device_poses=name == "device poses")
    print(name, info, gc.as_array(want)[:4].tolist())
    assert got.dtype == mapfile.GAIN_DTYPE and np.array_equal(_fields(got), gc.as_array(want)) and not got["reserved"].any()
    assert got.info == info and info["cells"] == int(np.prod(c["n"])) and info["poses"] == len(c["poses"])
    assert info["rays"] == c["view"][1][0] * c["view"][1][1] * sum(gr.pose_ok(T) for T in c["poses"])
    assert np.all(got["unknown_free"].astype(int) + got["unknown_surface"] <= got["unknown_inside"]) and np.all(got["unknown_inside"] <= info["unknown"])


def test_what_the_cases_are_built_for():
    w = gc.wall()
    behind = np.zeros(w["n"], bool)
    behind[14:] = True
    behind = behind.reshape(-1)
    rec, info, cls = gc.spec("wall, real volume")   # a miss is a hole
    assert rec[0]["hits"] == 16 * 12 and rec[0]["unknown_free"] == 0 == rec[0]["unknown_surface"]   # facing the wall: every ray ends on it
    assert not np.isin(cls[0][behind], (mc.FREE, mc.CONFIRMED)).any()
    assert rec[1]["unknown_free"] > 0 and np.isin(cls[1][behind], (mc.FREE,)).sum() == rec[1]["unknown_free"]  # facing the gap: all of it behind
    assert 0 < rec[1]["hits"] < 16 * 12 and rec[1]["unknown_surface"] > 0                                      # the far wall's cells
    holes, _, _ = gc.spec("wall, real volume")
    filled, _, cls = gc.spec("wall, miss depth")     # a miss reads as 2 m of free space
    assert filled[0]["unknown_free"] == 0 and filled[1]["unknown_free"] > holes[1]["unknown_free"]
    assert filled[1]["unknown_surface"] > holes[1]["unknown_surface"] and [r["hits"] for r in filled] == [r["hits"] for r in holes]
    rec, info, _ = gc.spec("wall, all seen")
    assert info["unknown"] == 0 and all(r["unknown_inside"] == 0 for r in rec) and all(r["hits"] > 0 for r in rec)
    rec, info, _ = gc.spec("wall, looking away")
    assert rec[0]["hits"] > 0 and rec[0]["unknown_inside"] == 0 and info["unknown"] > 0
    rec, info, cls = gc.spec("wall, through each face")
    assert all(r["unknown_inside"] > 0 for r in rec) and all(r["unknown_inside"] < info["unknown"] // 8 for r in rec)
    inside = (cls > 0).reshape(6, *w["n"])
    for j, (axis, last) in enumerate([(a, s > 0) for a in range(3) for s in (1, -1)]):  # the frustum reaches the face it looks at
        assert inside[j].take(-1 if last else 0, axis=axis).any() and not inside[j].take(0 if last else -1, axis=axis).any()
    rec, info, _ = gc.spec("wall, nearer than zmin")
    assert rec[0] == dict.fromkeys(gr.FIELDS, 0) and info["rays"] == 192
    rec, info, _ = gc.spec("empty map")
    assert all(r["hits"] == 0 and r["unknown_free"] == r["unknown_inside"] > 0 for r in rec)
    assert all(r["unknown_free"] == 0 and r["unknown_inside"] > 0 for r in gc.spec("empty map, holes")[0])
    rec, info, _ = gc.spec("device poses")
    assert [j for j, r in enumerate(rec) if r == dict.fromkeys(gr.FIELDS, 0)] == [3, 40, 64] and info["rays"] == 62 * 64
    assert gc.spec("min_views 0")[1]["unknown"] < gc.spec("min_views 2")[1]["unknown"]


@pytest.mark.parametrize("name", ["wall, real volume", "wall, miss depth", "box 9x7x5", "tail 3x3x5", "radius 2", "empty map", "few steps"])
def test_the_identity_with_observe(name):
    """With min_views 1, unknown_free + unknown_surface counts exactly the unknown cells whose byte changes under an accumulating
    observe with the predicted image (its misses replaced) as a raw view."""
    c = gc.cases()[name]
    p = dict(c["params"])
    assert p.get("min_views", 1) == 1
    rec = c["rec"].astype(RAW)
    k, size = c["view"]
    got = _gain(c)
    solid = mapfile.solid_cells(rec, np.asarray(c["lo"]), np.asarray(c["n"]), p.get("min_count", 1))[0]
    unknown = ~mapfile.seen_known(c["seen"], 1, solid)
    for j, T in enumerate(c["poses"]):
        D = mapfile.raycast_records(rec, gc.V, [(T, k, size)], p.get("min_count", 1), p.get("max_steps", 4096))["depth"][0]
        if p.get("miss_depth", 0.0):
            D = np.where(D == 0, F(p["miss_depth"]), D)
        after = mapfile.observe_records(gc.V, c["lo"], c["n"], [(D, T, k)], p.get("radius", 1), p.get("margin"), p.get("margin_rel", 0.0), seen=c["seen"])[0]
        changed = int(((after != c["seen"]) & unknown).sum())
        print(name, j, changed, got[j])
        assert changed == int(got[j]["unknown_free"]) + int(got[j]["unknown_surface"])
        assert int(((after & 0x80 != 0) & unknown).sum()) == int(got[j]["unknown_surface"])


def test_a_record_does_not_depend_on_the_call():
    c = gc.cases()["65 poses"]
    whole = _gain(c)
    rng = np.random.default_rng(9)
    perm = rng.permutation(65)
    assert np.array_equal(_gain(c, poses=c["poses"][perm]), whole[perm])
    parts = [_gain(c, poses=c["poses"][a:b]) for a, b in ((0, 1), (1, 30), (30, 65))]
    assert np.array_equal(np.concatenate(parts), whole)
    assert sum(p.info["unknown_free"] for p in parts) == whole.info["unknown_free"] and all(p.info["unknown"] == whole.info["unknown"] for p in parts)
    assert np.array_equal(_gain(c, poses=c["poses"][7]), whole[7:8])


def test_arguments_are_refused():
    c = gc.cases()["box 3x5x7"]
    for bad in (dict(radius=4), dict(radius=-1), dict(margin=-1.0), dict(margin=np.nan), dict(margin_rel=np.inf), dict(miss_depth=0.05),
                dict(miss_depth=float(gc.sc.ZMAX)), dict(miss_depth=-1.0), dict(miss_depth=np.nan), dict(max_steps=0), dict(max_steps=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            _gain(c, **bad)
    for kind in ("nan", "inf", "skew"):
        with pytest.raises(ValueError):
            _gain(c, poses=np.stack([gc.sc.I4, gc.bad_pose(kind)]))
        assert not _fields(_gain(c, poses=np.stack([gc.sc.I4, gc.bad_pose(kind)]), device_poses=True))[1].any()
    with pytest.raises(ValueError):
        _gain(c, poses=np.zeros((0, 4, 4), F))
    with pytest.raises(ValueError):
        _gain(c, poses=np.broadcast_to(gc.sc.I4, (4097, 4, 4)))
    with pytest.raises(ValueError):
        mapfile.gain_records(c["rec"].astype(RAW), gc.V, c["lo"], c["n"], c["seen"][1:], c["view"], c["poses"])
    with pytest.raises(ValueError):
        mapfile.gain_records(c["rec"].astype(RAW), gc.V, c["lo"], c["n"], c["seen"], ((8.5, 0.0, 7.5, 5.5, 0.1, 5.2), (16, 12)), c["poses"])
    with pytest.raises(ValueError):
        mapfile.gain_records(c["rec"].astype(RAW), gc.V, c["lo"], c["n"], c["seen"], (gc.KC, (16, 2049)), c["poses"])


# ------------------------------------------------------------------------------------------------------------ next view --
def _next(**kw):
    w = gc.wall()
    args = dict(headings=4, stride=4, miss_depth=2.0, up=(0, 0, 1))   # the scene's up is +z: yaw 0 looks down +x
    args.update(kw)
    return mapfile.next_view_records(w["rec"].astype(RAW), gc.V, w["lo"], w["n"], w["seen"], w["start"], gc.V, gc.VIEW, **args)


def test_next_view_on_the_wall_scene():
    w = gc.wall()
    r = _next()
    print(r["cell"], r["heading"], r["record"], r["scores"][r["index"]], len(r["cells"]))
    free = mapfile.known_field_records(w["rec"].astype(RAW), w["lo"], w["n"], w["seen"])[0] >= 1   # known, not solid, not next to unseen space
    # the candidates: reachable cells on the lattice of absolute indices, in ascending cell order; four poses at each
    cells = r["cells"].astype(np.int64)
    assert len(cells) > 4 and np.all(cells % 4 == 0) and len(r["poses"]) == 4 * len(cells) == len(r["scores"]) == len(r["gain"])
    lin = (cells[:, 0] * w["n"][1] + cells[:, 1]) * w["n"][2] + cells[:, 2]
    assert np.all(np.diff(lin) > 0) and free[tuple(cells.T)].all() and np.all(r["cost"][tuple(cells.T)] != mapfile.PLAN_NONE)
    assert np.array_equal(r["poses"][:, :3, 3].reshape(-1, 4, 3)[:, 0], ((cells.astype(F) + F(0.5)) * F(gc.V)))
    assert all(mapfile.gain_pose_ok(T) for T in r["poses"])
    # the best pose stands in front of the open cells and looks down +x, through the gap
    assert r["heading"] == r["index"] % 4 and np.array_equal(r["cell"], cells[r["index"] // 4]) and np.array_equal(r["pose"], r["poses"][r["index"]])
    assert r["pose"][0, 2] > 0.99 and r["cell"][1] >= 12 and int(r["record"]["unknown_free"]) > 0
    metres = r["cost"][tuple(cells.T)].astype(np.float64) * gc.V / 3.0
    want = r["gain"]["unknown_free"].astype(np.float64) / (1.0 + np.repeat(metres, 4))
    assert np.array_equal(r["scores"], want) and r["index"] == int(np.argmax(want)) and want[r["index"]] > 0
    # the path: from the position back to the start over known free cells
    path, status, cost = r["path"]
    assert status == mapfile.PLAN_REACHED and path[0].tolist() == r["cell"].tolist() and path[-1].tolist() == list(w["start"])
    assert free[tuple(path.astype(np.int64).T)].all() and cost == int(r["cost"][tuple(r["cell"])])
    # ties go to the lowest index: with no weight on the way and every view's gain the same (nothing is unknown), pose 0
    flat = mapfile.next_view_records(w["rec"].astype(RAW), gc.V, w["lo"], w["n"], np.full(w["n"], 0x7F, np.uint8), w["start"], gc.V, gc.VIEW, headings=4, up=(0, 0, 1),
                                     max_candidates=12)
    assert flat["index"] == 0 and not flat["scores"].any()
    # max_candidates cuts the positions, not the poses of one; a heavier weight can only move the choice towards the start
    few = _next(max_candidates=11)
    assert len(few["cells"]) == 2 and np.array_equal(few["cells"], r["cells"][:2]) and np.array_equal(few["scores"], r["scores"][:8])
    near = _next(weight=50.0)
    assert int(near["cost"][tuple(near["cell"])]) <= int(r["cost"][tuple(r["cell"])])
    eight = _next(headings=8, max_candidates=16)
    assert len(eight["poses"]) == 8 * len(eight["cells"]) and np.array_equal(eight["poses"][::2], r["poses"][:len(eight["poses"]) // 2])
    # nothing reachable: a start in unseen space; no stride; fewer candidates than one position's headings
    with pytest.raises(ValueError):
        _next_from((20, 8, 8))
    with pytest.raises(ValueError):
        _next(stride=0)
    with pytest.raises(ValueError):
        _next(max_candidates=3)


def _next_from(start):
    w = gc.wall()
    return mapfile.next_view_records(w["rec"].astype(RAW), gc.V, w["lo"], w["n"], w["seen"], start, gc.V, gc.VIEW, headings=4, up=(0, 0, 1))


def test_next_view_poses():
    cells = np.array([[0, 0, 0], [-3, 5, 9]])
    T = mapfile.next_view_poses(cells, 0.25, 4).reshape(2, 4, 4, 4)
    assert T.dtype == F and np.array_equal(T[1, :, :3, 3], np.broadcast_to(F([-0.625, 1.375, 2.375]), (4, 3)))
    # up = -y: yaw 0 looks down +z with the image's y along +y (the camera frame is the world's), then turns about -y
    assert np.allclose(T[0, 0, :3, :3], np.eye(3), atol=1e-7)
    assert np.allclose(T[0, 1, :3, 2], [-1, 0, 0], atol=1e-7) and np.allclose(T[0, 2, :3, 2], [0, 0, -1], atol=1e-7)
    assert np.allclose(T[0, :, :3, 1], np.broadcast_to([0, 1, 0], (4, 3)), atol=1e-7)
    for up in ((0, 0, 1), (1, 1, 0), (0, -2, 0.5)):
        for M in mapfile.next_view_poses(cells[:1], 0.25, 5, up):
            assert mapfile.gain_pose_ok(M) and abs(float(M[:3, 2] @ np.asarray(up))) < 1e-6 and float(M[:3, 1] @ np.asarray(up)) < 0
    with pytest.raises(ValueError):
        mapfile.next_view_poses(cells, 0.25, 0)
    with pytest.raises(ValueError):
        mapfile.next_view_poses(cells, 0.25, 4, (0, 0, 0))


# ---------------------------------------------------------------------------------------------------------------- tools --
def test_command_line(tmp_path, capsys):
    header, rec = mapfile.read(GOLDEN)
    lo, hi, _ = mapfile.bounds_records(rec)
    lo, n = mapfile.padded_box(lo, hi, 2)
    k, size = (16.0, 16.0, 15.5, 11.5, 0.1, 5.2), (32, 24)
    T2 = np.eye(4, dtype=F)
    T2[0, 3] = -2.0
    flat = np.full((24, 32), 3.0, F)
    seen = mapfile.observe_records(header["voxel"], lo, n, [(flat, np.eye(4, dtype=F), k)])[0]
    seen_path, poses_txt, gain_txt, pose_txt = (str(tmp_path / x) for x in ("seen.npz", "poses.txt", "gain.txt", "pose.txt"))
    mapfile.write_seen(seen_path, seen, lo, header["voxel"])
    poses = np.stack([np.eye(4, dtype=F), T2, gc.look((0.5, 0.0, 0.0), 0)])
    with open(poses_txt, "w") as f:
        f.write("# three poses\n" + "".join(" ".join("%.9g" % x for x in (T.reshape(-1) if i != 1 else T[:3].reshape(-1))) + "\n" for i, T in enumerate(poses)))
    cam = ["--camera", "16", "16", "15.5", "11.5", "--size", "32", "24", "--zrange", "0.1", "5.2"]
    assert mapfile.main(["gain", GOLDEN, "--seen", seen_path, "--poses", poses_txt, "--miss-depth", "2.5", "--radius", "2", "-o", gain_txt] + cam) == 0
    want = mapfile.gain_records(rec, header["voxel"], lo, n, seen, (k, size), poses, radius=2, miss_depth=2.5)
    assert np.loadtxt(gain_txt, dtype=np.int64).reshape(-1, 4).tolist() == _fields(want).tolist() and want["unknown_free"].any()
    assert np.array_equal(mapfile.read_poses(poses_txt), poses)
    free = np.argwhere(mapfile.seen_free(seen) & (mapfile.known_field_records(rec, lo, n, seen)[0] >= 1)) + lo
    start = free[len(free) // 2]
    nv = ["next-view", GOLDEN, "--seen", seen_path, "--start"] + [str(x) for x in start] + ["--clearance", str(header["voxel"]), "--headings", "4",
                                                                                             "--stride", "3", "--max-candidates", "24", "--miss-depth", "2.5", "-o", pose_txt]
    assert mapfile.main(nv + cam) == 0
    r = mapfile.next_view_records(rec, header["voxel"], lo, n, seen, start, header["voxel"], (k, size), headings=4, stride=3, max_candidates=24, miss_depth=2.5)
    assert np.array_equal(mapfile.read_pose(pose_txt), r["pose"]) and int(r["record"]["unknown_free"]) > 0
    # refused: a volume at another voxel edge, a bad parameter, an unreachable start; a missing -o or camera is a usage error
    mapfile.write_seen(str(tmp_path / "other.npz"), seen, lo, 0.5)
    assert mapfile.main(["gain", GOLDEN, "--seen", str(tmp_path / "other.npz"), "--poses", poses_txt, "-o", gain_txt] + cam) == 1
    assert mapfile.main(["gain", GOLDEN, "--seen", seen_path, "--poses", poses_txt, "--miss-depth", "9", "-o", gain_txt] + cam) == 1
    unseen = np.argwhere(~mapfile.seen_known(seen, 1, mapfile.solid_cells(rec, lo, n)[0]))[0] + lo
    assert mapfile.main(nv[:4] + ["--start"] + [str(x) for x in unseen] + nv[8:] + cam) == 1
    assert mapfile.main(["gain", GOLDEN, "--seen", seen_path, "--poses", poses_txt] + cam) == 2
    assert mapfile.main(["gain", GOLDEN, "--seen", seen_path, "--poses", poses_txt, "-o", gain_txt]) == 2
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------- the shared header --
def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "gain_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "gain_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def test_host_header(tmp_path):
    """revo_gain_host.h: every parameter rule and the defaults; a pose's descriptor against the specification's transform and
    the pose rules; and the cull -- over random poses, cameras and boxes no cell outside its range has a class other than
    OUTSIDE."""
    exe = _host(tmp_path)
    voxel, zmin, zmax = F(0.02), F(0.1), F(5.2)
    ok = (1, 1, 0.1, 0.0, 0.0, 4096, 0, 0)
    params = [(0, (9, 9, 9.0, 9.0, 9.0, 9, 9, 9)), (1, (0, 0, 0.0, 0.0, 0.0, 1, 0, 0)), (1, (3, 7, 0.5, 0.25, 2.0, 1 << 20, 0, 0))]
    params += [(1, ok[:i] + (v,) + ok[i + 1:]) for i, v in ((0, 4), (0, -1), (2, -0.1), (2, np.nan), (2, np.inf), (3, -1.0), (3, np.inf), (3, np.nan),
                                                           (4, 0.1), (4, 5.2), (4, -1.0), (4, np.nan), (4, 0.05), (5, 0), (5, (1 << 20) + 1), (6, 1), (7, 1))]
    want_params = [(1, 1, voxel, F(0), F(0), 4096), (0, 1, F(0), F(0), F(0), 1), (3, 7, F(0.5), F(0.25), F(2.0), 1 << 20)] + [None] * 17
    poses = [gc.sc.I4, gc.nudged(gc.sc.I4, 3, 0.5), gc.look((1.0, -2.0, 3.0), 1, -1), gc.bad_pose("nan"), gc.bad_pose("inf"), gc.bad_pose("skew"),
             np.diag(F([1, 1, -1, 1]))] + [gc.nudged(gc.sc.I4, 10 + i, 2.0) for i in range(20)]
    blob = struct.pack("<fffI", voxel, zmin, zmax, len(params))
    for has, p in params:
        blob += struct.pack("<iiIfffIII", has, *p)
    blob += struct.pack("<I", len(poses)) + b"".join(np.ascontiguousarray(np.asarray(T, F).T).tobytes() for T in poses)
    blob += struct.pack("<II", 4000, 25)
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = (tmp_path / "out.bin").read_bytes()
    o = 0
    for want in want_params:
        good, o = out[o], o + 1
        assert good == (want is not None)
        if good:
            got, o = struct.unpack_from("<iIfffIII", out, o), o + 32
            assert got[:2] == want[:2] and got[5:] == (want[5], 0, 0)
            assert all(F(g).tobytes() == w.tobytes() for g, w in zip(got[2:5], want[2:5]))
    for T in poses:
        good, o = out[o], o + 1
        d, o = np.frombuffer(out, "<f4", 24, o), o + 96
        assert good == gr.pose_ok(T) == mapfile.gain_pose_ok(np.asarray(T, F))
        if good:
            Rc, tc = gr.mr.world_to_camera(T)
            assert d[:3].tobytes() == np.asarray(T, F)[:3, 3].tobytes() and d[3:12].tobytes() == np.ascontiguousarray(np.asarray(T, F)[:3, :3]).tobytes()
            assert d[12:21].tobytes() == Rc.tobytes() and d[21:].tobytes() == tc.tobytes()
        else:
            assert not d.any()
    trials, cells, inside, violations, visited = struct.unpack_from("<5Q", out, o)
    assert o + 40 == len(out)
    print("cull: %d trials, %d cells, %d inside a view, %d left to visit, %d violations" % (trials, cells, inside, visited, violations))
    assert violations == 0 and trials > 3000 and inside > cells // 20 and inside <= visited < cells
