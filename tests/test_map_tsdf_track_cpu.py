"""Tracking a depth frame against the TSDF surface without a GPU: the exports and the two records' layout;
revo_amd.mapfile's vectorised tsdf_track_records against the per-pose, per-pixel loop tests/map_tsdf_track_ref.py on every shared case,
bit for bit, counts included; what the case table covers; poses that do not depend on each other; the refused arguments; the
convergence of the contract on the scene box and the wall's rank deficiency; the `surface-track` command; and
tests/cpp/tsdf_track_host.cpp, the header host and device code share."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, api, mapfile, tum
from revo_amd.settings import MapDfAlignInfo, MapTsdfTrackInfo, MapTsdfTrackParams

import map_carve_cases as cc
import map_tsdf_track_cases as kc
import map_tsdf_track_ref as kr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "small_map.rvm")
FIELDS = ("S", "matched", "considered", "skipped", "centre", "max_dist", "R", "T", "flags", "reserved")


def same_records(got, want, what):
    assert got.dtype.itemsize == want.dtype.itemsize == 208 and len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert np.asarray(g[f]).tobytes() == np.asarray(w[f]).tobytes(), (what, i, f, g[f], w[f])


def test_declared_exported_and_laid_out(tmp_path):
    names = ("revo_map_tsdf_track_eval", "revo_map_tsdf_track_system", "revo_map_tsdf_track")
    assert all(n in _lib.declared_symbols() and hasattr(_lib.lib(), n) for n in names)
    recs = {"revo_map_tsdf_track_params": (MapTsdfTrackParams, 32), "revo_map_tsdf_track_info": (MapTsdfTrackInfo, 208),
            "revo_map_df_align_info": (MapDfAlignInfo, 208)}
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
    # the record has revo_map_df_align_info's layout, and mapfile's and the loop's dtypes are it
    assert [(f, getattr(MapTsdfTrackInfo, f).offset) for f, _ in MapTsdfTrackInfo._fields_] == [(f, getattr(MapDfAlignInfo, f).offset) for f, _ in MapDfAlignInfo._fields_]
    for dt in (mapfile.TSDF_TRACK_DTYPE, kr.RECORD):
        assert dt.itemsize == 208 and [(f, dt.fields[f][1]) for f in FIELDS] == [(f, getattr(MapTsdfTrackInfo, f).offset) for f in FIELDS]


# ------------------------------------------------------------------------------------------------------------- the contract --
@pytest.mark.parametrize("name", list(kc.cases()))
def test_tsdf_track_records_follow_the_specification(name):
    c = kc.cases()[name]
    want, classes = kc.spec(name)
    a, kw = kc.args(c)
    got = mapfile.tsdf_track_records(*a, **kw)
    print(name, [(int(r["matched"]), int(r["considered"]), int(r["skipped"]), int(r["flags"])) for r in want])
    same_records(got, want, name)
    for r, cls, T in zip(want, classes, c["poses"]):
        if cls is None:
            assert r["flags"] == 1 and not r["S"].any() and r["matched"] == r["considered"] == r["skipped"] == 0
            continue
        h, w = c["depth"].shape
        assert r["considered"] == cls.size == -(-h // c["stride"]) * -(-w // c["stride"])
        assert r["matched"] + r["skipped"] + int((cls == kr.GATED).sum()) == r["considered"]
        # the vectorised classes are the loop's
        tr, md, st, mw, ce = mapfile.tsdf_track_params(c["trunc"], c["max_dist"], c["stride"], c["min_weight"], c["centre"])
        vec = mapfile.tsdf_track_terms(c["cells"], c["lo"], c["voxel"], tr, c["depth"], c["camera"], c["zrange"], T, md, st, mw, ce, classes=True)[4]
        assert np.array_equal(vec.reshape(cls.shape), np.array([0, 0, 0, 1, 2])[cls])


def test_the_case_table_covers_the_rules():
    """Conditions on the loop's own results: each class of pixel occurs where a case was built for it, and the marked cases meet the
    situation they were built for."""
    seen = set()
    for name, c in kc.cases().items():
        rec, classes = kc.spec(name)
        here = set()
        for cls in classes:
            if cls is not None:
                here |= {kr.CLASSES[k] for k in np.unique(cls)}
        assert set(c["kind"]) <= here, (name, c["kind"], here)
        seen |= here
    assert seen == set(kr.CLASSES)
    spec = lambda name: kc.spec(name)  # noqa: E731
    # an axis of one cell skips every pixel
    for n in ("1x5x5", "5x1x5", "5x5x1"):
        rec, classes = spec("axis of 1: " + n)
        assert all(np.all(cls == kr.OUTSIDE) for cls in classes) and np.all(rec["skipped"] == rec["considered"]) and not rec["S"].any()
    # the gate: on the lattice plane the cells hold 512, 513, -512, -513, 1024, 0 by (i + j) % 6; pixel (x, y) is the cell (x - 4, y - 3)
    rec, (cls,) = spec("the gate at equality")
    inside = cls[3:9, 4:12]
    i, j = np.meshgrid(np.arange(8), np.arange(6))
    kind = (i + j) % 6
    assert np.all(inside[np.isin(kind, (0, 2, 5))] == kr.ACCEPTED) and np.all(inside[np.isin(kind, (1, 3, 4))] == kr.GATED)
    assert np.all(np.delete(cls, np.s_[4:12], 1) == kr.OUTSIDE) and np.all(np.delete(cls, np.s_[3:9], 0) == kr.OUTSIDE)  # the rims: u = n - 1 is outside
    assert rec["max_dist"][0] == F(0.25) and rec["S"][0][27] == kr.round_exact([F(0.0625)] * int(((kind == 0) | (kind == 2)).sum()))
    _, (cls,) = spec("the gate given")
    assert np.all(cls[3:9, 4:12][np.isin(kind, (0, 1, 2, 3, 5))] == kr.ACCEPTED) and np.all(cls[3:9, 4:12][kind == 4] == kr.GATED)
    # e == 0 is accepted and adds nothing to S[21..27]
    rec, (cls,) = spec("zero sums")
    assert (cls == kr.ACCEPTED).sum() == 48 and not rec["S"][0][21:].any() and rec["S"][0][11] > 0
    # saturated: F = 1024 is e = trunc, G = 0: accepted only with max_dist = trunc, and then J = 0
    rec, _ = spec("saturated")
    assert rec["matched"][0] == 48 and not rec["S"][0][:27].any() and rec["S"][0][27] == F(48 * 0.25) and rec["matched"][1] > 0
    rec, (cls,) = spec("saturated and gated")
    assert rec["matched"][0] == 0 and (cls == kr.GATED).sum() == 48
    # every kind of hole is skipped before a point is formed; the two usable depths next to the range's ends are points outside the box
    _, (cls,) = spec("depths without a point")
    assert np.all(cls[4, 4:12] == kr.NO_DEPTH) and np.all(cls[5, 5:7] == kr.OUTSIDE) and (cls == kr.NO_DEPTH).sum() == 8
    _, (cls,) = spec("the rims")
    assert np.all(cls[3:9, 4:12] == kr.ACCEPTED) and (cls == kr.ACCEPTED).sum() == 48  # u = 0 is inside, u = n - 1 is not
    # the weight-0 corner takes the eight bases around it
    _, (cls, _) = spec("weight 0 in one corner")
    assert (cls == kr.INVALID_CELL).sum() == 4 and np.all(cls[5:7, 7:9] == kr.INVALID_CELL)  # the bases (1..2, 1..2, 2): the cells -1 .. 0 are the pixels 7 .. 8 x 5 .. 6
    # min_weight 0 counts as 1, 3 leaves fewer
    assert spec("min_weight 0")[0].tobytes() == spec("min_weight 1")[0].tobytes()
    assert spec("min_weight 3")[0]["matched"][0] < spec("min_weight 1")[0]["matched"][0]
    # strides: the visited pixels of stride k are every k-th of stride 1's
    for size in ("16x12", "33x17", "64x48"):
        full = spec("%s stride 1" % size)[1][0]
        for k in (2, 3, 8):
            assert np.array_equal(spec("%s stride %d" % (size, k))[1][0], full[::k, ::k]), (size, k)
    # flags
    rec, classes = spec("a pose that is no rotation, a pose that is not finite")
    assert rec["flags"].tolist() == [1, 0, 1] and np.isnan(rec["T"][2][1]) and rec["R"][0][3] == F(0.01)
    rec, _ = spec("65 poses")
    assert rec["flags"].sum() == 2 and rec["flags"][7] == rec["flags"][40] == 1


def test_poses_do_not_depend_on_each_other():
    for name in ("65 poses", "a pose that is no rotation, a pose that is not finite", "2 poses"):
        c = kc.cases()[name]
        a, kw = kc.args(c)
        together = mapfile.tsdf_track_records(*a, **kw)
        order = np.random.default_rng(3).permutation(len(c["poses"]))
        shuffled = mapfile.tsdf_track_records(*a[:-1], c["poses"][order], **kw)
        assert shuffled.tobytes() == together[order].tobytes()
        for i in (0, len(c["poses"]) - 1):
            assert mapfile.tsdf_track_records(*a[:-1], c["poses"][i], **kw).tobytes() == together[i:i + 1].tobytes()


def test_refused_arguments():
    c = kc.cases()["3x5x7 lo < 0"]
    a, kw = kc.args(c)
    cells, lo, voxel, trunc, depth, camera, zrange, poses = a
    ok = lambda *b, **k: mapfile.tsdf_track_records(*(b or a), **dict(kw, **k))  # noqa: E731
    base = ok()
    assert ok(max_dist=0).tobytes() == ok(max_dist=trunc / 2).tobytes() == base.tobytes() == ok(stride=0).tobytes() == ok(min_weight=0).tobytes()
    assert ok(max_dist=trunc)[0]["max_dist"] == F(trunc)
    for bad in (dict(max_dist=-0.1), dict(max_dist=float("nan")), dict(max_dist=float("inf")), dict(max_dist=float(np.nextafter(F(trunc), F(1)))),
                dict(stride=9), dict(stride=-1), dict(min_weight=-1), dict(centre=(0.0, float("nan"), 0.0)), dict(centre=(float("inf"), 0.0, 0.0))):
        with pytest.raises(ValueError):
            ok(**bad)
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ok(cells, lo, voxel, t, depth, camera, zrange, poses)
    for k, zr in (((0.0,) + camera[1:], zrange), (camera[:1] + (-1.0,) + camera[2:], zrange), (camera[:2] + (float("nan"),) + camera[3:], zrange),
                  (camera, (1.0, 1.0)), (camera, (-0.5, 1.0)), (camera, (0.1, float("inf")))):
        with pytest.raises(ValueError):
            ok(cells, lo, voxel, trunc, depth, k, zr, poses)
    for d in (depth[0], np.zeros((0, 4), F), np.zeros((2049, 1), F)):
        with pytest.raises(ValueError):
            ok(cells, lo, voxel, trunc, d, camera, zrange, poses)
    for p in (np.zeros((0, 4, 4), F), np.tile(np.eye(4, dtype=F), (4097, 1, 1))):
        with pytest.raises(ValueError):
            ok(cells, lo, voxel, trunc, depth, camera, zrange, p)
    for ce, l, v in ((cells.view(np.int64), lo, voxel), (cells, ((1 << 20) - 2, 0, 0), voxel), (cells, lo, 0.0), (cells, lo, float("nan"))):
        with pytest.raises(ValueError):
            ok(ce, l, v, trunc, depth, camera, zrange, poses)
    # a frame's pose is not an argument: a depth that is not finite is no error either
    holes = depth.copy()
    holes[0, 0] = np.nan
    assert ok(cells, lo, voxel, trunc, holes, camera, zrange, poses)[0]["considered"] == depth.size
    with pytest.raises(ValueError):
        mapfile.tsdf_track(cells, lo, voxel, trunc, depth, camera, zrange, np.full((4, 4), np.nan, F))
    with pytest.raises(ValueError):
        mapfile.tsdf_track(cells, lo, voxel, trunc, depth, camera, zrange, np.eye(4, dtype=F), max_iters=0)
    # the volume's own call needs a map's device
    with pytest.raises(ValueError):
        api.TsdfVolume(cells, lo, voxel, trunc).track((depth, camera, zrange), np.eye(4, dtype=F))


# ---------------------------------------------------------------------------------------------------------- convergence --
def test_convergence_on_the_scene_box():
    """mapfile.tsdf_track on the 64^3 scene box, view 0's depth image from every start of the table: CONVERGED, strictly nearer the
    truth than it started, and within twice the errors measured on the CPU (map_tsdf_track_cases.SCENE_END_*).  "Nearer" is
    measured where the model is: the RMS displacement of the box's corners (box_distance), one number for translation and rotation
    together -- a start that is a pure translation has no rotation error to improve on.  The measured errors lie below one voxel edge and
    below the angle one edge subtends over the box's half-diagonal: the sign and the scale of g are right."""
    cells, lo, trunc, views = kc.scene()
    k = cc.intrinsics320()
    starts, truth = kc.scene_starts()
    centre = kc.scene_centre()
    half_diagonal = 32 * np.sqrt(3.0) * cc.VOXEL
    assert len(starts) == 27
    assert kc.SCENE_END_ERR_T < cc.VOXEL and kc.SCENE_END_BOX < cc.VOXEL and kc.SCENE_END_ERR_R < cc.VOXEL / half_diagonal
    worst = [0.0, 0.0, 0.0]
    for name, T0 in starts.items():
        T, rec, it, status = mapfile.tsdf_track(cells, lo, cc.VOXEL, trunc, views[0][0], k[:4], k[4:], T0, stride=kc.SCENE_STRIDE, centre=centre)
        e0, e1 = kc.pose_error(T0, truth), kc.pose_error(T, truth)
        b0, b1 = kc.box_distance(T0, truth, lo, cells.shape, cc.VOXEL), kc.box_distance(T, truth, lo, cells.shape, cc.VOXEL)
        print("%-6s start %.4f m %.5f rad, box %.4f m -> end %.2e m %.2e rad, box %.2e m, %2d iterations, %s, %d matched"
              % ((name,) + e0 + (b0,) + e1 + (b1, it, ("converged", "limit", "lost")[status], int(rec["matched"]))))
        assert status == mapfile.ALIGN_CONVERGED, name
        assert b1 < b0, (name, b0, b1)
        assert e1[0] <= 2 * kc.SCENE_END_ERR_T and e1[1] <= 2 * kc.SCENE_END_ERR_R and b1 <= 2 * kc.SCENE_END_BOX, (name, e1, b1)
        worst = [max(worst[0], e1[0]), max(worst[1], e1[1]), max(worst[2], b1)]
    print("largest end error: %.3e m, %.3e rad, box %.3e m" % tuple(worst))


def test_the_wall_alone_is_rank_deficient():
    """A fronto-parallel wall constrains the depth and two tilts: the loop reports LOST and keeps the start, it does not solve."""
    c = kc.cases()["wall"]
    T0 = c["poses"][1]
    T, rec, it, status = mapfile.tsdf_track(c["cells"], c["lo"], c["voxel"], c["trunc"], c["depth"], c["camera"], c["zrange"], T0, min_matched=6)
    assert status == mapfile.ALIGN_LOST and it == 0 and T.tobytes() == T0.tobytes() and rec["matched"] >= 6
    H, _ = mapfile.df_align_system(rec)
    assert np.linalg.matrix_rank(H, tol=1e-6 * np.abs(H).max()) < 6


# ------------------------------------------------------------------------------------------------------------------ files --
def test_surface_track_command(tmp_path, capsys):
    header, rec = mapfile.read(GOLDEN)
    lo, hi, _ = mapfile.bounds_records(rec)
    blo, n = mapfile.padded_box(lo, hi, 2)
    voxel = header["voxel"]
    k = (16.0, 16.0, 31.5, 23.5, 0.1, 5.2)
    mid = (np.asarray(blo, np.float64) + np.asarray(n) / 2.0) * voxel
    # a corner of three walls in the map's bounds (8.25 x 3.75 x 3.75 m of 0.25 m voxels), seen by three cameras: depth images by
    # meeting every pixel's ray with the planes
    wall, trunc = (1.5, 0.9, 0.9), 1.0
    def corner_depth(T):
        x, y = np.meshgrid(np.arange(64), np.arange(48))
        d = np.stack([(x - k[2]) / k[0], (y - k[3]) / k[1], np.ones((48, 64))], -1) @ T[:3, :3].T.astype(np.float64)
        o = T[:3, 3].astype(np.float64)
        with np.errstate(all="ignore"):
            s = np.stack([np.where(d[..., a] > 1e-9, (mid[a] + wall[a] - o[a]) / d[..., a], np.inf) for a in range(3)], -1).min(-1)
        return np.where(np.isfinite(s) & (s > 0.1) & (s < 5.2), s, 0.0).astype(F)
    poses = [kc.about(kc.rc.at(np.eye(4, dtype=F), *(mid - (0.0, 0.0, 2.0))), mid, 1, a) for a in (0.0, 25.0, -20.0)]
    poses = [kc.about(T, mid, 0, 15.0) for T in poses]
    views = [(corner_depth(T), T, k) for T in poses]
    cells = mapfile.tsdf_records(voxel, blo, n, views, trunc)[0]
    vol, listed, folder, out = (str(tmp_path / x) for x in ("tsdf.npz", "truth.txt", "views", "refined.txt"))
    mapfile.write_tsdf(vol, cells, blo, voxel, trunc)
    from revo_amd import vo
    with open(listed, "w") as f:
        for T in poses:
            f.write(" ".join("%.9g" % x for x in T.reshape(-1)) + "\n")
    cam = ["--camera", "16", "16", "31.5", "23.5", "--zrange", "0.1", "5.2"]
    assert mapfile.main(["surface-views", vol, "--poses", listed, "-o", folder, "--size", "64", "48"] + cam) == 0
    truth = [T for _, T in tum.read_poses(os.path.join(folder, "poses.txt"))]
    # tracked from the poses the folder lists, the frames stay where they were ray-cast from
    assert mapfile.main(["surface-track", vol, "--views", folder, "-o", out, "--stride", "2"] + cam) == 0
    assert "3 frames" in capsys.readouterr().out
    for (ts, T), T0 in zip(tum.read_poses(out), truth):
        e = kc.pose_error(T, T0)
        assert e[0] < 0.25 * voxel and e[1] < 0.25 * voxel / 2.0, e  # a quarter of a voxel, and of the angle it subtends at the walls' 2 m
    # the listed poses a little off: the refined ones are mapfile.tsdf_track's, converged and nearer the truth
    off = [kc.about(T, mid, 2, 1.5) for T in truth]
    for T in off:
        T[:3, 3] += F([0.08, -0.06, 0.1])
    with open(os.path.join(folder, "poses.txt"), "w") as f:
        f.write("".join(line + "\n" for line in vo.tum_lines([(float(i), T) for i, T in enumerate(off)])))
    assert mapfile.main(["surface-track", vol, "--views", folder, "-o", out, "--stride", "2", "--max-dist", "0.8"] + cam) == 0
    capsys.readouterr()
    refined = tum.read_poses(out)
    frames = mapfile.read_views(folder, k[:4], k[4:])
    assert len(refined) == len(frames) == 3
    for (ts, T), (depth, T0, _), Tt in zip(refined, frames, truth):
        want = mapfile.tsdf_track(cells, blo, voxel, trunc, depth, k[:4], k[4:], T0, stride=2, max_dist=0.8)
        assert np.allclose(T, want[0], atol=1e-6)  # the text file holds nine decimals
        e0, e1 = kc.pose_error(T0, Tt), kc.pose_error(want[0], Tt)
        print("frame %d: %.4f m %.4f rad -> %.2e m %.2e rad, %d iterations" % ((int(ts),) + e0 + e1 + (want[2],)))
        assert want[3] == mapfile.ALIGN_CONVERGED and e1[0] < e0[0] and e1[1] < e0[1], (e0, e1)
    rows = [ln.split() for ln in open(out) if ln.startswith("# ") and ln.split()[1][0].isdigit()]
    assert len(rows) == 3 and all(r[-1] == "converged" for r in rows)
    assert mapfile.main(["surface-track", vol, "--views", folder, "-o", out, "--stride", "9"] + cam) == 1
    assert mapfile.main(["surface-track", vol, "-o", out]) == 2  # no views
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------- the shared header --
def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "tsdf_track_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "tsdf_track_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def _bits(x):
    return int(np.frombuffer(F(x).tobytes(), np.uint32)[0])


HOST_CASES = ("2x2x2", "axis of 1: 5x5x1", "3x5x7 lo < 0", "weight 0 in one corner", "min_weight 3", "the gate at equality", "the gate given", "zero sums",
              "saturated", "depths without a point", "the rims", "33x17 stride 3", "2 poses", "wall", "sphere")


def test_host_header(tmp_path):
    """revo_tsdf_track_host.h: the parameter rules and defaults, the lattice of a stride, the place of a point at the box's rims, the gate
    at equality, and the class and the 28 terms of every visited pixel of the chosen cases against the loop, bit for bit."""
    exe = _host(tmp_path)
    nan, inf = float("nan"), float("inf")
    # (given?, trunc, max_dist, stride, min_weight, centre, reserved)
    params = [(0, 0.5, 0.0, 0, 0, (0, 0, 0), (0, 0)), (1, 0.5, 0.0, 0, 0, (0, 0, 0), (0, 0)), (1, 0.5, 0.5, 8, 3, (1, -2, 3), (0, 0)), (1, 0.3, 0.1, 1, 0, (0, 0, 0), (0, 0)),
              (1, 0.5, float(np.nextafter(F(0.5), F(1))), 1, 1, (0, 0, 0), (0, 0)), (1, 0.5, -0.1, 1, 1, (0, 0, 0), (0, 0)), (1, 0.5, nan, 1, 1, (0, 0, 0), (0, 0)),
              (1, 0.5, 0.1, 9, 1, (0, 0, 0), (0, 0)), (1, 0.5, 0.1, 1, 1, (0, inf, 0), (0, 0)), (1, 0.5, 0.1, 1, 1, (0, 0, 0), (1, 0)), (1, 0.5, 0.1, 1, 1, (0, 0, 0), (0, 1))]
    want_params = [[_bits(0.25), 1, 1, 0, 0, 0], [_bits(0.25), 1, 1, 0, 0, 0], [_bits(0.5), 8, 3, _bits(1), _bits(-2), _bits(3)],
                   [_bits(F(0.1)), 1, 1, 0, 0, 0]] + [None] * 7
    lattices = [(1, 1), (16, 1), (16, 2), (17, 2), (33, 8), (2048, 8), (7, 8), (8, 8), (9, 8)]
    rng = np.random.default_rng(29)
    # g, lo, n at the voxel edge 1/8: u = g / voxel - (lo + 0.5); the rims are u = 0 and u = n - 1
    axes = [(F(0.0625), 0, 5), (np.nextafter(F(0.0625), F(0)), 0, 5), (F(0.5625), 0, 5), (np.nextafter(F(0.5625), F(0)), 0, 5), (F(-0.3125), -3, 2),
            (F(-0.1875), -3, 2), (F(0.2), 0, 1), (F(nan), 0, 5), (F(inf), 0, 5), (F(-0.0), -1, 9)]
    axes += [(F(rng.uniform(-2, 2)), int(rng.integers(-9, 3)), int(rng.integers(1, 12))) for _ in range(40)]
    blob = struct.pack("<I", len(params))
    for has, tr, md, st, mw, ce, res in params:
        blob += struct.pack("<IffII3f2I", has, tr, md, st, mw, *ce, *res)
    blob += struct.pack("<I", len(lattices)) + b"".join(struct.pack("<ii", *x) for x in lattices)
    blob += struct.pack("<I", len(axes)) + b"".join(struct.pack("<fii", *x) for x in axes)
    blob += struct.pack("<I", len(HOST_CASES))
    want_px = []
    for name in HOST_CASES:
        c = kc.cases()[name]
        tr, md, st, mw, ce = kr.params(c["trunc"], c["max_dist"], c["stride"], c["min_weight"], c["centre"])
        h, w = c["depth"].shape
        blob += struct.pack("<3i3i", *c["lo"], *c["cells"].shape) + np.ascontiguousarray(c["cells"]).tobytes()
        blob += struct.pack("<ff6f", c["voxel"], c["trunc"], *c["camera"], *c["zrange"]) + struct.pack("<fII3f", md, st, mw, *ce)
        blob += struct.pack("<ii", w, h) + np.ascontiguousarray(c["depth"], F).tobytes()
        poses = [T for T in c["poses"] if np.all(np.isfinite(T)) and kr.is_orthogonal(T[:3, :3])]
        blob += struct.pack("<I", len(poses)) + b"".join(np.ascontiguousarray(T[:3, :4].T, F).tobytes() for T in poses)  # R column-major, then t
        kq = F(tr / F(1024.0))
        cam = tuple(F(x) for x in c["camera"] + c["zrange"])
        with np.errstate(all="ignore"):
            for T in poses:
                for y in range(0, h, st):
                    for x in range(0, w, st):
                        cls, terms = kr.pixel(c["cells"], c["lo"], F(c["voxel"]), kq, mw, cam, T[:3, :3], T[:3, 3], md, ce, x, y, c["depth"][y, x])
                        want_px.append([[0, 0, 0, 1, 2][cls]] + ([_bits(t) for t in terms] if terms is not None else []))
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-3000:])
    rows = [ln.split() for ln in r.stdout.decode().splitlines()]
    by = lambda key: [[int(x) for x in row[1:]] if row[1:] != ["refused"] else None for row in rows if row[0] == key]  # noqa: E731
    assert by("params") == want_params
    assert by("lattice") == [[-(-n // s)] for n, s in lattices]
    want = []
    with np.errstate(all="ignore"):
        for g, lo, n in axes:
            u = F(F(g / F(0.125)) - F(F(lo) + F(0.5)))
            b = np.floor(u)
            want.append([1, int(b), _bits(F(u - b))] if np.isfinite(u) and 0 <= b <= n - 2 else [0])
    assert by("axis") == want
    # u == 0 and one step below it; u == n - 1 and one step below it; a box of two cells at u == 0 and at u == 1; an axis of 1; not finite
    assert [w[0] for w in want[:9]] == [1, 0, 0, 1, 1, 0, 0, 0, 0] and want[0][1:] == [0, 0] and want[3][1] == 3 and want[4][1:] == [0, 0]
    got_px = by("pixel")
    assert len(got_px) == len(want_px) and got_px == want_px
    assert {row[0] for row in want_px} == {0, 1, 2}
