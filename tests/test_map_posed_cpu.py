"""Maps under a pose without a GPU: the exports and the info record's layout, revo_amd.mapfile.pose_records against the
per-voxel loop of tests/map_posed_ref.py bit for bit on the synthetic scene and on hand-made records, the exact properties of
hand-made records (identity, whole-voxel translation, conservation, drops, min_count, refusals), merge followed by subtract,
`python -m revo_amd.mapfile transform`, and the canonicalisation of revo_map_pose_raw's host output (tests/cpp/pose_host.cpp)."""
import ctypes as C
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, mapfile, synth
from revo_amd.settings import ImgPyramidSettings, MapPoseInfo, PLANE_EDGES

import map_posed_cases as pc
import map_posed_ref as mp
import map_records_ref as mrr
import voxel_map_ref as ref

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I4 = pc.I4
S320 = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
KF_TWISTS = ([0, 0, 0, 0, 0, 0], [0.05, 0.01, 0.0, 0.0, 0.03, 0.0])
D_SMALL = synth.se3_exp(np.array([0.006, -0.004, 0.005, 0.002, -0.001, 0.0015]))  # DESIGN 16's D
RAW = mapfile.RAW_DTYPE


@functools.lru_cache(maxsize=None)
def _edge_scene(voxel):
    """The two-keyframe 320x240 synthetic scene (seeds 902 and 903) in edge mode: level-0 edge pixels of the oracle's pyramids."""
    from oracle import ro
    r = ref.VoxelMapRef(voxel)
    for sd, tw in zip((902, 903), KF_TWISTS):
        bgr, depth = synth.make_pair(sd, S320)["ref"]
        edges = ro.Pyramid(S320, bgr, depth).read(PLANE_EDGES, 0)
        xyz, rgb = ref.select_points(depth, edges, bgr, S320.fx, S320.fy, S320.cx, S320.cy, S320.depth_min, S320.depth_max, False)
        r.integrate(xyz, rgb, synth.se3_exp(np.asarray(tw, np.float64)).astype(F))
    return mrr.records_of(r)


def _same(rec, T, voxel_dst, min_count=1):
    """mapfile.pose_records against the reference loop, bit for bit; -> (records, info)."""
    want, winfo = mp.pose_raw(rec, T, voxel_dst, min_count)
    got, ginfo = mapfile.pose_records(rec.astype(RAW), T, voxel_dst, min_count)
    assert got.dtype == RAW and got.tobytes() == want.tobytes() and ginfo == winfo
    return got, ginfo


def test_declared_exported_and_laid_out(tmp_path):
    for name in ("revo_map_pose_raw", "revo_map_merge_posed", "revo_map_subtract_posed"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "revo_hip.h"\n'
                   '#define F(m) printf(#m " %zu\\n", offsetof(revo_map_pose_info, m));\n'
                   'int main(void) {\n  printf("info %zu\\n", sizeof(revo_map_pose_info));\n'
                   '  F(voxels_in) F(voxels_moved) F(voxels_dropped) F(voxels_skipped) F(points_moved) F(points_dropped) F(points_skipped) '
                   'F(reserved)\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines())
    assert int(got["info"]) == 64 == C.sizeof(MapPoseInfo)
    for i, (name, _) in enumerate(MapPoseInfo._fields_):
        assert int(got[name]) == getattr(MapPoseInfo, name).offset == 8 * i, name
    assert [n for n, _ in MapPoseInfo._fields_][:7] == list(mp.INFO_KEYS)


@pytest.mark.parametrize("voxel_dst", [0.02, 0.04])
def test_pose_records_equal_the_reference_on_the_scene(voxel_dst):
    rec = _edge_scene(0.02)
    assert len(rec) > 3000
    for mc in (1, 2):
        out, info = _same(rec, D_SMALL.astype(F), voxel_dst, mc)
        assert info["voxels_in"] == len(rec) and info["voxels_dropped"] == 0
        assert info["voxels_moved"] == int((rec["count"] >= mc).sum()) >= len(out) > 1000
        assert int(out["count"].sum()) == info["points_moved"] == int(rec["count"][rec["count"] >= mc].sum())
        assert out["sum_bgr"].sum(0).tolist() == rec["sum_bgr"][rec["count"] >= mc].sum(0).tolist()
    coarse = _same(rec, D_SMALL.astype(F), 0.04)[0]
    assert len(coarse) < len(_same(rec, D_SMALL.astype(F), 0.02)[0])


def test_pose_records_equal_the_reference_on_hand_made_records():
    rot = synth.se3_exp(np.array([0.3, -0.2, 0.1, 0.4, -0.3, 0.2])).astype(F)
    for rec, voxel in ((pc.singles(), 0.02), (pc.counted(), pc.V6)):
        for T in (I4, rot, pc.translation([0.011, 0.0, -0.007])):
            for vd in (voxel, 2 * voxel, 0.013):
                _same(rec, T, vd)
                _same(rec, T, vd, 2)
    rec, T, vd = pc.edge_cases()
    _same(rec, T, vd)
    rec, T = pc.last_index()
    _same(rec, T, 2.0 ** -9)
    _same(np.zeros(0, mrr.DTYPE), rot, 0.02)
    # 3x4 and 4x4 poses are the same pose
    assert mapfile.pose_records(pc.singles().astype(RAW), rot[:3], 0.02)[0].tobytes() == mapfile.pose_records(pc.singles().astype(RAW), rot, 0.02)[0].tobytes()


def test_identity_gives_count_one_records_back():
    rec = pc.singles()
    assert len(rec) >= 290 and np.all(rec["count"] == 1)
    out, info = _same(rec, I4, 0.02)
    assert out.tobytes() == rec.astype(RAW).tobytes()
    assert info == dict(voxels_in=len(rec), voxels_moved=len(rec), voxels_dropped=0, voxels_skipped=0, points_moved=len(rec),
                        points_dropped=0, points_skipped=0)


def test_whole_voxel_translation_shifts_keys_and_sums():
    rec = pc.counted()
    assert rec["count"].max() > 1
    T = pc.translation(np.array(pc.SHIFT) * pc.V6)
    out, info = _same(rec, T, pc.V6)
    assert out.tobytes() == pc.shifted(rec).astype(RAW).tobytes()
    moved = out["sum_q"].sum(0) - rec["sum_q"].sum(0)
    assert moved.tolist() == [int(rec["count"].sum()) * k * (1 << 14) for k in pc.SHIFT]  # exactly k * 2^14 per point
    back, _ = _same(out, pc.translation(-np.array(pc.SHIFT) * pc.V6), pc.V6)
    assert back.tobytes() == rec.astype(RAW).tobytes()


def test_counts_and_colours_are_conserved_and_drops_counted():
    rec, T, vd = pc.edge_cases()
    posed, info, status = mp.posed(rec, T, vd)
    assert status.tolist() == [mp.MOVED, mp.DROPPED, mp.DROPPED]  # ascending keys: 1 m, 1023.5 m (key range), 2047 m (2048 m)
    out, ginfo = _same(rec, T, vd)
    assert ginfo == dict(voxels_in=3, voxels_moved=1, voxels_dropped=2, voxels_skipped=0, points_moved=3, points_dropped=12, points_skipped=0)
    assert out["count"].tolist() == [3] and out["sum_bgr"].tolist() == rec["sum_bgr"][:1].tolist()
    # a larger set under a pose that drops some and a min_count that skips some: every point and colour sum is accounted for
    rng = np.random.default_rng(5)
    big = pc.records_at(rng.integers(-(1 << 23), 1 << 23, (400, 3)) * 256, rng.integers(1, 4, 400), 0.02, 21)  # up to 2048 m
    Tb = pc.translation([700.0, -650.0, 10.0])
    posed, info, status = mp.posed(big, Tb, 0.02, 2)
    out, ginfo = _same(big, Tb, 0.02, 2)
    assert min(info["voxels_moved"], info["voxels_dropped"], info["voxels_skipped"]) > 20
    assert info["voxels_in"] == len(big) == info["voxels_moved"] + info["voxels_dropped"] + info["voxels_skipped"]
    assert info["points_moved"] + info["points_dropped"] + info["points_skipped"] == int(big["count"].sum())
    for st, key in ((mp.MOVED, "points_moved"), (mp.DROPPED, "points_dropped"), (mp.SKIPPED, "points_skipped")):
        assert int(big["count"][status == st].sum()) == info[key]
    assert out["sum_bgr"].sum(0).tolist() == big["sum_bgr"][status == mp.MOVED].sum(0).tolist()
    assert int(out["count"].sum()) == info["points_moved"]
    assert np.all(big["count"][status == mp.SKIPPED] == 1) and np.all(big["count"][status != mp.SKIPPED] >= 2)


def test_the_last_index_is_kept():
    rec, T = pc.last_index()
    out, info = _same(rec, T, 2.0 ** -9)
    assert info["voxels_moved"] == 1 and (int(out["key"][0]) >> 42) == (1 << 21) - 1
    assert _same(rec, pc.translation([2.0 ** -8, 0, 0]), 2.0 ** -9)[1]["voxels_dropped"] == 1  # one voxel further: out of key range


def test_refusals():
    rec = pc.singles().astype(RAW)
    big = rec.copy()
    big["count"][3] = 1 << 32
    skew, nan = I4.copy(), I4.copy()
    skew[0, 1] = 0.01
    nan[1, 3] = np.nan
    mirror = np.diag(F([1, 1, -1, 1]))
    for bad_rec, T, v in ((big, I4, 0.02), (rec, skew, 0.02), (rec, nan, 0.02), (rec, mirror, 0.02), (rec, I4, 0.0), (rec, I4, float("inf")),
                          (rec, I4, float("nan")), (rec, I4, -0.02)):
        with pytest.raises(ValueError):
            mapfile.pose_records(bad_rec, T, v)
        with pytest.raises(ValueError):
            mp.pose_raw(bad_rec, T, v)
    big["count"][3] = (1 << 32) - 1
    big["sum_q"][3] *= (1 << 32) - 1
    _same(big, I4, 0.02)  # the largest count there is: count * q stays inside int64


def test_merge_then_subtract_gives_the_destination_back():
    dst = _edge_scene(0.02).astype(RAW)
    posed, info = mapfile.pose_records(dst, D_SMALL.astype(F), 0.02)
    both = mapfile.merge_records(dst, posed)
    assert len(dst) < len(both) < len(dst) + len(posed)  # some voxels are shared, some are new
    assert mapfile.subtract_records(both, posed).tobytes() == dst.tobytes()
    got, _ = mp.merge_posed(dst, dst, D_SMALL.astype(F), 0.02)
    assert got.tobytes() == both.tobytes()
    assert mp.subtract_posed(both, dst, D_SMALL.astype(F), 0.02)[0].tobytes() == dst.tobytes()
    with pytest.raises(ValueError):
        mp.subtract_posed(dst, dst, D_SMALL.astype(F), 0.02)  # never put there


def test_transform_cli_round_trip(tmp_path, capsys):
    a_rec, b_rec = pc.counted().astype(RAW), pc.shifted(pc.counted(seed=31), (1, 0, -1)).astype(RAW)
    a, b, x, m, back, pose12, pose16 = (str(tmp_path / n) for n in ("a.rvm", "b.rvm", "x.rvm", "m.rvm", "back.rvm", "p12.txt", "p16.txt"))
    mapfile.write(a, mapfile.make_header(pc.V6, 0, a_rec, 7, 2), a_rec)
    mapfile.write(b, mapfile.make_header(2 * pc.V6, 1, b_rec, 1, 3), b_rec)
    T = synth.se3_exp(np.array([0.3, -0.2, 0.1, 0.4, -0.3, 0.2])).astype(F)
    np.savetxt(pose12, T[:3].astype(np.float64), fmt="%.9g")
    np.savetxt(pose16, T.astype(np.float64), fmt="%.9g")
    assert mapfile.read_pose(pose12).tobytes() == T.tobytes() == mapfile.read_pose(pose16).tobytes()
    assert mapfile.main(["transform", a, pose12, "-o", x, "--voxel", str(2 * pc.V6), "--min-count", "2"]) == 0
    h, rec = mapfile.read(x)
    want, info = mp.pose_raw(a_rec, T, 2 * pc.V6, 2)
    assert rec.tobytes() == want.tobytes() and info["voxels_skipped"] > 0
    assert (h["voxel"], h["dense"], h["points_dropped"], h["keyframes"]) == (2 * pc.V6, 0, 7 + info["points_dropped"], 2)
    assert mapfile.main(["merge", m, b, x]) == 0
    assert mapfile.main(["subtract", m, x, "-o", back]) == 0
    assert open(back, "rb").read() == open(b, "rb").read()
    # the defaults: the file's own edge, min_count 1; a 4x4 pose file
    assert mapfile.main(["transform", a, pose16, "-o", x]) == 0
    assert mapfile.read(x)[1].tobytes() == mp.pose_raw(a_rec, T, pc.V6)[0].tobytes() and mapfile.read(x)[0]["voxel"] == pc.V6
    with open(pose12, "w") as f:
        f.write("1 0 0 0 0 1 0 0 0 0 2 0")
    assert mapfile.main(["transform", a, pose12, "-o", x]) == 1  # not a rotation
    assert mapfile.main(["transform", a, "-o", x]) == 2
    capsys.readouterr()


def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "pose_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "pose_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def test_host_canonicalisation(tmp_path):
    """revo_pose_host.h over unsorted records with repeated keys (sums that wrap included) and over poses: the bytes
    mapfile.merge_records gives, and the pose rules of the reference."""
    exe = _host(tmp_path)
    rng = np.random.default_rng(3)
    keys = rng.integers(1, 1 << 62, 200).astype(np.uint64)
    rec = np.zeros(1000, RAW)
    rec["key"] = keys[rng.integers(0, 200, 1000)]
    rec["count"] = rng.integers(1, 1 << 20, 1000)
    rec["sum_q"] = rng.integers(-(1 << 61), 1 << 61, (1000, 3))
    rec["sum_bgr"] = rng.integers(0, 1 << 40, (1000, 3))
    skew, nan = I4.copy(), I4.copy()
    skew[0, 1] = 0.01
    nan[1, 3] = np.nan
    almost = I4.copy()
    almost[0, 1] = 5e-6  # |R R^T - I|_F = 7.07e-6: inside the rule
    poses = [I4, D_SMALL.astype(F), skew, nan, np.diag(F([1, 1, -1, 1])), almost]
    for r in (rec, rec[:1], rec[:0]):
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<I", len(poses)) + b"".join(np.ascontiguousarray(T.T).tobytes() for T in poses))
            f.write(struct.pack("<Q", len(r)) + r.tobytes())
        subprocess.run([exe, inp, out], check=True, timeout=120)
        raw = open(out, "rb").read()
        flags = list(raw[:len(poses)])
        want_flags = []
        for T in poses:
            try:
                mp.check_pose(T, 0.02)
                want_flags.append(3)
            except ValueError:
                want_flags.append(1 if np.all(np.isfinite(T)) else 0)
        assert flags == want_flags == [3, 3, 1, 0, 1, 3]
        m = struct.unpack_from("<Q", raw, len(poses))[0]
        want = mapfile.merge_records(r, np.zeros(0, RAW)) if len(r) else r
        assert m == len(want) and raw[len(poses) + 8:] == want.tobytes()
        assert [mapfile.pose_is_orthogonal(T[:3, :3]) for T in poses if np.all(np.isfinite(T))] == [True, True, False, False, True]
