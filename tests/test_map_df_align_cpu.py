"""Registration against the distance field without a GPU: the exports and the record's layout, revo_amd.mapfile's
restatement against the numpy specification tests/map_df_align_ref.py bit for bit, analytic checks of the interpolant on a field
with one solid voxel, the host-only revo_map_df_align_system against a direct evaluation of the cost's derivatives, the
`mapfile df-align` command, a loaded DistanceField, and the host arithmetic of revo_map_df_align (tests/cpp/df_align_host.cpp)
replayed over the records of the specification's loop."""
import ctypes as C
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, api, mapfile, synth
from revo_amd.settings import MapDfAlignInfo

import map_df_align_cases as dc
import map_df_align_ref as dfr
import map_plane_ref as mpr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I4 = np.eye(4, dtype=F)
V = dc.V


def test_declared_exported_and_laid_out(tmp_path):
    for name in ("revo_map_df_align_eval", "revo_map_df_align_system", "revo_map_df_align"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "revo_hip.h"\n'
                   '#define F(m) printf(#m " %zu\\n", offsetof(revo_map_df_align_info, m));\n'
                   'int main(void) {\n  printf("info %zu\\n", sizeof(revo_map_df_align_info));\n'
                   '  F(S) F(matched) F(considered) F(skipped) F(centre) F(max_dist) F(R) F(T) F(flags) F(reserved)\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines())
    assert int(got["info"]) == 208 == C.sizeof(MapDfAlignInfo) == C.sizeof(dfr.DfAlignInfo) == mapfile.DF_ALIGN_DTYPE.itemsize
    for name, _ in dfr.DfAlignInfo._fields_:
        assert int(got[name]) == getattr(MapDfAlignInfo, name).offset == getattr(dfr.DfAlignInfo, name).offset == mapfile.DF_ALIGN_DTYPE.fields[name][1], name


def _same(d2, lo, n, voxel, pts, poses, max_dist, centre, what):
    got = mapfile.df_align_records(d2, lo, n, voxel, pts, poses, max_dist, centre)
    want = [dfr.df_align_eval(d2, lo, voxel, pts, T, max_dist, centre) for T in poses]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == bytes(w), (what, i)
    return want


def test_mapfile_follows_the_specification():
    d2, lo, n = dc.base()
    pts = np.concatenate([dc.random_points(lo, n, 2000, 1), dc.cell_points(lo, dc.rim_cells(n)), dc.ODD_POINTS])
    poses = dc.poses(3, 2) + list(dc.bad_poses())
    w = _same(d2, lo, n, V, pts, poses, 0.08, (0.1, -0.05, 0.2), "base")
    assert [x.flags for x in w] == [0, 0, 0, 1, 1, 1] and all(0 < x.matched < x.considered - x.skipped for x in w[:3])
    assert all(x.matched == x.skipped == x.considered == 0 and not any(x.S) for x in w[3:])
    # another edge (cell boundaries are not exact), a clamped field, a field without a solid, an axis of one cell
    _same(d2, lo, n, 0.02, dc.random_points(lo, n, 700, 3, 0.02), poses[:2], 0.05, (0, 0, 0), "0.02 m")
    w = _same(np.minimum(d2, 3), lo, n, V, pts, poses[:2], 1.0, (0, 0, 0), "clamped")
    assert w[0].matched == w[0].considered - w[0].skipped  # nothing is gated: the clamp caps every residual at sqrt(3) cells
    w = _same(dc.field_of(n, []), lo, n, V, pts, poses[:1], 1.0, (0, 0, 0), "all NONE")
    assert (w[0].matched, w[0].skipped) == (0, len(pts))
    for flat in ((1, 7, 11), (9, 1, 11), (9, 7, 1)):
        w = _same(dc.field_of(flat, [(0, 0, 0)]), lo, flat, V, pts, poses[:1], 1.0, (0, 0, 0), "one cell")
        assert (w[0].matched, w[0].skipped) == (0, len(pts))


def test_one_solid_voxel_analytically():
    n, lo, s = (6, 7, 8), (-3, 2, -5), (2, 3, 4)
    d2 = dc.field_of(n, [s])
    root = np.sqrt(d2.astype(np.float64))
    # a point at a cell centre: w = 0 and c is that cell's value; at the solid cell: e = 0 and zero sums
    cells = np.array([(0, 0, 0), (1, 2, 3), (4, 5, 6), (2, 3, 4), (3, 3, 4)], np.float64)
    r = dfr.interpolate(d2, lo, V, dc.cell_points(lo, cells), I4)
    assert r["ok"].all() and not r["none"].any() and not r["w"].any()
    assert r["c"].tolist() == [float(F(root[tuple(int(x) for x in c)])) for c in cells] and r["c"][3] == 0 and r["c"][4] == 1
    at = dfr.df_align_eval(d2, lo, V, np.repeat(dc.cell_points(lo, [s]), 5, 0), I4, 1.0)
    # every sum that carries the residual (J e, e e) is exactly +0; the one-sided gradient there is (1, 1, 1), so S[0] = 5
    assert (at.matched, at.skipped) == (5, 0) and np.array(list(at.S[21:]), F).tobytes() == np.zeros(7, F).tobytes() and at.S[0] == 5
    # inside one cell the interpolant is trilinear: its reported gradient is its derivative, by central differences in double
    base, h = np.array([3.3, 4.6, 1.2]), 2.0 ** -6
    at = dfr.interpolate(d2, lo, V, dc.cell_points(lo, [base]), I4)
    for i in range(3):
        d = np.zeros(3)
        d[i] = h
        pm = dfr.interpolate(d2, lo, V, dc.cell_points(lo, [base + d, base - d]), I4)
        fd = (float(pm["c"][0]) - float(pm["c"][1])) / (2 * h)
        assert abs(fd - float(at["g"][0, i])) < 2e-5, (i, fd, at["g"][0])  # float32 values of a few cells over 2h = 2^-5
    assert at["e"][0] == at["c"][0] * F(V)


def test_df_system_against_the_cost_derivatives():
    """cost(x) = sum (e + g.v + w.(u x g))^2: revo_map_df_align_system's H is half its Hessian, g half its gradient at 0,
    S[27] the cost."""
    rng = np.random.default_rng(23)
    n = 12
    u = rng.uniform(-1, 1, (n, 3)).astype(F)
    gr = rng.uniform(-1, 1, (n, 3)).astype(F)
    e = rng.uniform(0, 0.1, n).astype(F)
    info = MapDfAlignInfo()
    for i, t in enumerate(dfr.terms_of(u, gr, e)):
        info.S[i] = dfr.xr.round_exact_f32(t)
    info.matched = info.considered = n
    H, g = api.df_align_system(info)
    assert np.array_equal(H, H.T)
    Hr, gs = dfr.system(dfr.DfAlignInfo.from_buffer_copy(bytes(info)))
    Hm, gm = mapfile.df_align_system(np.frombuffer(bytes(info), mapfile.DF_ALIGN_DTYPE)[0])
    assert np.array_equal(H, Hr) and np.array_equal(g, gs) and np.array_equal(H, Hm) and np.array_equal(g, gm)
    ud, gd, ed = u.astype(np.float64), gr.astype(np.float64), e.astype(np.float64)
    J = np.hstack([gd, np.cross(ud, gd)])
    Hd, gv, cost = J.T @ J, J.T @ ed, float(ed @ ed)
    eps = 2.0 ** -21  # half a float ulp per product, per rounded factor and for the sum, with room (test_map_plane_cpu's bound)
    assert np.max(np.abs(H - Hd)) <= eps * (np.abs(J)[:, :, None] * np.abs(J)[:, None, :]).sum(0).max()
    assert np.max(np.abs(g - gv)) <= eps * (np.abs(J) * np.abs(ed)[:, None]).sum(0).max()
    assert abs(float(info.S[27]) - cost) <= eps * cost

    def cost_at(x):
        ee = ed + gd @ x[:3] + np.cross(ud, gd) @ x[3:]
        return float(ee @ ee)

    h = 1e-3
    for a in range(6):
        d = np.zeros(6)
        d[a] = h
        assert abs((cost_at(d) - cost_at(-d)) / (2 * h) - 2 * g[a]) < 1e-6
        assert abs((cost_at(d) - 2 * cost_at(0 * d) + cost_at(-d)) / (h * h) - 2 * H[a, a]) < 1e-5
    info.flags = 1
    dp = C.POINTER(C.c_double)
    assert _lib.lib().revo_map_df_align_system(C.byref(info), H.ctypes.data_as(dp), g.ctypes.data_as(dp)) == -1
    assert _lib.lib().revo_map_df_align_system(None, H.ctypes.data_as(dp), g.ctypes.data_as(dp)) == -1


@functools.lru_cache(maxsize=None)
def _blob():
    return dc.blob()


TWIST = (0.03, -0.02, 0.025, 0.02, -0.015, 0.01)  # about a cell along every axis


def _blob_source(twist=TWIST):
    """The blob's own solids as a cloud, moved by D^-1: registering it recovers D."""
    d2, lo, n, solids = _blob()
    D = dc.se3(twist)
    Di = np.linalg.inv(D)
    return (dc.cell_points(lo, solids).astype(np.float64) @ Di[:3, :3].T + Di[:3, 3]).astype(F), D


def test_mapfile_loop_and_loaded_field(tmp_path):
    d2, lo, n, _ = _blob()
    p, D = _blob_source()
    c = dfr.default_centre(p, I4)
    T, rec, it, st = dfr.df_align(d2, lo, V, p, I4, F(8 * V), c)
    assert st == dfr.CONVERGED and 2 < it < 30 and rec.matched == len(p)
    assert np.linalg.norm((np.linalg.inv(D) @ T)[:3, 3]) < 1e-6  # the cloud's own cell centres: the residual vanishes at D
    Tm, rm, im, sm = mapfile.df_align(d2, lo, n, V, p, None, 8 * V)
    assert Tm.tobytes() == T.tobytes() and rm.tobytes() == bytes(rec) and (im, sm) == (it, st)
    assert mapfile.df_align_centre(p, I4).tobytes() == c.tobytes()
    # a DistanceField without a map (a loaded one) goes through mapfile: the same records and loop
    path = str(tmp_path / "f.npz")
    api.DistanceField(d2, lo, V).save(path)
    f = api.DistanceField.load(path)
    poses = dc.poses(3, 4, 0.3)
    got = f.align_eval(p, poses, 8 * V)
    assert [bytes(g) for g in got] == [bytes(dfr.df_align_eval(d2, lo, V, p, Tq, 8 * V, c)) for Tq in poses]
    assert isinstance(got[0], MapDfAlignInfo) and bytes(f.align_eval(p, poses[1], 8 * V, c)) == bytes(got[1])
    r = f.align(p)
    assert r["T"].tobytes() == T.tobytes() and bytes(r["info"]) == bytes(rec) and (r["iterations"], r["status"]) == (it, st)
    H, _ = dfr.system(rec)
    assert r["sigma2"] == float(rec.S[27]) / (rec.matched - 6) and np.allclose(r["cov"] @ H, r["sigma2"] * np.eye(6), atol=1e-9 * r["sigma2"] + 1e-15)
    with pytest.raises(ValueError):
        mapfile.df_align_records(d2, lo, n, V, p, poses, 0.0, c)
    with pytest.raises(ValueError):
        mapfile.df_align(d2, lo, n, V, p, None, 8 * V, max_iters=0)


def test_mapfile_df_align_round_trip(tmp_path, capsys):
    """`mapfile df-align DST SRC -o POSE`: two .rvm files of the same surface, the second moved, give the pose between them."""
    d2, lo, n, solids = _blob()
    p, D = _blob_source()

    def rvm(path, pts):
        rec = np.zeros(len(pts), mapfile.RAW_DTYPE)
        k = np.floor(pts.astype(np.float64) / V).astype(np.int64) + (1 << 20)
        rec["key"] = (k[:, 0].astype(np.uint64) << np.uint64(42)) | (k[:, 1].astype(np.uint64) << np.uint64(21)) | k[:, 2].astype(np.uint64)
        rec["count"], rec["sum_q"] = 1, np.rint(pts.astype(np.float64) * 2.0 ** 20).astype(np.int64)
        rec = rec[np.argsort(rec["key"])]
        assert len(np.unique(rec["key"])) == len(rec)
        mapfile.write(path, mapfile.make_header(V, 0, rec), rec)
        return rec

    a, b, out, init = (str(tmp_path / x) for x in ("a.rvm", "b.rvm", "pose.txt", "init.txt"))
    rvm(a, dc.cell_points(lo, solids))
    src = rvm(b, p)
    assert mapfile.main(["df-align", a, b, "--max-dist", "0.2", "-o", out]) == 0
    assert "converged" in capsys.readouterr().out
    T = mapfile.read_pose(out)
    E = np.linalg.inv(D) @ T.astype(np.float64)
    assert np.linalg.norm(E[:3, 3]) < 1e-5 and synth.rot_angle(np.eye(3), E[:3, :3]) < 1e-5
    # the command is the functions: the same field box, points, default centre and loop
    lo2, hi2, _ = mapfile.bounds_records(mapfile.read(a)[1])
    blo, bn = mapfile.padded_box(lo2, hi2, 9)  # ceil(0.2 / V) + 2
    f2 = mapfile.distance_field_records(mapfile.read(a)[1], blo, bn)[0]
    want = mapfile.df_align(f2, blo, bn, V, mapfile.to_points(src)[0], None, 0.2)
    assert np.array_equal(T, np.float32(["%.9g" % x for x in want[0].reshape(-1)]).reshape(4, 4))
    # from a start pose, with a pad; a start far outside the field is lost (exit status 1); usage errors
    np.savetxt(init, D.astype(F))
    assert mapfile.main(["df-align", a, b, "--init", init, "--pad", "4", "-o", out]) == 0
    far = np.eye(4)
    far[:3, 3] = (7, -9, 11)
    np.savetxt(init, far)
    assert mapfile.main(["df-align", a, b, "--init", init, "-o", out]) == 1 and "lost" in capsys.readouterr().out
    assert mapfile.main(["df-align", a, "-o", out]) == 2 and mapfile.main(["df-align", a, b]) == 2
    capsys.readouterr()


def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "df_align_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "df_align_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def test_host_loop_follows_the_specification(tmp_path):
    """revo_map_df_align's host arithmetic replayed over the records the specification's loop evaluated: the same poses asked
    for and returned bit for bit, the same iterations and status -- converged, iteration limit, and lost outside the field."""
    exe = _host(tmp_path)
    d2, lo, n, _ = _blob()
    p, _ = _blob_source()
    away = I4.copy()
    away[:3, 3] = (7, -9, 11)
    for T0, max_iters, want_status in ((I4, 30, dfr.CONVERGED), (I4, 2, dfr.ITER_LIMIT), (away, 30, dfr.LOST)):
        c = dfr.default_centre(p, T0)
        seen = []
        T, info, it, status = dfr.df_align(d2, lo, V, p, T0, F(8 * V), c, max_iters=max_iters, seen=seen)
        assert status == want_status and len(seen) == it + (2 if status == dfr.LOST else 1)
        if status == dfr.LOST:
            assert it == 0 and seen[0].matched == 0 and seen[0].skipped == len(p) and T.tobytes() == away.tobytes()
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.asarray(c, F).tobytes() + np.ascontiguousarray(T0.T).tobytes())
            f.write(struct.pack("<iddQi", max_iters, 1e-6, 1e-6, 12, len(seen)) + b"".join(bytes(x) for x in seen))
        subprocess.run([exe, inp, out], check=True, timeout=120)
        raw = open(out, "rb").read()
        Tc = np.frombuffer(raw, F, 16).reshape(4, 4).T
        itc, stc, calls = struct.unpack_from("<3i", raw, 64)
        worst = struct.unpack_from("<d", raw, 76)[0]
        H = np.frombuffer(raw, np.float64, 36, 84).reshape(6, 6)
        g = np.frombuffer(raw, np.float64, 6, 84 + 288)
        print("status %d: %d iterations, %d evaluations, poses asked for differ by at most %.3g" % (stc, itc, calls, worst))
        assert (itc, stc, calls) == (it, status, len(seen))
        assert worst == 0.0 and Tc.tobytes() == T.tobytes()  # bit for bit
        Hs, gs = mpr.system(seen[0])
        assert np.array_equal(H, Hs) and np.array_equal(g, gs)
