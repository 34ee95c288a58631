"""Point-to-plane registration of voxel maps without a GPU: the exports and the record's layout, the numpy
specification tests/map_plane_ref.py against itself on hand-made maps, the host-only revo_map_align_plane_system against a direct
evaluation of the cost's derivatives, the float32 Jacobi normals against a double eigh on the dense scene, and the host
arithmetic of revo_map_align_plane (tests/cpp/align_plane_host.cpp) replayed over the records of the specification's loop."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np

from revo_amd import _lib
from revo_amd.settings import MapNormalsParams, MapPlaneInfo

import map_align_ref as mar
import map_plane_cases as mc
import map_plane_ref as mpr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I4 = np.eye(4, dtype=F)
# Float32 Jacobi normals against numpy.linalg.eigh in double on the dense 320x240 scene (seeds 902 / 903, 0.02 m; 64 682 voxels,
# 54 899 valid under both): the largest angle measured is 2.39e-7 rad, and no voxel is valid under one and not the other
# (DESIGN 17).  The bounds are twice the measured figures.
JACOBI_MAX_ANGLE, JACOBI_MAX_SHARE = 2 * 2.39e-7, 2 * 0.0


def test_declared_exported_and_laid_out(tmp_path):
    for name in ("revo_map_normals", "revo_map_align_plane_eval", "revo_map_align_plane_system", "revo_map_align_plane"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "revo_hip.h"\n'
                   '#define F(m) printf(#m " %zu\\n", offsetof(revo_map_plane_info, m));\n'
                   'int main(void) {\n'
                   '  printf("info %zu\\nparams %zu\\n", sizeof(revo_map_plane_info), sizeof(revo_map_normals_params));\n'
                   '  F(S) F(matched) F(considered) F(skipped) F(centre) F(max_dist) F(R) F(T) F(flags) F(dst_normals)\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines())
    assert int(got["info"]) == 208 == C.sizeof(MapPlaneInfo) == C.sizeof(mpr.PlaneInfo) and int(got["params"]) == 16 == C.sizeof(MapNormalsParams)
    for name, _ in mpr.PlaneInfo._fields_:
        assert int(got[name]) == getattr(MapPlaneInfo, name).offset == getattr(mpr.PlaneInfo, name).offset, name


def test_flat_patch_has_the_exact_normal():
    keys, m, nv, lam, nb, valid = mpr.normals(mc.records(mc.patch()))
    assert nb.tolist() == [4, 6, 4, 6, 9, 6, 4, 6, 4]
    assert valid.tolist() == [n >= 5 for n in nb.tolist()]  # the corners have four neighbours: below min_neighbours
    assert nv[valid].tobytes() == np.tile(F([0, 0, 1]), (5, 1)).tobytes() and not nv[~valid].any()
    assert np.all(lam[:, 0] == 0) and lam[4].tolist() == [0.0, float(F(6 * mc.S * mc.S)), float(F(6 * mc.S * mc.S))]
    # lambda and neighbours are reported for the invalid corners too
    assert lam[0, 1] > 0 and nb[0] == 4
    assert not mpr.normals(mc.records(mc.patch()), min_neighbours=10)[5].any()
    assert mpr.normals(mc.records(mc.patch()), min_neighbours=3)[5].all()


def test_tilted_patch_against_eigh():
    rec = mc.records(mc.patch(mc.TILT))
    keys, m, nv, lam, nb, valid = mpr.normals(rec)
    nd, vd = mc.normals_double(rec)
    assert valid.tolist() == vd.tolist() and valid.sum() == 5
    # the plane z = B + a x + b y: every valid voxel sees the same normal (-a, -b, 1) / |.|, made positive in z
    a, b = mc.TILT[0] / mc.S, mc.TILT[1] / mc.S
    want = np.array([-a, -b, 1.0]) / np.sqrt(a * a + b * b + 1.0)
    for got, d in zip(nv[valid].astype(np.float64), nd[valid]):
        # float32 sums of a 9-point covariance with eigenvalue gaps of the order of the eigenvalues: errors of a few float ulps
        assert np.linalg.norm(np.cross(got, d)) < 1e-5 and np.linalg.norm(got - want) < 1e-5
    assert np.all(np.abs(np.linalg.norm(nv[valid].astype(np.float64), axis=1) - 1) < 2e-7) and np.all(nv[valid][:, 2] > 0)


def test_lines_and_blocks_are_no_planes():
    keys, m, nv, lam, nb, valid = mpr.normals(mc.records(mc.line()), min_neighbours=3)
    assert nb.tolist() == [2, 3, 2] and not valid.any() and not nv.any()
    assert lam[1].tolist() == [0.0, 0.0, float(F(2 * mc.S * mc.S))]  # l1 == 0: no spread across the line (min_spread)
    keys, m, nv, lam, nb, valid = mpr.normals(mc.records(mc.block()), min_neighbours=3)
    assert nb[13] == 27 and not valid.any() and not nv.any()
    assert lam[13, 0] == lam[13, 1] == lam[13, 2] > 0  # l0 > planarity * l1 (planarity)


def test_a_map_against_itself():
    """Three orthogonal patches, every voxel with a valid normal (a voxel without one is no candidate, and its source voxel
    would match a neighbour at a distance)."""
    rec = mc.records(mc.three_patches())
    tgt = mpr.Target(rec, F(0.02), min_neighbours=3)
    assert tgt.dst_normals == len(rec) == 27
    c = mar.default_centre(rec, I4)
    info = mpr.align_plane_eval(tgt, rec, I4, F(0.02), centre=c)
    assert info.flags == 0 and info.matched == info.considered == 27 and info.skipped == 0 and info.dst_normals == 27
    assert np.array(list(info.S[21:]), F).tobytes() == np.zeros(7, F).tobytes()  # every one exactly +0
    x = mar.solve(*mpr.system(info))
    assert x is not None and not x.any()
    T, info2, it, status = mpr.align_plane(tgt, F(0.02), rec, I4, F(0.02), centre=c)
    assert status == mpr.CONVERGED and it == 1 and T.tobytes() == I4.tobytes() and bytes(info2) == bytes(info)
    # on a scene with voxels that have no normal, those match a neighbour: fewer candidates, every source voxel still considered
    sheet = mc.sheet_records(0.02, [I4, I4])
    big = mpr.Target(sheet, F(0.02))
    info = mpr.align_plane_eval(big, sheet, I4, F(0.02), centre=c)
    assert 1000 < big.dst_normals == info.dst_normals < len(sheet) and big.dst_normals <= info.matched <= info.considered == len(sheet)


def test_plane_system_against_the_cost_derivatives():
    """cost(x) = sum (e + n.v + w.(u x n))^2: revo_map_align_plane_system's H is half its Hessian, g half its gradient at 0,
    S[27] the cost."""
    rng = np.random.default_rng(17)
    n = 12
    u = rng.uniform(-1, 1, (n, 3)).astype(F)
    r = rng.uniform(-0.02, 0.02, (n, 3)).astype(F)
    nv = rng.normal(size=(n, 3))
    nv = (nv / np.linalg.norm(nv, axis=1)[:, None]).astype(F)
    info = MapPlaneInfo()
    for i, t in enumerate(mpr.plane_terms(u, r, nv)):
        info.S[i] = mpr.xr.round_exact_f32(t)
    info.matched = info.considered = n
    H, g = np.zeros(36), np.zeros(6)
    dp = C.POINTER(C.c_double)
    assert _lib.lib().revo_map_align_plane_system(C.byref(info), H.ctypes.data_as(dp), g.ctypes.data_as(dp)) == 0
    H = H.reshape(6, 6)
    assert np.array_equal(H, H.T)
    Hr, gr = mpr.system(mpr.PlaneInfo.from_buffer_copy(bytes(info)))
    assert np.array_equal(H, Hr) and np.array_equal(g, gr)
    ud, rd, nd = u.astype(np.float64), r.astype(np.float64), nv.astype(np.float64)
    J = np.hstack([nd, np.cross(ud, nd)])
    e = (nd * rd).sum(1)
    Hd, gd, cost = J.T @ J, J.T @ e, float(e @ e)
    # every S is within half a float ulp of a sum of float products of float-rounded factors: 2^-21 of the sums of magnitudes
    # bounds the roundings of e and u x n, of the products and of the sum with room
    eps = 2.0 ** -21
    assert np.max(np.abs(H - Hd)) <= eps * (np.abs(J)[:, :, None] * np.abs(J)[:, None, :]).sum(0).max()
    assert np.max(np.abs(g - gd)) <= eps * (np.abs(J) * np.abs(rd).sum(1)[:, None]).sum(0).max()
    assert abs(float(info.S[27]) - cost) <= 4 * eps * (np.abs(rd).sum(1) ** 2).sum()

    def cost_at(x):
        ee = e + nd @ x[:3] + np.cross(ud, nd) @ x[3:]
        return float(ee @ ee)

    h = 1e-3
    for a in range(6):
        d = np.zeros(6)
        d[a] = h
        assert abs((cost_at(d) - cost_at(-d)) / (2 * h) - 2 * g[a]) < 1e-6
        assert abs((cost_at(d) - 2 * cost_at(0 * d) + cost_at(-d)) / (h * h) - 2 * H[a, a]) < 1e-5
    info.flags = 1
    assert _lib.lib().revo_map_align_plane_system(C.byref(info), H.ctypes.data_as(dp), g.ctypes.data_as(dp)) == -1


def test_float_jacobi_against_double_eigh_on_the_dense_scene():
    rec = mc.dense_scene_records(0.02)
    keys, m, nv, lam, nb, valid = mpr.normals(rec)
    nd, vd = mc.normals_double(rec)
    both = valid & vd
    ang = np.arcsin(np.minimum(np.linalg.norm(np.cross(nv[both].astype(np.float64), nd[both]), axis=1), 1.0))
    share = float((valid != vd).mean())
    print("%d voxels, %d valid under both, largest angle %.3g rad, valid under one only: %d (share %.3g)"
          % (len(keys), int(both.sum()), float(ang.max()), int((valid != vd).sum()), share))
    assert len(keys) > 60000 and both.sum() > 50000
    assert float(ang.max()) <= JACOBI_MAX_ANGLE and share <= JACOBI_MAX_SHARE


def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "align_plane_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "align_plane_host.cpp"),
            "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def test_host_loop_follows_the_specification(tmp_path):
    """revo_map_align_plane's host arithmetic replayed over the records the specification's loop evaluated: the same poses asked
    for and returned bit for bit, the same iterations and status -- converged, iteration limit, and lost on a single plane."""
    exe = _host(tmp_path)
    D = mar.se3_exp([0.006, -0.004, 0.005, 0.002, -0.001, 0.0015])
    dst = mc.sheet_records(0.02, [I4, I4])
    src = mc.sheet_records(0.02, [D.astype(F), D.astype(F)])
    flat = mc.records(mc.plane_grid())
    flat_src = mc.records(mc.plane_grid(shift=(2.0 ** -9, 0.0, 2.0 ** -9)))
    for d, s, max_iters, want_status in ((dst, src, 30, mpr.CONVERGED), (dst, src, 2, mpr.ITER_LIMIT), (flat, flat_src, 30, mpr.LOST)):
        tgt = mpr.Target(d, F(0.02))
        c = mar.default_centre(s, I4)
        seen = []

        def evaluate(T):
            seen.append(mpr.align_plane_eval(tgt, s, T, F(0.02), centre=c))
            return seen[-1]

        T, info, it, status = mpr.gauss_newton(evaluate, mpr.system, I4, c, max_iters=max_iters)
        assert status == want_status and len(seen) == it + (2 if status == mpr.LOST else 1)
        if status == mpr.LOST:
            assert it == 0 and seen[0].matched >= 300 and T.tobytes() == I4.tobytes()  # matches enough, but one plane: rank-deficient
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.asarray(c, F).tobytes() + np.ascontiguousarray(I4.T).tobytes())
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
