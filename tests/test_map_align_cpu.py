"""Registration of voxel maps without a GPU: the numpy specification tests/map_align_ref.py against itself (a map
aligned to itself, coarsening against a map built at the coarse edge), the host-only revo_map_align_system against a direct
evaluation of the cost's derivatives, the record's ctypes mirror, `python -m revo_amd.mapfile coarsen`, and the host arithmetic
of revo_map_align (tests/cpp/align_host.cpp) replayed over the records of the specification's loop."""
import ctypes as C

import numpy as np

from revo_amd import _lib, mapfile
from revo_amd.settings import MapAlignInfo, MapAlignOpts, MapAlignParams

import map_align_ref as mar
import map_records_ref as mrr
import voxel_map_ref as ref

F = np.float32


def _cloud(seed, n=3000, offset=(0.0, 0.0, 0.0)):
    """A bumpy sheet with a step in it, around `offset`: points (keyframe frame) and colours."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-0.6, 0.6, n), rng.uniform(-0.5, 0.5, n)
    z = 1.5 + 0.15 * np.sin(4 * x) * np.cos(3 * y) + 0.2 * (x > 0.1) + 0.25 * y
    xyz = (np.stack([x, y, z], 1) + np.asarray(offset)).astype(F)
    return xyz, rng.integers(0, 256, (n, 3)).astype(np.uint8)


def _map(voxel, clouds, poses):
    r = ref.VoxelMapRef(voxel)
    for (xyz, rgb), T in zip(clouds, poses):
        r.integrate(xyz, rgb, T)
    return r


POSES = [np.eye(4, dtype=F), np.array([[1, 0, 0, 0.013], [0, 1, 0, -0.021], [0, 0, 1, 0.008], [0, 0, 0, 1]], F)]


def test_declared_and_exported():
    for name in ("revo_map_coarsen", "revo_map_align_eval", "revo_map_align_system", "revo_map_align"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    assert C.sizeof(MapAlignInfo) == C.sizeof(mar.Info) == 160 and C.sizeof(MapAlignInfo) % 16 == 0
    for name, _ in mar.Info._fields_:
        assert getattr(MapAlignInfo, name).offset == getattr(mar.Info, name).offset, name
    assert C.sizeof(MapAlignParams) == 24 and C.sizeof(MapAlignOpts) == 32


def test_a_map_against_itself():
    rec = mrr.records_of(_map(0.02, [_cloud(1), _cloud(2)], POSES))
    assert len(rec) > 1000
    c = mar.default_centre(rec, np.eye(4))
    info = mar.align_eval(rec, F(0.02), rec, np.eye(4, dtype=F), F(0.02), centre=c)
    assert info.flags == 0 and info.matched == info.considered == len(rec) and info.skipped == 0
    assert np.array(list(info.S[9:]), F).tobytes() == np.zeros(7, F).tobytes()  # every one exactly +0
    x = mar.solve(*mar.system(info))
    assert x is not None and not x.any()
    T, info2, it, status = mar.align(rec, F(0.02), rec, np.eye(4, dtype=F), F(0.02), centre=c)
    assert status == mar.CONVERGED and it == 1 and T.tobytes() == np.eye(4, dtype=F).tobytes()
    assert bytes(info2) == bytes(info)
    # min_count selects on both sides
    info3 = mar.align_eval(rec, F(0.02), rec, np.eye(4, dtype=F), F(0.02), 2, 2, centre=c)
    assert 0 < info3.matched == int((rec["count"] >= 2).sum()) < len(rec)


def test_coarsening_equals_building_at_the_coarse_edge():
    clouds = [_cloud(3), _cloud(4)]
    fine = mrr.records_of(_map(0.01, clouds, POSES))
    for shift in (1, 3):
        coarse_edge = F(np.ldexp(F(0.01), shift))
        want = mrr.records_of(_map(coarse_edge, clouds, POSES))
        got = mar.coarsen(fine, shift)
        assert len(got) == len(want) < len(fine) and got.tobytes() == want.tobytes(), shift
        assert mapfile.coarsen_records(fine, shift).tobytes() == want.tobytes(), shift


def test_coarsening_negative_indices():
    """Points at small negative coordinates: index -1 must stay -1 (floor), where a division towards zero gives 0."""
    clouds = [_cloud(5, 2000, offset=(-0.6, -0.5, -1.8))]
    fine_map = _map(0.01, clouds, POSES[:1])
    fine = mrr.records_of(fine_map)
    k = mar.unpack_keys(fine["key"])
    assert (k < 0).any() and (k == -1).any() and (k >= 0).any()
    for shift in (1, 3):
        want = mrr.records_of(_map(F(np.ldexp(F(0.01), shift)), clouds, POSES[:1]))
        got = mar.coarsen(fine, shift)
        assert got.tobytes() == want.tobytes(), shift
        kc = mar.unpack_keys(got["key"])
        assert (kc == -1).any()  # an index in [-2^shift, -1] lands on -1
        towards_zero = ref.pack_keys(np.sign(k) * (np.abs(k) >> shift))
        assert not np.array_equal(np.unique(towards_zero), got["key"])


def test_align_system_against_the_cost_derivatives():
    """cost(x) = sum |r + v + w x u|^2: revo_map_align_system's H is half its Hessian, g half its gradient at 0, S[15] the cost."""
    rng = np.random.default_rng(7)
    n = 12
    u = rng.uniform(-1, 1, (n, 3)).astype(F)
    r = rng.uniform(-0.02, 0.02, (n, 3)).astype(F)
    ux, uy, uz = u.T
    rx, ry, rz = r.T
    terms = [ux, uy, uz, ux * ux, ux * uy, ux * uz, uy * uy, uy * uz, uz * uz, rx, ry, rz,
             np.concatenate([uy * rz, -(uz * ry)]), np.concatenate([uz * rx, -(ux * rz)]), np.concatenate([ux * ry, -(uy * rx)]),
             np.concatenate([rx * rx, ry * ry, rz * rz])]
    info = MapAlignInfo()
    for i, t in enumerate(terms):
        info.S[i] = mar.xr.round_exact_f32(t)
    info.matched = info.considered = n
    H, g = np.zeros(36), np.zeros(6)
    dp = C.POINTER(C.c_double)
    assert _lib.lib().revo_map_align_system(C.byref(info), H.ctypes.data_as(dp), g.ctypes.data_as(dp)) == 0
    H = H.reshape(6, 6)
    assert np.array_equal(H, H.T)
    Hr, gr = mar.system(mar.Info.from_buffer_copy(bytes(info)))
    assert np.array_equal(H, Hr) and np.array_equal(g, gr)
    # the direct evaluation in double: J_i = [I, -hat(u_i)]
    Hd, gd, cost = np.zeros((6, 6)), np.zeros(6), 0.0
    for ui, ri in zip(u.astype(np.float64), r.astype(np.float64)):
        J = np.hstack([np.eye(3), -np.array([[0, -ui[2], ui[1]], [ui[2], 0, -ui[0]], [-ui[1], ui[0], 0]])])
        Hd += J.T @ J
        gd += J.T @ ri
        cost += ri @ ri
    # every S is within half a float ulp of the sum of float terms that are themselves rounded products: 2^-22 of the
    # sums of magnitudes bounds both roundings with room
    eps = 2.0 ** -22
    assert np.max(np.abs(H - Hd)) <= eps * (n + np.abs(u).sum() + (u.astype(np.float64) ** 2).sum())
    assert np.max(np.abs(g - gd)) <= eps * (np.abs(r).sum() + (np.abs(u).sum(1) * np.abs(r).sum(1)).sum())
    assert abs(float(info.S[15]) - cost) <= eps * cost
    # and numerically: the gradient of the cost at 0 is 2 g, by central differences (exact for a quadratic up to rounding)
    def cost_at(x):
        e = r.astype(np.float64) + x[:3] + np.cross(x[3:], u.astype(np.float64))
        return float((e * e).sum())
    h = 1e-3
    for a in range(6):
        e = np.zeros(6)
        e[a] = h
        assert abs((cost_at(e) - cost_at(-e)) / (2 * h) - 2 * g[a]) < 1e-6
        assert abs((cost_at(e) - 2 * cost_at(0 * e) + cost_at(-e)) / (h * h) - 2 * H[a, a]) < 1e-5
    info.flags = 1
    assert _lib.lib().revo_map_align_system(C.byref(info), H.ctypes.data_as(dp), g.ctypes.data_as(dp)) == -1


def test_mapfile_coarsen_round_trip(tmp_path, capsys):
    m = _map(0.01, [_cloud(8), _cloud(9)], POSES)
    rec = mrr.records_of(m).astype(mapfile.RAW_DTYPE)
    a, b, c, d = (str(tmp_path / n) for n in ("a.rvm", "b.rvm", "c.rvm", "d.rvm"))
    mapfile.write(a, mapfile.make_header(0.01, 0, rec, 3, 2), rec)
    assert mapfile.main(["coarsen", a, "1", "-o", b]) == 0
    h, got = mapfile.read(b)
    assert got.tobytes() == mar.coarsen(rec, 1).tobytes()
    assert np.float32(h["voxel"]).tobytes() == F(np.ldexp(F(0.01), 1)).tobytes()
    assert (h["points_dropped"], h["keyframes"], h["dense"]) == (3, 2, 0) and h["points_integrated"] == int(rec["count"].sum())
    # the file is the one a map built at the coarse edge saves
    want = mrr.records_of(_map(F(np.ldexp(F(0.01), 1)), [_cloud(8), _cloud(9)], POSES))
    assert open(b, "rb").read() == mrr.file_bytes(F(np.ldexp(F(0.01), 1)), 0, want, 3, 2)
    # coarsening by 1 twice is coarsening by 2; -o may come first
    assert mapfile.main(["coarsen", "-o", c, b, "1"]) == 0 and mapfile.main(["coarsen", a, "2", "-o", d]) == 0
    assert open(c, "rb").read() == open(d, "rb").read()
    assert mapfile.main(["coarsen", a, "0", "-o", d]) == 1 and mapfile.main(["coarsen", a, "21", "-o", d]) == 1
    assert mapfile.main(["coarsen", a, "1"]) == 2
    capsys.readouterr()


def _align_host(tmp_path):
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "align_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(root, "tests", "cpp", "align_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def test_host_loop_follows_the_specification(tmp_path, monkeypatch):
    """revo_map_align's host arithmetic (revo_align_host.h: system, Cholesky solve, SE(3) exponential, update, stopping rule)
    replayed over the records the specification's loop evaluated: it must ask for the same poses, in the same number of
    evaluations, and end with the same pose, iterations and status -- converged, iteration limit and lost."""
    import struct
    import subprocess
    exe = _align_host(tmp_path)
    dst = mrr.records_of(_map(0.02, [_cloud(1), _cloud(2)], POSES))
    D = mar.se3_exp([0.006, -0.004, 0.005, 0.002, -0.001, 0.0015])
    src = mrr.records_of(_map(0.02, [_cloud(1), _cloud(2)], [(D @ T.astype(np.float64)).astype(F) for T in POSES]))
    c = mar.default_centre(src, np.eye(4))
    away = np.eye(4, dtype=F)
    away[:3, 3] = (7, -9, 11)
    for T0, max_iters, want_status in ((np.eye(4, dtype=F), 30, mar.CONVERGED), (np.eye(4, dtype=F), 2, mar.ITER_LIMIT), (away, 30, mar.LOST)):
        seen = []
        real = mar.align_eval
        monkeypatch.setattr(mar, "align_eval", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
        T, info, it, status = mar.align(dst, F(0.02), src, T0, F(0.02), centre=c, max_iters=max_iters)
        monkeypatch.setattr(mar, "align_eval", real)
        assert status == want_status and len(seen) == it + (2 if status == mar.LOST else 1)
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.asarray(c, F).tobytes() + np.ascontiguousarray(T0.T).tobytes())
            f.write(struct.pack("<iddQi", max_iters, 1e-6, 1e-6, 12, len(seen)) + b"".join(bytes(s) for s in seen))
        subprocess.run([exe, inp, out], check=True, timeout=120)
        raw = open(out, "rb").read()
        Tc = np.frombuffer(raw, F, 16).reshape(4, 4).T
        itc, stc, calls = struct.unpack_from("<3i", raw, 64)
        worst = struct.unpack_from("<d", raw, 76)[0]
        H = np.frombuffer(raw, np.float64, 36, 84).reshape(6, 6)
        g = np.frombuffer(raw, np.float64, 6, 84 + 288)
        print("status %d: %d iterations, %d evaluations, poses asked for differ by at most %.3g, T_out by %.3g"
              % (stc, itc, calls, worst, np.max(np.abs(Tc - T))))
        assert (itc, stc, calls) == (it, status, len(seen))
        # double arithmetic in another order (numpy's products) may move a float pose by an ulp of its entries (|T| < 4)
        assert worst <= 2.0 ** -21 and np.max(np.abs(Tc - T)) <= 2.0 ** -21
        if not (seen[0].flags & 1):
            Hs, gs = mar.system(seen[0])
            assert np.array_equal(H, Hs) and np.array_equal(g, gs)
