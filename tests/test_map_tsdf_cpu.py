"""The TSDF volume and its mesh without a GPU: the exports and the records' layout; revo_amd.mapfile's vectorised
tsdf_records and mesh_records against the per-view, per-cell and per-cube specification tests/map_tsdf_ref.py on every shared
case; the named cells have the quantum their case was built for; the identity with observe_records; the stated exact properties;
every refused argument; the closed mesh of a sphere; the wall; api.TsdfVolume, the npz and PLY round trips; the tsdf / mesh
commands on the golden map; and tests/cpp/tsdf_host.cpp, the header host and device code share."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, api, mapfile, ply
from revo_amd.settings import MapMeshInfo, MapTsdfCell, MapTsdfInfo, MapTsdfParams

import map_carve_ref as mc
import map_seen_cases as sc
import map_tsdf_cases as tc
import map_tsdf_ref as tr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "small_map.rvm")


def test_declared_exported_and_laid_out(tmp_path):
    for name in ("revo_map_tsdf_fuse", "revo_map_tsdf_mesh"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    recs = {"revo_map_tsdf_cell": (MapTsdfCell, 8), "revo_map_tsdf_params": (MapTsdfParams, 16), "revo_map_tsdf_info": (MapTsdfInfo, 64),
            "revo_map_mesh_info": (MapMeshInfo, 64)}
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
    assert mapfile.TSDF_INFO_KEYS == tr.INFO_KEYS and mapfile.MESH_INFO_KEYS == tr.MESH_KEYS
    assert mapfile.TSDF_CELL_DTYPE == tr.CELL and mapfile.TSDF_CELL_DTYPE.itemsize == 8 and mapfile.TSDF_W_MAX == tr.W_MAX
    assert [f for f, _ in MapTsdfInfo._fields_][:5] == list(tr.INFO_KEYS) and [f for f, _ in MapMeshInfo._fields_][:7] == list(tr.MESH_KEYS)


# ---------------------------------------------------------------------------------------------------------------- fusion --
@pytest.mark.parametrize("name", list(tc.fuse_cases()))
def test_tsdf_records_follow_the_specification(name):
    c = tc.fuse_cases()[name]
    want = tc.fuse_spec(name)
    got = mapfile.tsdf_records(tc.V, c["lo"], c["n"], c["views"], c["trunc"])
    print(name, want[1], want[2][0])
    assert got[0].dtype == tr.CELL and got[0].shape == tuple(c["n"]) and got[0].tobytes() == want[0].tobytes()
    assert got[1] == want[1] and got[2] == want[2]
    assert all(sum(v.values()) == want[1]["cells"] for v in want[2]) and want[1]["saturated"] == 0
    assert want[1]["updates"] == int(want[0]["weight"].sum()) and int(np.abs(want[0]["sum"]).max()) <= 1024 * len(c["views"])
    # in pieces: the chunks of the vectorised form cannot show
    assert mapfile.tsdf_records(tc.V, c["lo"], c["n"], c["views"], c["trunc"], chunk=50)[0].tobytes() == want[0].tobytes()


def test_named_cells_have_their_quantum():
    cells, info, counts, cls = tc.fuse_spec("plane alone")
    n = tc.N

    def at(cell):
        return cells[cell], mc.CLASSES[cls[(cell[0] * n[1] + cell[1]) * n[2] + cell[2], 0]]

    for name, q in tc.QUANTA.items():
        (s, w), c = at(tc.plane_cell(name))
        assert (int(s), int(w)) == ((q, 1) if q is not None else (0, 0)), (name, s, w, c)
        assert (c in ("free", "confirmed")) == (q is not None), name
    for name, (_, _, want_cls, q) in tc.EXTRA.items():
        (s, w), c = at(tc.plane_cell(name))
        assert c == want_cls and int(w) == 1 and (q is None or int(s) == q), (name, s, c)
    # one float32 step inside either boundary still rounds to the full quantum: |q| <= 1024 without a clamp
    assert int(at(tc.plane_cell("inside_front_boundary"))[0][0]) == 1024 and int(at(tc.plane_cell("inside_back_boundary"))[0][0]) == -1024
    assert counts[0]["outside"] == 0 and info["cells_inside"] >= 3
    cells, info, counts, _ = tc.fuse_spec("behind")
    assert not cells["weight"].any() and not cells["sum"].any() and counts[0]["outside"] == info["cells"] and info["updates"] == 0
    cells, info, _, cls = tc.fuse_spec("64 views")
    assert cls.shape[1] == 64 and int(cells["weight"].max()) > 32 and info["updates"] == int(((cls == mc.FREE) | (cls == mc.CONFIRMED)).sum())
    assert tc.fuse_spec("1x1x1 trunc M")[0].shape == (1, 1, 1)
    # the host's quantum: rint is to even
    assert int(np.rint(F(0.5))) == 0 and int(np.rint(F(1.5))) == 2


def test_the_identity_with_observe():
    for name in ("9x7x5 trunc M", "9x7x5 default trunc", "64 views", "3x5x7 trunc M", "borders"):
        c = tc.fuse_cases()[name]
        cells, info, counts = mapfile.tsdf_records(tc.V, c["lo"], c["n"], c["views"], c["trunc"])
        trunc = mapfile.tsdf_trunc(tc.V, c["trunc"])
        seen, sinfo, scounts = mapfile.observe_records(tc.V, c["lo"], c["n"], c["views"], radius=0, margin=trunc, margin_rel=0.0)
        assert np.array_equal(cells["weight"] > 0, seen != 0), name
        assert counts == scounts and info["cells_weighted"] == sinfo["newly_known"]
        votes = (seen & 0x7F).astype(np.int64)
        assert np.all(cells["weight"] >= votes) and np.all(cells["weight"][seen < 0x80] == votes[seen < 0x80])


def test_the_exact_properties():
    c = tc.fuse_cases()["9x7x5 default trunc"]
    lo, n, views = c["lo"], c["n"], c["views"]
    whole = mapfile.tsdf_records(tc.V, lo, n, views)
    assert whole[0].tobytes() == tc.fuse_spec("9x7x5 default trunc")[0].tobytes()
    # the order of the views cannot show
    for order in (views[::-1], views[3:] + views[:3]):
        back = mapfile.tsdf_records(tc.V, lo, n, order)
        assert back[0].tobytes() == whole[0].tobytes() and back[1] == whole[1]
    assert mapfile.tsdf_records(tc.V, lo, n, views[::-1])[2] == whole[2][::-1]
    # A, then B accumulating, is A and B together; the specification's loop says the same
    a = mapfile.tsdf_records(tc.V, lo, n, views[:3])
    ab = mapfile.tsdf_records(tc.V, lo, n, views[3:], tsdf=a[0])
    assert ab[0].tobytes() == whole[0].tobytes() and a[1]["updates"] + ab[1]["updates"] == whole[1]["updates"]
    assert ab[1]["cells_weighted"] == whole[1]["cells_weighted"] and ab[1]["cells_inside"] == whole[1]["cells_inside"]
    assert tr.fuse(tc.V, lo, n, views[3:], tsdf=a[0])[0].tobytes() == whole[0].tobytes()
    assert a[0].tobytes() == mapfile.tsdf_records(tc.V, lo, n, views[:3])[0].tobytes()  # the volume accumulated into is not changed
    # saturation: one update under a full weight, two views
    two = [views[0], views[1]]
    near = tc.nearly_full(n)
    got = mapfile.tsdf_records(tc.V, lo, n, two, tsdf=near)
    want = tr.fuse(tc.V, lo, n, two, tsdf=near)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[1]["saturated"] > 0
    assert int(got[0]["weight"].max()) == tr.W_MAX and got[1]["updates"] + got[1]["saturated"] == sum(v["free"] + v["confirmed"] for v in got[2])
    full = near.copy()
    full["weight"] = tr.W_MAX
    again = mapfile.tsdf_records(tc.V, lo, n, two, tsdf=full)
    assert again[0].tobytes() == full.tobytes() and again[1]["updates"] == 0 and again[1]["saturated"] > 0
    # |sum| <= 2^30 whatever comes: a cell takes 2^20 updates of at most 1024
    assert tr.W_MAX * 1024 == 1 << 30
    # refused arguments
    for bad in (dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=np.nan), dict(trunc=np.inf), dict(tsdf=near[:-1]), dict(tsdf=near["sum"])):
        with pytest.raises(ValueError):
            mapfile.tsdf_records(tc.V, lo, n, views, **bad)
    with pytest.raises(ValueError):
        mapfile.tsdf_records(tc.V, lo, n, [])
    with pytest.raises(ValueError):
        mapfile.tsdf_records(tc.V, lo, n, views * 9)
    with pytest.raises(ValueError):
        mapfile.tsdf_records(tc.V, lo, (1025, 1, 1), views)


# ------------------------------------------------------------------------------------------------------------------ mesh --
@pytest.mark.parametrize("name", list(tc.mesh_cases()))
def test_mesh_records_follow_the_specification(name):
    c = tc.mesh_cases()[name]
    wv, wt, wi = tc.mesh_spec(name)
    m = mapfile.mesh_records(c["cells"], c["lo"], tc.V, c["min_weight"])
    print(name, wi)
    assert m.vertices.dtype == np.float32 and m.triangles.dtype == np.uint32
    assert m.vertices.tobytes() == wv.tobytes() and m.triangles.tobytes() == wt.tobytes() and m.info == wi
    if name.startswith("no cube"):
        assert wi["cubes"] == 0 and len(wv) == 0 and len(wt) == 0
    if len(wt):
        assert int(wt.max()) < len(wv) and len(np.unique(wt)) == len(wv)  # every vertex is used
        assert np.all(wt[:, 0] != wt[:, 1]) and np.all(wt[:, 1] != wt[:, 2]) and np.all(wt[:, 0] != wt[:, 2])


def test_the_table_is_the_geometric_rule():
    assert tuple(tr.swap_table()) == mapfile.TSDF_SWAP and tuple(tr.tetra_corners(k) for k in range(6)) == mapfile.TSDF_TETRA
    wi = tc.mesh_spec("256 patterns")[2]
    assert wi["cubes_active"] == 256 and wi["valid"] == 2048 and wi["inside"] == 1024
    # per pattern: a tetrahedron with 1 or 3 corners inside gives one triangle, with 2 two
    want = 0
    for p in range(256):
        for k in range(6):
            ins = sum((p >> v) & 1 for v in tr.tetra_corners(k))
            want += {0: 0, 4: 0, 2: 2}.get(ins, 1)
    assert wi["triangles"] == want
    assert tc.mesh_spec("256 patterns, zero sums")[2] == wi  # sum == 0 is outside
    big = tc.mesh_cases()["256 patterns, random weights"]["cells"]
    assert int(big["weight"].max()) == 1 << 20 and int(np.abs(big["sum"].astype(np.int64)).max()) == 1 << 30
    mw = [tc.mesh_spec("min_weight %d" % k)[2] for k in (0, 1, 3)]
    assert mw[0] == mw[1] and mw[2]["valid"] < mw[1]["valid"]


def test_the_sphere_is_closed():
    v, t, info = tc.mesh_spec("sphere")
    nv, ne, nf, ok, vol6 = tc.closed_mesh_numbers(v, t)
    print(info, nv, ne, nf, vol6 / 6)
    assert ok and nv == len(v) and nv - ne + nf == 2 and vol6 > 0
    assert abs(vol6 / 6 - 4 / 3 * np.pi * (4.2 * tc.V) ** 3) < 0.1 * 4 / 3 * np.pi * (4.2 * tc.V) ** 3
    # the shared faces of 2 x 2 x 3 boxes: every inner edge of the mesh is used once in each direction
    for seed in (1, 2, 3):
        v, t, _ = tc.mesh_spec("shared face %d" % seed)
        used = {}
        for a, b, c in t.tolist():
            for e in ((a, b), (b, c), (c, a)):
                used[e] = used.get(e, 0) + 1
        assert all(k == 1 for k in used.values()) and all(used.get((b, a), 0) <= 1 for a, b in used)


def test_the_wall():
    """A wall at depth d seen fronto-parallel.  A cell's distance is dc - z with z its centre's depth, and its stored value is
    q = K (dc - z) + e with K = 1024 / trunc and |e| <= 1/2 from the rounding to an integer.  Between the two planes of cells
    z0 < z1 = z0 + voxel around the wall, with t = d - z0, the zero of the line through (z0, q0) and (z1, q1) lies at
    z0 + voxel q0 / (q0 - q1), which is off the wall by ((voxel - t) e0 + t e1) / (K voxel + e0 - e1): the two half-quantum
    roundings move it by at most (voxel / 2) / (K voxel - 1) < trunc / 1024.  The bound is doubled for the float32 steps of the
    quantum, of a and of the position: every vertex lies within trunc / 512 of the wall."""
    w = tc.wall()
    cells, info, _ = mapfile.tsdf_records(tc.V, w["lo"], w["n"], w["views"], w["trunc"])
    assert info["cells_weighted"] == info["cells"] and 0 < info["cells_inside"] < info["cells"]
    trunc = float(mapfile.tsdf_trunc(tc.V, w["trunc"]))
    m = mapfile.mesh_records(cells, w["lo"], tc.V)
    want = tr.mesh(cells, w["lo"], tc.V)
    assert m.vertices.tobytes() == want[0].tobytes() and m.triangles.tobytes() == want[1].tobytes()
    err = np.abs(m.vertices[:, 2].astype(np.float64) - float(tc.WALL_DEPTH))
    print("wall: %d vertices, %d triangles, worst %.3g m, bound %.3g m" % (len(m.vertices), len(m.triangles), err.max(), trunc / 512))
    assert len(m.triangles) > 0 and err.max() <= trunc / 512
    # the normals point from the inside (behind the wall) to the outside (the camera): towards -z
    p = m.vertices.astype(np.float64)
    nz = np.cross(p[m.triangles[:, 1]] - p[m.triangles[:, 0]], p[m.triangles[:, 2]] - p[m.triangles[:, 0]])[:, 2]
    assert np.all(nz < 0)
    sdf = mapfile.tsdf_sdf(cells, trunc)
    z = (np.arange(w["lo"][2], w["lo"][2] + w["n"][2]) + 0.5) * tc.V
    assert np.allclose(sdf, (float(tc.WALL_DEPTH) - z)[None, None, :], atol=trunc / 1024)


def test_refused_mesh_arguments():
    vol = tc.mesh_cases()["sphere"]["cells"]
    for bad in (vol["sum"], vol[0], vol.astype([("sum", "<i8"), ("weight", "<u4")])):
        with pytest.raises(ValueError):
            mapfile.mesh_records(bad, (0, 0, 0), tc.V)
    with pytest.raises(ValueError):
        mapfile.mesh_records(vol, ((1 << 20) - 3, 0, 0), tc.V)


# ------------------------------------------------------------------------------------------------------- Python and tools --
def test_volume_npz_and_ply(tmp_path):
    c = tc.fuse_cases()["9x7x5 default trunc"]
    cells, info, counts = mapfile.tsdf_records(tc.V, c["lo"], c["n"], c["views"])
    v = api.TsdfVolume(cells, c["lo"], tc.V, None, info, counts)
    assert v.n.tolist() == list(c["n"]) and v.lo.dtype == np.int32 and v.voxel == tc.V and v.trunc == 4 * tc.V and v.info == info
    sdf = v.sdf()
    assert sdf.shape == cells.shape and np.array_equal(np.isnan(sdf), cells["weight"] == 0)
    assert np.array_equal(sdf[cells["weight"] > 0], tr.sdf(cells, 4 * tc.V)[cells["weight"] > 0]) and np.nanmax(np.abs(sdf)) <= v.trunc
    path = v.save(str(tmp_path / "tsdf.npz"))
    w = api.TsdfVolume.load(path)
    assert w.cells.tobytes() == cells.tobytes() and w.lo.tolist() == list(c["lo"]) and (w.voxel, w.trunc) == (tc.V, 4 * tc.V) and w.info is None
    m = w.mesh()  # a loaded volume has no map: mapfile's mesh
    assert m.vertices.tobytes() == mapfile.mesh_records(cells, c["lo"], tc.V).vertices.tobytes()
    with pytest.raises(ValueError):
        api.TsdfVolume(cells["sum"], c["lo"], tc.V, None)
    np.savez(str(tmp_path / "bad.npz"), sum=cells["sum"], weight=cells["weight"], lo=np.zeros(2, np.int32), n=np.asarray(cells.shape, np.int32),
             voxel=F(tc.V), trunc=F(0.5))
    with pytest.raises(ValueError):
        api.TsdfVolume.load(str(tmp_path / "bad.npz"))
    sv, st, _ = tc.mesh_spec("sphere")
    mesh = mapfile.Mesh(sv, st)
    out = mesh.save_ply(str(tmp_path / "sphere.ply"))
    rv, rt = ply.read_mesh_ply(out)
    assert rv.tobytes() == sv.tobytes() and rt.tobytes() == st.tobytes() and rt.dtype == np.uint32
    head = open(out, "rb").read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(sv)) and b"element face %d\n" % len(st) in head
    back = mapfile.Mesh.load_ply(out)
    assert back.triangles.tobytes() == st.tobytes() and back.info is None
    empty = ply.read_mesh_ply(ply.write_mesh_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), F), np.zeros((0, 3), np.uint32)))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)
    with pytest.raises(ValueError):
        ply.write_mesh_ply(str(tmp_path / "x.ply"), sv[:3], st)
    open(str(tmp_path / "cut.ply"), "wb").write(open(out, "rb").read()[:-5])
    with pytest.raises(ValueError):
        ply.read_mesh_ply(str(tmp_path / "cut.ply"))


def test_command_line(tmp_path, capsys):
    from PIL import Image
    from revo_amd import vo
    header, rec = mapfile.read(GOLDEN)
    folder, out, mesh_out = (str(tmp_path / x) for x in ("views", "tsdf.npz", "mesh.ply"))
    os.makedirs(os.path.join(folder, "depth"))
    os.makedirs(os.path.join(folder, "rgb"))
    T2 = np.eye(4, dtype=F)
    T2[0, 3] = -0.25
    k = (16.0, 16.0, 31.5, 23.5, 0.1, 5.2)
    lo, hi, _ = mapfile.bounds_records(rec)
    depth = float((hi[2] + lo[2]) / 2 * header["voxel"])  # a wall through the middle of the map's bounds
    views, stamps = [], [(1.5, np.eye(4, dtype=F)), (2.5, T2)]
    with open(os.path.join(folder, "poses.txt"), "w") as f:
        f.write("".join(line + "\n" for line in vo.tum_lines(stamps)))
    with open(os.path.join(folder, "associate.txt"), "w") as f:
        for i, (ts, T) in enumerate(stamps):
            D = np.full((48, 64), depth + 0.01 * i, F)
            D[:6] = 0.0
            name = "%.6f.png" % ts
            raw = np.rint(D * 5000.0).astype(np.uint16)
            Image.fromarray(raw).save(os.path.join(folder, "depth", name))
            Image.fromarray(np.zeros((48, 64, 3), np.uint8)).save(os.path.join(folder, "rgb", name))
            f.write("%.6f rgb/%s %.6f depth/%s\n" % (ts, name, ts, name))
            views.append((raw.astype(F) / F(5000.0), T, k))
    cam = ["--camera", "16", "16", "31.5", "23.5", "--zrange", "0.1", "5.2"]
    assert mapfile.main(["tsdf", GOLDEN, "--views", folder, "-o", out, "--pad", "2", "--trunc", "0.3"] + cam) == 0
    blo, n = mapfile.padded_box(lo, hi, 2)
    want = mapfile.tsdf_records(header["voxel"], blo, n, views, 0.3)[0]
    cells, tlo, voxel, trunc = mapfile.read_tsdf(out)
    assert cells.tobytes() == want.tobytes() and tlo.tolist() == blo.tolist() and voxel == header["voxel"] and trunc == float(F(0.3))
    assert int(cells["weight"].max()) == 2
    assert mapfile.main(["mesh", out, "--min-weight", "2", "-o", mesh_out]) == 0
    wm = mapfile.mesh_records(want, blo, header["voxel"], 2)
    rv, rt = ply.read_mesh_ply(mesh_out)
    assert rv.tobytes() == wm.vertices.tobytes() and rt.tobytes() == wm.triangles.tobytes()
    print(wm.info)
    assert len(rt) > 1000 and wm.info["valid"] < mapfile.mesh_records(want, blo, voxel).info["valid"]  # a wall two views see, one of them less of it
    assert mapfile.main(["mesh", out, "-o", mesh_out]) == 0 and len(ply.read_mesh_ply(mesh_out)[1]) == mapfile.mesh_records(want, blo, voxel).info["triangles"]
    # the default trunc; a missing folder, a bad trunc and a file that is no volume are refused; a missing -o is a usage error
    assert mapfile.main(["tsdf", GOLDEN, "--views", folder, "-o", out] + cam) == 0 and mapfile.read_tsdf(out)[3] == float(F(4) * F(header["voxel"]))
    assert mapfile.main(["tsdf", GOLDEN, "--views", str(tmp_path / "nothing"), "-o", out]) == 1
    assert mapfile.main(["tsdf", GOLDEN, "--views", folder, "-o", out, "--trunc", "0"] + cam) == 1
    assert mapfile.main(["mesh", GOLDEN, "-o", mesh_out]) == 1
    assert mapfile.main(["mesh", out]) == 2 and mapfile.main(["tsdf", GOLDEN, "-o", out]) == 2
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------- the shared header --
def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "tsdf_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "tsdf_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def test_host_header(tmp_path):
    """revo_tsdf_host.h: every parameter rule and the default, the quantum against the specification's float32 numbers, a vertex's
    place on its edge with 64-bit products, the update with its saturation, the 6 x 16 table against the geometric rule decided in
    the program and in the specification, the case triangles, and which cubes an edge of each type belongs to."""
    exe = _host(tmp_path)
    voxel = F(0.02)
    nan, inf = float("nan"), float("inf")
    params = [(0, (9.0, 9, 9, 9)), (1, (0.25, 0, 0, 0)), (1, (1e-3, 1, 0, 0)), (1, (0.0, 0, 0, 0)), (1, (-0.5, 0, 0, 0)), (1, (nan, 0, 0, 0)),
              (1, (inf, 0, 0, 0)), (1, (0.1, 2, 0, 0)), (1, (0.1, 0, 1, 0)), (1, (0.1, 1, 0, 7))]
    want_params = [(F(4.0) * voxel, 0), (F(0.25), 0), (F(1e-3), 1)] + [None] * 7
    rng = np.random.default_rng(26)
    quanta = []
    for trunc in (F(0.5), F(sc.M), F(0.3), F(0.07)):
        for z in rng.uniform(0.3, 4.0, 40).astype(F):
            for frac in (F(-1), F(1), F(0), F(0.5 / 1024), F(1.5 / 1024), F(2.5 / 1024)) + tuple(rng.uniform(-1, 1, 6).astype(F)):
                dc = F(z + frac * trunc)
                if abs(F(z - dc)) <= trunc:
                    quanta.append((dc, z, trunc))
    edges = [(-1, 1, 1, 1), (-1, 1, 0, 1), (1, 1, -1, 1), (0, 5, -3, 2), (-(1 << 30), 1 << 20, 1 << 30, 1 << 20), (-(1 << 30), 1 << 20, (1 << 30) - 1, 1),
             (-1, 1 << 20, 1 << 30, 1), (1 << 30, 1 << 20, -1, 1 << 20)]
    for _ in range(300):
        s0, s1 = -int(rng.integers(1, 1 << 30)), int(rng.integers(0, 1 << 30))
        e = (s0, int(rng.integers(1, (1 << 20) + 1)), s1, int(rng.integers(1, (1 << 20) + 1)))
        edges.append(e if rng.integers(2) else (e[2], e[3], e[0], e[1]))
    updates = [(0, 0, 1024), (5, 3, -1024), (-7, (1 << 20) - 1, 1024), (-7, 1 << 20, 1024), ((1 << 30) - 1024, (1 << 20) - 1, 1024), (1, (1 << 20) + 5, -3)]
    blob = struct.pack("<fI", voxel, len(params))
    for has, p in params:
        blob += struct.pack("<ifIII", has, *p)
    blob += struct.pack("<I", len(quanta)) + b"".join(struct.pack("<fff", *q) for q in quanta)
    blob += struct.pack("<I", len(edges)) + b"".join(struct.pack("<iIiI", *e) for e in edges)
    blob += struct.pack("<I", len(updates)) + b"".join(struct.pack("<iIi", *u) for u in updates)
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-3000:])
    rows = [ln.split() for ln in r.stdout.decode().splitlines()]
    by = lambda key: [[int(x) for x in row[1:]] for row in rows if row[0] == key]  # noqa: E731
    for got, want in zip(by("param"), want_params):
        assert got[0] == (want is not None)
        if want is not None:
            assert got[1] == int(np.frombuffer(F(want[0]).tobytes(), np.uint32)[0]) and got[2] == want[1]
    assert len(by("param")) == len(params)
    with np.errstate(all="ignore"):
        assert [g[0] for g in by("q")] == [int(np.rint(((dc - z) / t) * F(1024))) for dc, z, t in quanta] and len(quanta) > 500
    assert max(abs(g[0]) for g in by("q")) == 1024
    want_alpha = [F(np.float64(s0 * w1) / np.float64(s0 * w1 - s1 * w0)) for s0, w0, s1, w1 in edges]
    assert [g[0] for g in by("alpha")] == [int(np.frombuffer(a.tobytes(), np.uint32)[0]) for a in want_alpha]
    assert all(0 <= a <= 1 for a in want_alpha)
    assert by("update") == [[0, 1024, 1], [0, -1019, 4], [0, 1017, 1 << 20], [1, -7, 1 << 20], [0, 1 << 30, 1 << 20], [1, 1, (1 << 20) + 5]]
    # the table: the header's, the program's geometric decision and the specification's are one
    table = tr.swap_table()
    assert [g[1] for g in by("swap")] == [g[1] for g in by("geo")] == table == list(mapfile.TSDF_SWAP)
    assert [g[1:] for g in by("corner")] == [list(tr.tetra_corners(k)) for k in range(6)]
    tris = {(g[0], g[1]): g[2] for g in by("tri")}
    for code in range(16):
        ins = [bool((code >> i) & 1) for i in range(4)]
        want = tr.case_triangles(ins)
        assert [tris.get((code, j)) for j in range(len(want))] == [sum((i | (j << 2)) << (4 * q) for q, (i, j) in enumerate(t)) for t in want]
        assert (code, len(want)) not in tris
    # the edge of type t at a cell belongs to the cubes at cell - o for the corners o that share no bit with t + 1
    own, chain = dict(by("own")), dict(by("chain"))
    for t in range(7):
        want = sum(1 << o for o in range(8) if not (o & (t + 1)))
        assert own[t] == chain[t] == want and bin(want).count("1") == 1 << (3 - bin(t + 1).count("1"))
