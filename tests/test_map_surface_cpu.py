"""Colour and normals on the TSDF surface without a GPU: the exports and the two records' layout; revo_amd.mapfile's
vectorised tsdf_records(bgr=) and mesh_attr_records against the per-cell and per-vertex specification tests/map_surface_ref.py on
every shared case; the stated exact properties; every refused argument; api.TsdfVolume with colour, the npz and PLY round trips
with the attributes and byte-identical without them; the tsdf --color / mesh --normals --colors commands on the golden map; and
tests/cpp/surface_host.cpp, the header host and device code share."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, api, mapfile, ply
from revo_amd.settings import MapTsdfColor, MapTsdfColorInfo

import map_surface_cases as su
import map_surface_ref as sf
import map_tsdf_cases as tc
import map_tsdf_ref as tr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "small_map.rvm")


def test_declared_exported_and_laid_out(tmp_path):
    for name in ("revo_map_tsdf_fuse_color", "revo_map_tsdf_mesh_attr"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    recs = {"revo_map_tsdf_color": (MapTsdfColor, 16), "revo_map_tsdf_color_info": (MapTsdfColorInfo, 32)}
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
    assert mapfile.TSDF_COLOR_DTYPE == sf.COLOR and mapfile.TSDF_COLOR_DTYPE.itemsize == 16 and mapfile.TSDF_COLOR_INFO_KEYS == sf.COLOR_KEYS
    assert [f for f, _ in MapTsdfColor._fields_] == list(sf.COLOR.names) and [f for f, _ in MapTsdfColorInfo._fields_][:2] == list(sf.COLOR_KEYS)


# ---------------------------------------------------------------------------------------------------------------- fusion --
@pytest.mark.parametrize("name", su.FUSE_NAMES)
def test_tsdf_records_with_colour_follow_the_specification(name):
    c = su.fuse_cases()[name]
    want = su.fuse_spec(name)
    got = mapfile.tsdf_records(tc.V, c["lo"], c["n"], c["views"], c["trunc"], bgr=c["bgr"])
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2]
    assert got[3].dtype == mapfile.TSDF_COLOR_DTYPE and got[3].tobytes() == want[3].tobytes() and got[4] == want[4]
    # the tsdf volume, info and view counts are those of the call without colour
    plain = mapfile.tsdf_records(tc.V, c["lo"], c["n"], c["views"], c["trunc"])
    assert plain[0].tobytes() == got[0].tobytes() and plain[1] == got[1] and plain[2] == got[2]
    assert got[0].tobytes() == tc.fuse_spec(name)[0].tobytes()
    assert got[4]["color_updates"] == int(got[3]["weight"].sum()) and np.all(got[3]["weight"] <= got[0]["weight"])
    assert mapfile.tsdf_records(tc.V, c["lo"], c["n"], c["views"], c["trunc"], bgr=c["bgr"], chunk=50)[3].tobytes() == want[3].tobytes()


def test_the_cases_colour_something():
    assert su.fuse_spec("64 views")[4]["color_updates"] > 100 and su.fuse_spec("3x3x33")[4]["cells_colored"] > 0
    assert su.fuse_spec("plane alone")[4]["cells_colored"] > 0


def test_the_exact_properties():
    c = su.fuse_cases()["64 views"]
    lo, n, views, bgr = c["lo"], c["n"], c["views"][:8], c["bgr"][:8]
    whole = mapfile.tsdf_records(tc.V, lo, n, views, bgr=bgr)
    assert whole[1]["saturated"] == 0 and whole[4]["color_updates"] > 0
    # the order of the views cannot show in either volume
    for order in (list(range(8))[::-1], [3, 4, 5, 6, 7, 0, 1, 2]):
        got = mapfile.tsdf_records(tc.V, lo, n, [views[i] for i in order], bgr=[bgr[i] for i in order])
        assert got[0].tobytes() == whole[0].tobytes() and got[3].tobytes() == whole[3].tobytes() and got[4] == whole[4]
    # A and then an accumulating call with B leave the bytes of one call with A and B
    a = mapfile.tsdf_records(tc.V, lo, n, views[:3], bgr=bgr[:3])
    keep = (a[0].tobytes(), a[3].tobytes())
    ab = mapfile.tsdf_records(tc.V, lo, n, views[3:], bgr=bgr[3:], tsdf=a[0], color=a[3])
    assert ab[0].tobytes() == whole[0].tobytes() and ab[3].tobytes() == whole[3].tobytes()
    assert ab[4]["cells_colored"] == whole[4]["cells_colored"] and a[4]["color_updates"] + ab[4]["color_updates"] == whole[4]["color_updates"]
    assert (a[0].tobytes(), a[3].tobytes()) == keep  # the volumes accumulated into are not changed
    spec = sf.fuse_color(tc.V, lo, n, views[3:], bgr[3:], tsdf=a[0], color=a[3])
    assert spec[0].tobytes() == whole[0].tobytes() and spec[3].tobytes() == whole[3].tobytes()
    # a negative sum needs a CONFIRMED update: every inside cell is coloured
    for name in su.FUSE_NAMES:
        cells, _, _, col, _ = su.fuse_spec(name)
        assert np.all(col["weight"][cells["sum"] < 0] > 0)
    # saturation: one update under a full weight, two CONFIRMED views: the second leaves both cells alone
    w = tc.wall()
    vol, col = su.nearly_full(w["n"])
    two = w["views"] * 2
    img = [su.wall_image((1, 2, 3)), su.wall_image((200, 100, 50))]
    got = mapfile.tsdf_records(tc.V, w["lo"], w["n"], two, bgr=img, tsdf=vol, color=col)
    want = sf.fuse_color(tc.V, w["lo"], w["n"], two, img, tsdf=vol, color=col)
    assert got[0].tobytes() == want[0].tobytes() and got[3].tobytes() == want[3].tobytes() and got[1] == want[1] and got[4] == want[4]
    assert got[1]["saturated"] == got[1]["updates"] == vol.size and got[4]["color_updates"] == vol.size
    assert np.all(got[3]["weight"] == 6) and np.all(got[3]["sum_b"] == 101) and np.all(got[3]["sum_r"] == 1278)


def test_refused_fuse_arguments():
    c = su.fuse_cases()["two views"]
    lo, n, views, bgr = c["lo"], c["n"], c["views"], c["bgr"]
    ok = mapfile.tsdf_records(tc.V, lo, n, views, bgr=bgr)
    for bad in ([bgr[0]], [bgr[0], None], [bgr[0], bgr[1][:, :-1]], [bgr[0], bgr[1].astype(np.int32)], [bgr[0], bgr[1][..., :2]], bgr + bgr[:1]):
        with pytest.raises(ValueError):
            mapfile.tsdf_records(tc.V, lo, n, views, bgr=bad)
    with pytest.raises(ValueError):  # both volumes or none
        mapfile.tsdf_records(tc.V, lo, n, views, bgr=bgr, tsdf=ok[0])
    with pytest.raises(ValueError):
        mapfile.tsdf_records(tc.V, lo, n, views, bgr=bgr, color=ok[3])
    with pytest.raises(ValueError):  # a colour volume without images
        mapfile.tsdf_records(tc.V, lo, n, views, tsdf=ok[0], color=ok[3])
    with pytest.raises(ValueError):
        mapfile.tsdf_records(tc.V, lo, n, views, bgr=bgr, tsdf=ok[0], color=ok[3][:-1])
    with pytest.raises(ValueError):
        mapfile.tsdf_records(tc.V, lo, n, views, bgr=bgr, tsdf=ok[0], color=ok[3].view(np.uint32).reshape(ok[3].shape + (4,)))


# --------------------------------------------------------------------------------------------------------- the attributes --
@pytest.mark.parametrize("name", list(su.mesh_cases()))
def test_mesh_attr_records_follow_the_specification(name):
    c = su.mesh_cases()[name]
    v, t, info, normals, colours = su.mesh_spec(name)
    got = mapfile.mesh_attr_records(c["cells"], c["color"], c["lo"], tc.V, c["min_weight"])
    plain = mapfile.mesh_records(c["cells"], c["lo"], tc.V, c["min_weight"])
    assert got.vertices.tobytes() == plain.vertices.tobytes() == v.tobytes() and got.triangles.tobytes() == plain.triangles.tobytes() == t.tobytes()
    assert got.info == plain.info == info
    assert got.normals.dtype == F and got.normals.shape == (len(v), 3) and got.normals.tobytes() == normals.tobytes()
    assert got.colors.dtype == np.uint8 and got.colors.shape == (len(v), 4) and got.colors.tobytes() == colours.tobytes()
    without = mapfile.mesh_attr_records(c["cells"], None, c["lo"], tc.V, c["min_weight"])
    assert without.colors is None and without.normals.tobytes() == normals.tobytes()
    ln = np.linalg.norm(normals.astype(np.float64), axis=1)
    assert np.all((np.abs(ln - 1) < 1e-6) | (ln == 0))


def _gradient_cases(cells, min_weight):
    """Which of (c - e valid, c + e valid) occur over the end cells of the mesh's edges and the three axes."""
    seen = set()
    for c0, typ in sf.vertex_edges(cells, min_weight):
        d = tr.offset(typ + 1)
        for cell in (c0, (c0[0] + d[0], c0[1] + d[1], c0[2] + d[2])):
            for axis in range(3):
                ok = []
                for s in (-1, 1):
                    x = tuple(cell[i] + s * (i == axis) for i in range(3))
                    ok.append(all(0 <= x[i] < cells.shape[i] for i in range(3)) and int(cells[x]["weight"]) >= max(1, min_weight))
                seen.add(tuple(ok))
    return seen


def test_the_cases_reach_every_rule():
    _, _, _, normals, colours = su.mesh_spec("256 patterns")
    assert set(np.unique(colours[:, 3]).tolist()) == {0, 1, 2}
    assert np.all(colours[colours[:, 3] == 0, :3] == 0)
    # A cube between planes of weight-0 cells has only one-sided axes; the sphere, all valid, has two-sided ones and the box's faces.
    # An edge's end is a corner of an active cube, so one neighbour per axis is always valid: the neither-valid case cannot be
    # reached through a mesh and is checked on the shared header alone (test_host_header).
    assert _gradient_cases(su.mesh_cases()["256 patterns"]["cells"], 1) == {(False, True), (True, False)}
    assert (True, True) in _gradient_cases(su.mesh_cases()["sphere"]["cells"], 1)
    assert _gradient_cases(su.mesh_cases()["weights 2 .. 5, min_weight 3"]["cells"], 3) == {(False, True), (True, False), (True, True)}
    # f = -1 on the plane x = 0 and 0 on x = 1: the gradient is (1, 0, 0) at every cell, and so is every normal
    flat = tc.volume(np.full((2, 2, 2), -1), np.ones((2, 2, 2), np.int64))
    flat["sum"][1] = 0
    m = mapfile.mesh_attr_records(flat, None, (0, 0, 0), tc.V)
    assert len(m.vertices) == 9 and np.all(m.normals[:, 0] == 1) and np.all(m.normals[:, 1:] == 0)


def test_the_sphere_and_the_wall():
    c = su.mesh_cases()["sphere"]
    m = mapfile.mesh_attr_records(c["cells"], None, c["lo"], tc.V)
    face = np.zeros((len(m.vertices), 3))
    p = m.vertices.astype(np.float64)
    t = m.triangles.astype(np.int64)
    fn = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    for k in range(3):
        np.add.at(face, t[:, k], fn)
    assert np.all(np.einsum("ij,ij->i", face, m.normals.astype(np.float64)) > 0)
    w = tc.wall()
    colour = (17, 130, 251)
    cells, _, _, col, cinfo = mapfile.tsdf_records(tc.V, w["lo"], w["n"], w["views"], w["trunc"], bgr=[su.wall_image(colour)])
    m = mapfile.mesh_attr_records(cells, col, w["lo"], tc.V)
    assert len(m.vertices) and np.all(m.colors[:, :3] == np.array(colour, np.uint8)) and np.all(m.colors[:, 3] >= 1)
    assert cinfo["cells_colored"] == cells.size
    # fused through the colour call only: no vertex is without a colour
    for name in su.FUSE_NAMES:
        c = su.fuse_cases()[name]
        cells, _, _, col, _ = su.fuse_spec(name)
        m = mapfile.mesh_attr_records(cells, col, c["lo"], tc.V)
        assert not len(m.colors) or int(m.colors[:, 3].min()) >= 1


def test_refused_mesh_arguments():
    c = su.mesh_cases()["min_weight 1"]
    for bad in (c["color"][:-1], c["color"].view(np.uint32).reshape(c["color"].shape + (4,)), np.zeros(c["cells"].shape, tr.CELL)):
        with pytest.raises(ValueError):
            mapfile.mesh_attr_records(c["cells"], bad, c["lo"], tc.V)
    with pytest.raises(ValueError):
        mapfile.mesh_attr_records(c["color"], c["color"], c["lo"], tc.V)
    with pytest.raises(ValueError):
        mapfile.Mesh(np.zeros((3, 3)), np.zeros((1, 3)), None, np.zeros((2, 3)))
    vol = api.TsdfVolume(c["cells"], c["lo"], tc.V, None)
    with pytest.raises(ValueError):
        vol.mesh(colors=True)
    with pytest.raises(ValueError):
        api.TsdfVolume(c["cells"], c["lo"], tc.V, None, color=c["color"][:-1])


# ------------------------------------------------------------------------------------------------------------------ files --
def test_volume_npz_and_ply(tmp_path):
    c = su.mesh_cases()["sphere"]
    plain = api.TsdfVolume(c["cells"], c["lo"], tc.V, 0.3)
    full = api.TsdfVolume(c["cells"], c["lo"], tc.V, 0.3, color=c["color"])
    a, b, old = (str(tmp_path / x) for x in ("plain.npz", "colour.npz", "old.npz"))
    plain.save(a)
    full.save(b)
    mapfile.write_tsdf(old, c["cells"], c["lo"], tc.V, 0.3)
    assert open(a, "rb").read() == open(old, "rb").read()  # a file without colour is what it was
    with np.load(a) as z:
        assert sorted(z.files) == ["lo", "n", "sum", "trunc", "voxel", "weight"]
    back = api.TsdfVolume.load(b)
    assert back.color.tobytes() == c["color"].tobytes() and back.cells.tobytes() == c["cells"].tobytes() and back.trunc == plain.trunc
    assert api.TsdfVolume.load(a).color is None and len(mapfile.read_tsdf(b)) == 4
    # a loaded volume without a map is meshed by the numpy contract
    m = back.mesh(normals=True, colors=True)
    want = mapfile.mesh_attr_records(c["cells"], c["color"], c["lo"], tc.V)
    assert m.normals.tobytes() == want.normals.tobytes() and m.colors.tobytes() == want.colors.tobytes()
    assert back.mesh(colors=True).normals is None and back.mesh(normals=True).colors is None and back.mesh().normals is None
    # PLY: with both, with one, and without (byte for byte the file of the plain mesh)
    p0, p1, p2, p3 = (str(tmp_path / x) for x in ("plain.ply", "both.ply", "n.ply", "c.ply"))
    ply.write_mesh_ply(p0, want.vertices, want.triangles)
    mapfile.Mesh(want.vertices, want.triangles).save_ply(p1)
    assert open(p0, "rb").read() == open(p1, "rb").read()
    assert open(p0, "rb").read()[:400].count(b"property") == 4
    want.save_ply(p1)
    mapfile.Mesh(want.vertices, want.triangles, None, want.normals).save_ply(p2)
    mapfile.Mesh(want.vertices, want.triangles, None, None, want.colors).save_ply(p3)
    for path, has_n, has_c in ((p1, True, True), (p2, True, False), (p3, False, True), (p0, False, False)):
        r = mapfile.Mesh.load_ply(path)
        assert r.vertices.tobytes() == want.vertices.tobytes() and r.triangles.tobytes() == want.triangles.tobytes()
        assert (r.normals is not None) == has_n and (r.colors is not None) == has_c
        if has_n:
            assert r.normals.tobytes() == want.normals.tobytes()
        if has_c:
            assert np.array_equal(r.colors[:, :3], want.colors[:, :3])
        assert len(ply.read_mesh_ply(path)) == 2 and ply.read_mesh_ply(path)[0].tobytes() == want.vertices.tobytes()
    head = open(p1, "rb").read(400)
    assert b"property float nx" in head and b"property uchar red" in head and head.index(b"nx") < head.index(b"red")
    size = os.path.getsize(p1)
    assert size == head.index(b"end_header\n") + 11 + 27 * len(want.vertices) + 13 * len(want.triangles)


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
    views, bgr, stamps = [], [], [(1.5, np.eye(4, dtype=F)), (2.5, T2)]
    rng = np.random.default_rng(27)
    with open(os.path.join(folder, "poses.txt"), "w") as f:
        f.write("".join(line + "\n" for line in vo.tum_lines(stamps)))
    with open(os.path.join(folder, "associate.txt"), "w") as f:
        for i, (ts, T) in enumerate(stamps):
            D = np.full((48, 64), depth + 0.01 * i, F)
            D[:6] = 0.0
            name = "%.6f.png" % ts
            raw = np.rint(D * 5000.0).astype(np.uint16)
            im = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
            Image.fromarray(raw).save(os.path.join(folder, "depth", name))
            Image.fromarray(np.ascontiguousarray(im[..., ::-1])).save(os.path.join(folder, "rgb", name))  # the file holds R, G, B
            f.write("%.6f rgb/%s %.6f depth/%s\n" % (ts, name, ts, name))
            views.append((raw.astype(F) / F(5000.0), T, k))
            bgr.append(im)
    cam = ["--camera", "16", "16", "31.5", "23.5", "--zrange", "0.1", "5.2"]
    assert mapfile.main(["tsdf", GOLDEN, "--views", folder, "--color", "-o", out, "--pad", "2", "--trunc", "0.3"] + cam) == 0
    blo, n = mapfile.padded_box(lo, hi, 2)
    want = mapfile.tsdf_records(header["voxel"], blo, n, views, 0.3, bgr=bgr)
    cells, tlo, voxel, trunc, col = mapfile.read_tsdf(out, color=True)
    assert cells.tobytes() == want[0].tobytes() and col.tobytes() == want[3].tobytes() and tlo.tolist() == blo.tolist()
    assert want[4]["cells_colored"] > 100
    assert mapfile.main(["mesh", out, "--normals", "--colors", "-o", mesh_out]) == 0
    wm = mapfile.mesh_attr_records(want[0], want[3], blo, header["voxel"])
    got = mapfile.Mesh.load_ply(mesh_out)
    assert got.vertices.tobytes() == wm.vertices.tobytes() and got.triangles.tobytes() == wm.triangles.tobytes() and len(wm.triangles) > 1000
    assert got.normals.tobytes() == wm.normals.tobytes() and np.array_equal(got.colors[:, :3], wm.colors[:, :3])
    assert int(wm.colors[:, 3].min()) >= 1 and len(np.unique(wm.colors[:, :3], axis=0)) > 100
    assert mapfile.main(["mesh", out, "--normals", "-o", mesh_out]) == 0
    got = mapfile.Mesh.load_ply(mesh_out)
    assert got.colors is None and got.normals.tobytes() == wm.normals.tobytes()
    assert mapfile.main(["mesh", out, "--colors", "--min-weight", "2", "-o", mesh_out]) == 0
    got = mapfile.Mesh.load_ply(mesh_out)
    assert got.normals is None and np.array_equal(got.colors[:, :3], mapfile.mesh_attr_records(want[0], want[3], blo, voxel, 2).colors[:, :3])
    # without the flags the two commands write what they wrote before
    plain, plain_mesh = str(tmp_path / "plain.npz"), str(tmp_path / "plain.ply")
    assert mapfile.main(["tsdf", GOLDEN, "--views", folder, "-o", plain, "--pad", "2", "--trunc", "0.3"] + cam) == 0
    with np.load(plain) as z:
        assert "color_sum" not in z.files and z["sum"].tobytes() == want[0]["sum"].tobytes()
    assert mapfile.main(["mesh", plain, "-o", plain_mesh]) == 0
    ply.write_mesh_ply(mesh_out, wm.vertices, wm.triangles)
    assert open(plain_mesh, "rb").read() == open(mesh_out, "rb").read()
    assert mapfile.main(["mesh", plain, "--colors", "-o", mesh_out]) == 1  # no colour volume in the file
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------- the shared header --
def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "surface_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "surface_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def _bits(x):
    return int(np.frombuffer(F(x).tobytes(), np.uint32)[0])


def test_host_header(tmp_path):
    """revo_tsdf_host.h: the colour update with its saturation tie to the TSDF update, the field, the gradient's cases, the
    interpolated normal with the zero gradient, the colour byte at k = 0, 1, 2 and at v exactly on .5, and the bgr argument rule."""
    exe = _host(tmp_path)
    rng = np.random.default_rng(27)
    W = 1 << 20
    # sum, weight, q, confirmed, (sum_b, sum_g, sum_r, weight), (b, g, r)
    updates = [(0, 0, 0, 1, (0, 0, 0, 0), (7, 8, 9)), (0, 0, 1024, 0, (1, 2, 3, 4), (7, 8, 9)), (-7, W - 1, -5, 1, (10, 20, 30, 5), (255, 0, 1)),
               (-7, W, -5, 1, (10, 20, 30, 5), (255, 0, 1)), (3, W + 9, 1024, 0, (1, 1, 1, 1), (2, 2, 2)),
               (5, W - 1, 0, 1, (255 * (W - 1), 0, 255 * (W - 1), W - 1), (255, 255, 255))]
    want_updates = [[0, 0, 1, 1, 7, 8, 9, 1], [0, 1024, 1, 0, 1, 2, 3, 4], [0, -12, W, 1, 265, 20, 31, 6], [1, -7, W, 0, 10, 20, 30, 5],
                    [1, 3, W + 9, 0, 1, 1, 1, 1], [0, 5, W, 1, 255 * W, 255, 255 * W, W]]
    fields = [(-1, 1), (1 << 30, 1 << 20), (1023, 3), (16777217, 3), (255 * W, W)] + [(int(rng.integers(0, 1 << 30)), int(rng.integers(1, W + 1))) for _ in range(50)]
    grads = [(1, F(-2.5), F(9), 1, F(3.25)), (0, F(-2.5), F(0.5), 1, F(3.25)), (1, F(-2.5), F(0.5), 0, F(3.25)), (0, F(1), F(2), 0, F(3))]
    grads += [(int(rng.integers(2)), F(rng.normal() * 300), F(rng.normal() * 300), int(rng.integers(2)), F(rng.normal() * 300)) for _ in range(60)]
    normals = [tuple(F(x) for x in (0, 0, 0, 0, 0, 0, 0.5)), tuple(F(x) for x in (1, 2, 3, -1, -2, -3, 0.5)), tuple(F(x) for x in (3e38, 3e38, 0, 3e38, 3e38, 0, 0.25)),
               tuple(F(x) for x in (0, 0, 5, 0, 0, 5, 1))]
    normals += [tuple(F(x) for x in list(rng.normal(size=6) * 10.0 ** rng.integers(-3, 4)) + [rng.uniform()]) for _ in range(60)]
    # s0, w0, s1, w1, a: k = 0, 1 (either end), 2; v exactly on .5 (ties to even)
    bytes_ = [(9, 0, 9, 0, F(0.5)), (7, 2, 0, 0, F(0.9)), (0, 0, 9, 2, F(0.1)), (5, 2, 5, 2, F(0.3)), (1, 2, 0, 0, F(0)), (3, 2, 0, 0, F(0)), (509, 2, 0, 0, F(0)),
               (0, 1, 1, 1, F(0.5)), (1, 1, 2, 1, F(0.5)), (255, 1, 255, 1, F(1)), (255 * W, W, 0, 1, F(0))]
    bytes_ += [(int(rng.integers(0, 256 * 7)), 7, int(rng.integers(0, 256 * 3)), 3, F(rng.uniform())) for _ in range(60)]
    blob = struct.pack("<I", len(updates)) + b"".join(struct.pack("<iIiI4I3I", s, w, q, c, *col, *px) for s, w, q, c, col, px in updates)
    blob += struct.pack("<I", len(fields)) + b"".join(struct.pack("<iI", *x) for x in fields)
    blob += struct.pack("<I", len(grads)) + b"".join(struct.pack("<IffIf", *x) for x in grads)
    blob += struct.pack("<I", len(normals)) + b"".join(struct.pack("<7f", *x) for x in normals)
    blob += struct.pack("<I", len(bytes_)) + b"".join(struct.pack("<4If", *x) for x in bytes_)
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-3000:])
    rows = [ln.split() for ln in r.stdout.decode().splitlines()]
    by = lambda key: [[int(x) for x in row[1:]] for row in rows if row[0] == key]  # noqa: E731
    assert by("update") == want_updates
    assert by("field") == [[_bits(F(s) / F(w)), _bits(F(s & 0xffffffff) / F(w))] for s, w in fields]
    want = []
    for vm, fm, fc, vp, fp in grads:
        want.append([_bits((fp - fm) * F(0.5) if vm and vp else fp - fc if vp else fc - fm if vm else F(0))])
    assert by("grad") == want and by("grad")[3] == [0]
    want = []
    with np.errstate(all="ignore"):
        for g in normals:
            v = [g[i] + g[6] * (g[3 + i] - g[i]) for i in range(3)]
            l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
            want.append([0, 0, 0] if not np.isfinite(l2) or l2 == 0 else [_bits(x / np.sqrt(l2)) for x in v])
    assert by("normal") == want and by("normal")[0] == [0, 0, 0] and by("normal")[2] == [0, 0, 0] and by("normal")[3] == [0, 0, _bits(1)]
    want = []
    for s0, w0, s1, w1, a in bytes_:
        m0, m1 = (F(s0) / F(w0) if w0 else None), (F(s1) / F(w1) if w1 else None)
        v = m0 + a * (m1 - m0) if w0 and w1 else m0 if w0 else m1 if w1 else F(0)
        want.append([int(np.rint(min(max(v, F(0)), F(255)))), (w0 > 0) + (w1 > 0)])
    assert by("byte") == want
    assert [b[0] for b in by("byte")[:11]] == [0, 4, 4, 2, 0, 2, 254, 0, 2, 255, 255] and [b[1] for b in by("byte")[:4]] == [0, 1, 1, 2]
    assert by("bgr") == [[1, 0], [0, 1]]


def test_run_tum_surface_usage_errors(capsys):
    """The option rules of run_tum --surface are decided before any file is read or a device is opened."""
    from revo_amd import run_tum
    base = ["settings.yaml", "dataset.yaml"]
    for extra in (["--surface", "s.ply"],                                             # without --map
                  ["--map", "0.02", "--surface-trunc", "0.2"],                        # a sub-option without --surface
                  ["--map", "0.02", "--surface", "s.ply", "--map-window", "2"],
                  ["--map", "0.02", "--surface", "s.ply", "--streams", "2"],
                  ["--map", "0.02", "--surface", "s.ply", "--surface-box", "0", "0", "0", "0", "4", "4"],
                  ["--map", "0.02", "--surface", "s.ply", "--surface-box", "0", "0", "0", "4", "4"],
                  ["--map", "0.02", "--surface", "s.ply", "--surface-trunc", "0"],
                  ["--map", "0.02", "--surface", "s.ply", "--surface-min-weight", "x"]):
        assert run_tum.main(base + extra) == 2, extra
    assert "--surface" in capsys.readouterr().out
