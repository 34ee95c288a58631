"""Known space without a GPU: the exports and the records' layout; revo_amd.mapfile's vectorised observe_records,
known_field_records and frontier_records against the per-cell specification tests/map_seen_ref.py on every shared case; the
named cells have the class their case was built for; the byte rule; the three exact properties; the degenerate fields; the
route around and not through unseen space; api.SeenVolume; the observe / esdf --seen / plan --seen / frontiers commands on the
golden map; and tests/cpp/seen_host.cpp, the header host and device code share."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, api, mapfile
from revo_amd.settings import DF_NONE, MapKnownInfo, MapObserveInfo, MapObserveParams

import map_carve_ref as mc
import map_seen_cases as sc
import map_seen_ref as sr

F = np.float32
RAW = mapfile.RAW_DTYPE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "small_map.rvm")
EMPTY = np.zeros(0, RAW)


def test_declared_exported_and_laid_out(tmp_path):
    for name in ("revo_map_observe", "revo_map_known_field", "revo_map_frontiers"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    recs = {"revo_map_observe_params": (MapObserveParams, 16), "revo_map_observe_info": (MapObserveInfo, 64),
            "revo_map_known_info": (MapKnownInfo, 64)}
    body = ""
    for cname, (cls, _) in recs.items():
        body += '  printf("%s %%zu\\n", sizeof(%s));\n' % (cname, cname)
        for f, _t in cls._fields_:
            body += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (cname, f, cname, f)
    for f in ("cells", "solid", "outside", "below", "max_d2"):
        body += '  printf("df.%s %%zu\\n", offsetof(revo_map_df_info, %s));\n' % (f, f)
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
    for f in ("cells", "solid", "outside", "below", "max_d2"):  # the kernels share the line
        assert int(got["df." + f]) == getattr(MapKnownInfo, f).offset
    assert mapfile.SEEN_INFO_KEYS == sr.INFO_KEYS and mapfile.KNOWN_INFO_KEYS == sr.KNOWN_KEYS


# ------------------------------------------------------------------------------------------------------------- observe --
@pytest.mark.parametrize("name", list(sc.cases()))
def test_observe_records_follow_the_specification(name):
    c = sc.cases()[name]
    want = sc.spec(name)
    got = mapfile.observe_records(sc.V, c["lo"], c["n"], c["views"], c["radius"], c["margin"], c["margin_rel"])
    print(name, want[1], want[2][0])
    assert got[0].dtype == np.uint8 and got[0].tobytes() == want[0].tobytes()
    assert got[1] == want[1] and got[2] == want[2]
    assert all(sum(v.values()) == want[1]["cells"] for v in want[2])
    # in pieces: the chunks of the vectorised form cannot show
    assert mapfile.observe_records(sc.V, c["lo"], c["n"], c["views"], c["radius"], c["margin"], c["margin_rel"], chunk=50)[0].tobytes() == want[0].tobytes()


def _class_of(name, cell, view=0):
    n = sc.cases()[name]["n"]
    return mc.CLASSES[sc.spec(name)[3][(cell[0] * n[1] + cell[1]) * n[2] + cell[2], view]]


def test_named_cells_have_their_class():
    for cell, (_, _, cls) in sc.PIXELS.items():
        assert _class_of("plane alone, radius 0", sc.plane_cell(cell)) == cls, cell
    r1 = "9x7x5 radius 1"
    assert _class_of(r1, sc.plane_cell("edge_centre")) == "edge" and _class_of(r1, sc.plane_cell("free")) == "free"
    assert _class_of(r1, sc.plane_cell("unknown_nan")) == "unknown" and _class_of(r1, (0, 0, 2)) == "unknown"  # a NaN in the window's corner
    # the windows at the borders: view 1 puts the plane's x index on pixel i + 4, view 2 on i + 12, views 3 and 4 likewise along v
    for r in range(4):
        name = "9x7x5 radius %d" % r
        for ix in range(9):
            assert _class_of(name, (ix, 3, 2), 1) == ("outside" if ix - r < 0 else "free"), (r, ix)
            assert _class_of(name, (ix, 3, 2), 2) == ("outside" if ix + 8 + r > 15 else "free"), (r, ix)
        for iy in range(7):
            assert _class_of(name, (4, iy, 2), 3) == ("outside" if iy - r < 0 else "free"), (r, iy)
            assert _class_of(name, (4, iy, 2), 4) == ("outside" if iy + 6 + r > 11 else "free"), (r, iy)
    seen, info, counts, cls = sc.spec("behind")
    assert not seen.any() and counts[0]["outside"] == info["cells"] and info["newly_known"] == 0
    seen, info, _, cls = sc.spec("64 views")
    assert cls.shape[1] == 64 and int((seen & 0x7F).max()) > 32 and info["votes"] == int((cls == mc.FREE).sum())
    assert sc.spec("1x1x1 radius 0")[0].shape == (1, 1, 1)


def test_the_byte():
    assert sr.byte(0x7D, 8, 0) == 0x7F == int(mapfile.seen_update([0x7D], [8], [0])[0])
    assert sr.byte(0x7F, 64, 0) == 0x7F and sr.byte(0x00, 64, 1) == 0xC0
    for b_in in range(256):  # the surface bit survives and never leaks into the count
        for f in (0, 1, 3, 64):
            for s in (0, 1):
                b = sr.byte(b_in, f, s)
                assert b == int(mapfile.seen_update([b_in], [f], [s])[0])
                assert (b & 0x80) == ((b_in & 0x80) | (s << 7)) and (b & 0x7F) == min(127, (b_in & 0x7F) + f)


def test_the_three_exact_properties():
    c = sc.cases()["9x7x5 radius 1"]
    kw = dict(radius=1, margin=sc.M)
    views = c["views"]
    whole = mapfile.observe_records(sc.V, c["lo"], c["n"], views, **kw)
    # the order of the views cannot show
    back = mapfile.observe_records(sc.V, c["lo"], c["n"], views[::-1], **kw)
    assert back[0].tobytes() == whole[0].tobytes() and back[1] == whole[1] and back[2] == whole[2][::-1]
    # observe(A) then an accumulating observe(B) is observe(A + B); the specification's loop says the same
    a = mapfile.observe_records(sc.V, c["lo"], c["n"], views[:3], **kw)
    ab = mapfile.observe_records(sc.V, c["lo"], c["n"], views[3:], seen=a[0], **kw)
    assert ab[0].tobytes() == whole[0].tobytes() and a[1]["votes"] + ab[1]["votes"] == whole[1]["votes"]
    assert a[1]["newly_known"] + ab[1]["newly_known"] == whole[1]["newly_known"] == int((whole[0] != 0).sum())
    assert sr.observe(sc.V, c["lo"], c["n"], views[3:], seen=a[0], **kw)[0].tobytes() == whole[0].tobytes()
    # ... saturation included: the 64 views three times over end at 127 where they give 43 votes or more
    v64 = sc.cases()["64 views"]["views"]
    once = mapfile.observe_records(sc.V, c["lo"], c["n"], v64, **kw)
    thrice = mapfile.observe_records(sc.V, c["lo"], c["n"], v64, seen=mapfile.observe_records(sc.V, c["lo"], c["n"], v64, seen=once[0], **kw)[0], **kw)
    want = np.minimum(127, 3 * (once[0] & 0x7F).astype(int)).astype(np.uint8) | (once[0] & 0x80)
    assert thrice[0].tobytes() == want.tobytes() and int((thrice[0] & 0x7F).max()) == 127 > int((once[0] & 0x7F).max()) >= 43
    near = np.full(tuple(c["n"]), 0x7D, np.uint8)
    full = mapfile.observe_records(sc.V, c["lo"], c["n"], v64[:8], seen=near, **kw)
    assert set(np.unique(full[0] & 0x7F)) <= set(range(0x7D, 0x80)) and 0x7F in (full[0] & 0x7F)
    # a call that does not accumulate takes no volume
    assert mapfile.observe_records(sc.V, c["lo"], c["n"], views, seen=None, **kw)[0].tobytes() == whole[0].tobytes()
    with pytest.raises(ValueError):
        mapfile.observe_records(sc.V, c["lo"], c["n"], views, seen=near[:-1], **kw)
    for bad in (dict(radius=4), dict(margin=-1.0), dict(margin_rel=np.nan)):
        with pytest.raises(ValueError):
            mapfile.observe_records(sc.V, c["lo"], c["n"], views, **dict(kw, **bad))
    with pytest.raises(ValueError):
        mapfile.observe_records(sc.V, c["lo"], c["n"], [], **kw)
    with pytest.raises(ValueError):
        mapfile.observe_records(sc.V, c["lo"], (1025, 1, 1), views, **kw)


# ------------------------------------------------------------------------------------------- the field and the frontiers --
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_known_field_and_frontiers_follow_the_specification(seed):
    c = sc.random_volume(seed)
    rec = c["rec"].astype(RAW)
    for min_count, clamp, min_views in ((1, 0, 1), (2, 40, 2), (1, 0, 200)):
        want = sr.known_field(c["rec"], c["lo"], c["n"], c["seen"], min_count, clamp, min_views)
        got = mapfile.known_field_records(rec, c["lo"], c["n"], c["seen"], min_count, clamp, min_views)
        print(seed, min_count, clamp, min_views, want[1])
        assert got[0].dtype == np.uint32 and got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
        assert want[1]["unknown"] > 0 and want[1]["known_free"] + want[1]["solid"] + want[1]["unknown"] == want[1]["cells"]
        fw = sr.frontiers(c["rec"], c["lo"], c["n"], c["seen"], min_count, min_views)
        fg = mapfile.frontier_records(rec, c["lo"], c["n"], c["seen"], min_count, min_views)
        assert fg.dtype == np.int32 and fg.tolist() == fw.tolist() and (len(fw) > 0 or min_views == 200)
        a = fg - c["lo"]
        lin = (a[:, 0] * c["n"][1] + a[:, 1]) * c["n"][2] + a[:, 2]
        assert np.all(np.diff(lin) > 0)  # ascending place in the box
        if len(fw):  # a frontier cell is known and free, so not an obstacle, and next to one
            assert np.all(got[0][tuple(a.T)] == (1 if not clamp else min(1, clamp)))
    try:
        from scipy import ndimage
    except ImportError:
        return
    solid, unknown = sr.unknown_cells(c["rec"], c["lo"], c["n"], c["seen"])
    edt = ndimage.distance_transform_edt(~(solid | unknown))
    assert np.array_equal(np.rint(edt ** 2).astype(np.uint32), mapfile.known_field_records(rec, c["lo"], c["n"], c["seen"])[0])


def test_degenerate_fields():
    lo, n = (-3, 2, 1), (6, 5, 4)
    rec = sc.records_at([(-2, 3, 2), (1, 5, 4), (40, 0, 0)]).astype(RAW)
    nothing, all_seen = np.zeros(n, np.uint8), np.full(n, 0x7F, np.uint8)
    d2, info = mapfile.known_field_records(rec, lo, n, nothing)
    assert not d2.any() and info["unknown"] == info["cells"] - 2 and info["known_free"] == 0 and info["max_d2"] == 0 and info["outside"] == 1
    d2, info = mapfile.known_field_records(EMPTY, lo, n, np.full(n, 0x80, np.uint8))
    assert np.all(d2 == DF_NONE) and info["unknown"] == 0 and info["known_free"] == info["cells"] and info["max_d2"] == 0
    d2, info = mapfile.known_field_records(rec, lo, n, all_seen, clamp=7)
    plain = mapfile.distance_field_records(rec, lo, n, clamp=7)
    assert d2.tobytes() == plain[0].tobytes() and {k: info[k] for k in mapfile.DF_INFO_KEYS} == plain[1] and info["unknown"] == 0
    assert len(mapfile.frontier_records(rec, lo, n, all_seen)) == 0 and len(mapfile.frontier_records(rec, lo, n, nothing)) == 0
    with pytest.raises(ValueError):
        mapfile.known_field_records(rec, lo, n, nothing.astype(np.int8))
    with pytest.raises(ValueError):
        mapfile.frontier_records(rec, lo, n, nothing[1:])


def test_frontier_rules():
    lo, n = (10, -2, 0), (4, 3, 3)
    seen = np.full(n, 1, np.uint8)  # all free: the faces of the box are no frontier
    assert len(mapfile.frontier_records(EMPTY, lo, n, seen)) == 0 == len(sr.frontiers(EMPTY, lo, n, seen))
    seen[1, 1, 1] = 0                # one unseen cell: its six face neighbours, not the diagonal ones
    fr = mapfile.frontier_records(EMPTY, lo, n, seen)
    want = sorted([11 + d[0], -1 + d[1], 1 + d[2]] for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)))
    assert fr.tolist() == want == sr.frontiers(EMPTY, lo, n, seen).tolist()
    solid = sc.records_at([(11, -1, 1)]).astype(RAW)  # the same cell solid: known, so no frontier
    assert len(mapfile.frontier_records(solid, lo, n, seen)) == 0 == len(sr.frontiers(solid, lo, n, seen))
    assert len(mapfile.frontier_records(solid, lo, n, seen, min_count=2)) == 6  # ... unless its count is too small to be solid
    seen[1, 1, 1] = 0x80             # a surface bit: known, so no frontier
    assert len(mapfile.frontier_records(EMPTY, lo, n, seen)) == 0 == len(sr.frontiers(EMPTY, lo, n, seen))
    seen[1, 1, 1] = 1                # one vote is unseen at min_views 2, and so is everything else: nothing is free
    assert len(mapfile.frontier_records(EMPTY, lo, n, seen, min_views=2)) == 0
    seen[0, 0, 0], seen[0, 0, 1] = 0, 2  # a corner cell, at a face of the box: its neighbours inside the box decide
    seen[2, 1, 1] = 0x82             # free with the surface bit: a frontier cell like any other free one
    seen[3, 1, 1] = 0
    got = mapfile.frontier_records(EMPTY, lo, n, seen)
    assert got.tolist() == sr.frontiers(EMPTY, lo, n, seen).tolist() and [10, -2, 1] in got.tolist() and [12, -1, 1] in got.tolist()
    assert [10, -2, 0] not in got.tolist()


# --------------------------------------------------------------------------------------------------------------- the route --
def test_the_route_stays_in_known_space():
    w = sc.wall_scene()
    rec, lo, n = w["rec"].astype(RAW), w["lo"], w["n"]
    seen, info, counts = mapfile.observe_records(sc.V, lo, n, w["views"])
    print(info, counts)
    free, known = mapfile.seen_free(seen), mapfile.seen_known(seen)
    assert free[:11, :, :8].all() and not free[11:].any() and known[11:14, :, :8].all() and not known[14:].any() and not known[:, :, 15].any()
    r2 = mapfile.plan_r2(sc.V, sc.V)
    assert r2 == 1
    # the plain field: the goal behind the wall is reached around it
    plain, _ = mapfile.distance_field_records(rec, lo, n)
    cost, pinfo = mapfile.plan_records(plain, lo, n, mapfile.plan_seeds([w["goal"]]), r2)
    cells, status, _ = mapfile.plan_paths(cost, lo, n, [w["start"]])[0]
    assert pinfo["seeds_used"] == 1 and status == mapfile.PLAN_REACHED and cells[-1].tolist() == list(w["goal"])
    assert cells[:, 1].max() >= 12 and not known[tuple(cells[-1])]  # through the gap, into space no view has seen
    # the known field: the same goal is blocked
    d2, kinfo = mapfile.known_field_records(rec, lo, n, seen)
    cost, pinfo = mapfile.plan_records(d2, lo, n, mapfile.plan_seeds([w["goal"]]), r2)
    assert pinfo["seeds_blocked"] == 1 and pinfo["seeds_used"] == 0 and pinfo["reachable"] == 0
    assert kinfo["unknown"] == int((~mapfile.seen_known(seen, 1, mapfile.solid_cells(rec, lo, n)[0])).sum()) > 0
    # explore: from a seen start to the nearest frontier, through known free cells that keep the clearance
    d2e, fr, cost, einfo, (cells, status, c0) = mapfile.explore_records(rec, lo, n, sc.V, seen, w["start"], sc.V)
    assert d2e.tobytes() == d2.tobytes() and fr.tolist() == sr.frontiers(w["rec"], lo, n, seen).tolist() and len(fr) > 0
    assert einfo["seeds_used"] == len(fr) and status == mapfile.PLAN_REACHED and cells[0].tolist() == list(w["start"])
    assert cells[-1].tolist() in fr.tolist() and c0 > 0
    at = tuple((cells - np.asarray(lo)).T)
    assert free[at].all() and np.all(d2[at] >= r2)
    with pytest.raises(ValueError):
        mapfile.explore_records(rec, lo, n, sc.V, np.full(n, 1, np.uint8), w["start"], sc.V)  # all seen: nowhere to go
    with pytest.raises(ValueError):
        mapfile.explore_records(rec, lo, n, sc.V, seen, w["start"], 3 * sc.V)  # a frontier cell has d2 = 1: none keeps three cells


# ------------------------------------------------------------------------------------------------------- Python and tools --
def test_seen_volume(tmp_path):
    c = sc.cases()["9x7x5 radius 1"]
    seen, info, counts = mapfile.observe_records(sc.V, c["lo"], c["n"], c["views"], 1, sc.M)
    v = api.SeenVolume(seen, c["lo"], sc.V, info, counts)
    assert v.n.tolist() == list(c["n"]) and v.lo.dtype == np.int32 and v.voxel == sc.V and v.info == info and v.view_info == counts
    assert np.array_equal(v.free(), (seen & 0x7F) >= 1) and np.array_equal(v.free(3), (seen & 0x7F) >= 3)
    assert np.array_equal(v.known(), ((seen & 0x7F) >= 1) | (seen >= 0x80))
    solid = np.zeros(seen.shape, bool)
    solid[0, 0, 0] = True
    assert v.known(solid)[0, 0, 0] and np.array_equal(v.known(solid)[1:], v.known()[1:])
    path = v.save(str(tmp_path / "seen.npz"))
    w = api.SeenVolume.load(path)
    assert w.seen.tobytes() == seen.tobytes() and w.lo.tolist() == list(c["lo"]) and w.voxel == sc.V and w.info is None
    with pytest.raises(ValueError):
        api.SeenVolume(seen.astype(np.int32), c["lo"], sc.V)
    np.savez(str(tmp_path / "bad.npz"), seen=seen, lo=np.zeros(2, np.int32), n=np.asarray(seen.shape, np.int32), voxel=F(sc.V))
    with pytest.raises(ValueError):
        api.SeenVolume.load(str(tmp_path / "bad.npz"))


def test_command_line(tmp_path, capsys):
    from PIL import Image
    from revo_amd import vo
    header, rec = mapfile.read(GOLDEN)
    folder, out, field, cells_txt, path_txt = (str(tmp_path / x) for x in ("views", "seen.npz", "field.npz", "cells.txt", "path.txt"))
    os.makedirs(os.path.join(folder, "depth"))
    os.makedirs(os.path.join(folder, "rgb"))
    T2 = np.eye(4, dtype=F)
    T2[0, 3] = -2.0
    k = (16.0, 16.0, 31.5, 23.5, 0.1, 5.2)
    views, stamps = [], [(1.5, np.eye(4, dtype=F)), (2.5, T2)]
    with open(os.path.join(folder, "poses.txt"), "w") as f:
        f.write("".join(line + "\n" for line in vo.tum_lines(stamps)))
    with open(os.path.join(folder, "associate.txt"), "w") as f:
        for i, (ts, T) in enumerate(stamps):
            D = np.full((48, 64), 2.5 + 0.5 * i, F)
            D[:6] = 0.0
            name = "%.6f.png" % ts
            raw = np.rint(D * 5000.0).astype(np.uint16)
            Image.fromarray(raw).save(os.path.join(folder, "depth", name))
            Image.fromarray(np.zeros((48, 64, 3), np.uint8)).save(os.path.join(folder, "rgb", name))
            f.write("%.6f rgb/%s %.6f depth/%s\n" % (ts, name, ts, name))
            views.append((raw.astype(F) / F(5000.0), T, k))
    cam = ["--camera", "16", "16", "31.5", "23.5", "--zrange", "0.1", "5.2"]
    assert mapfile.main(["observe", GOLDEN, "--views", folder, "-o", out, "--pad", "2", "--radius", "2", "--margin", "0.125"] + cam) == 0
    lo, hi, _ = mapfile.bounds_records(rec)
    lo, n = mapfile.padded_box(lo, hi, 2)
    want = mapfile.observe_records(header["voxel"], lo, n, views, radius=2, margin=0.125)[0]
    seen, slo, voxel = mapfile.read_seen(out)
    assert seen.tobytes() == want.tobytes() and slo.tolist() == lo.tolist() and voxel == header["voxel"] and (seen & 0x7F).max() == 2
    assert mapfile.main(["esdf", GOLDEN, "-o", field, "--seen", out, "--clamp", "50"]) == 0
    d2, flo, _ = mapfile.read_field(field)
    assert d2.tobytes() == mapfile.known_field_records(rec, lo, n, want, clamp=50)[0].tobytes() and flo.tolist() == lo.tolist()
    assert mapfile.main(["frontiers", GOLDEN, "--seen", out, "-o", cells_txt]) == 0
    fr = mapfile.frontier_records(rec, lo, n, want)
    assert np.loadtxt(cells_txt, dtype=np.int64).reshape(-1, 3).tolist() == fr.tolist() and len(fr) > 0
    # plan --seen: from a free cell to a frontier cell through known space; a goal in unseen space is refused
    free = np.argwhere(mapfile.seen_free(want) & (mapfile.known_field_records(rec, lo, n, want)[0] >= 1)) + lo
    goal, start = [str(x) for x in fr[0]], [str(x) for x in free[len(free) // 2]]
    assert mapfile.main(["plan", GOLDEN, "--seen", out, "--goal"] + goal + ["--start"] + start + ["--clearance", "0.25", "-o", path_txt]) == 0
    cost, _, _, r2, info, paths = mapfile.plan_file(GOLDEN, [fr[0]], [free[len(free) // 2]], 0.25, seen=out)
    assert r2 == 1 and info["seeds_used"] == 1 and len(open(path_txt).read().splitlines()) == 1 + len(paths[0][0])
    unseen = np.argwhere(~mapfile.seen_known(want, 1, mapfile.solid_cells(rec, lo, n)[0]))[0] + lo
    assert mapfile.main(["plan", GOLDEN, "--seen", out, "--goal"] + [str(x) for x in unseen] + ["--start"] + start + ["--clearance", "0.25", "-o", path_txt]) == 1
    # a volume observed at another voxel edge is refused; so is a missing folder, and a missing -o is a usage error
    mapfile.write_seen(str(tmp_path / "other.npz"), want, lo, 0.5)
    assert mapfile.main(["esdf", GOLDEN, "-o", field, "--seen", str(tmp_path / "other.npz")]) == 1
    assert mapfile.main(["observe", GOLDEN, "--views", str(tmp_path / "nothing"), "-o", out]) == 1
    assert mapfile.main(["observe", GOLDEN, "--views", folder, "-o", out, "--radius", "4"] + cam) == 1
    assert mapfile.main(["frontiers", GOLDEN, "-o", cells_txt]) == 2
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------- the shared header --
def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "seen_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "seen_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def test_host_header(tmp_path):
    """revo_seen_host.h: every parameter rule and the defaults, the cell centres against the specification's float32 numbers,
    the byte update over every input, and the predicates against the specification's."""
    exe = _host(tmp_path)
    voxel = F(0.02)
    params = [(0, (9, 9, 9.0, 9.0)), (1, (0, 0, 0.0, 0.0)), (1, (3, 1, 0.5, 0.25)), (1, (4, 0, 0.1, 0.0)), (1, (-1, 0, 0.1, 0.0)),
              (1, (1, 2, 0.1, 0.0)), (1, (1, 0, -0.1, 0.0)), (1, (1, 0, np.nan, 0.0)), (1, (1, 0, np.inf, 0.0)), (1, (1, 0, 0.1, -1.0)),
              (1, (1, 0, 0.1, np.inf)), (1, (1, 0, 0.1, np.nan))]
    want_params = [(1, 0, voxel, F(0)), (0, 0, F(0), F(0)), (3, 1, F(0.5), F(0.25))] + [None] * 9
    rng = np.random.default_rng(24)
    cells = [(-(1 << 20), 0), ((1 << 20) - 1024, 1023), (0, 0), (-1, 0), (-3, 2)] + [tuple(int(x) for x in rng.integers(-5000, 5000, 2)) for _ in range(200)]
    updates = [(b, f, s) for b in range(256) for f in (0, 1, 2, 8, 63, 64) for s in (0, 1)]
    asks = [(so, b, mv, nb) for so in (0, 1) for b in (0, 1, 2, 0x7F, 0x80, 0x81, 0xFF) for mv in (0, 1, 2, 127, 128, 1 << 20) for nb in (0, 1, 6)]
    blob = struct.pack("<fI", voxel, len(params))
    for has, p in params:
        blob += struct.pack("<iiIff", has, *p)
    blob += struct.pack("<I", len(cells)) + b"".join(struct.pack("<ii", *c) for c in cells)
    blob += struct.pack("<I", len(updates)) + b"".join(struct.pack("<III", *u) for u in updates)
    blob += struct.pack("<I", len(asks)) + b"".join(struct.pack("<IIIi", *a) for a in asks)
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = (tmp_path / "out.bin").read_bytes()
    o = 0
    for want in want_params:
        good, o = out[o], o + 1
        assert good == (want is not None)
        if good:
            got, o = struct.unpack_from("<iIff", out, o), o + 16
            assert got[:2] == want[:2] and F(got[2]).tobytes() == want[2].tobytes() and F(got[3]).tobytes() == want[3].tobytes()
    got = np.frombuffer(out, "<f4", len(cells), o)
    o += 4 * len(cells)
    assert got.tobytes() == np.array([sr.centre((lo, 0, 0), (a, 0, 0), voxel)[0] for lo, a in cells], F).tobytes()
    got = np.frombuffer(out, np.uint8, len(updates), o)
    o += len(updates)
    assert got.tolist() == [sr.byte(*u) for u in updates]
    got = np.frombuffer(out, np.uint8, 4 * len(asks), o).reshape(-1, 4)
    assert o + 4 * len(asks) == len(out)
    for (so, b, mv, nb), g in zip(asks, got.tolist()):
        free, unknown = sr.is_free(b, mv), sr.is_unknown(bool(so), b, mv)
        assert g == [free, free or bool(b & 0x80), unknown, (not so) and free and nb > 0], (so, b, mv, nb)
